#!/usr/bin/env python3
"""Headline benchmark: training snapshots/sec of gatres_small on C-Town-shaped batches (BASELINE.json).

One "step" = one full reference training iteration (train.py:159-190) on one batch of `--batch-size` snapshots per
GPU: device mask sampling -> x[mask]=0 -> forward -> MSE on masked nodes -> backward -> [RCCL all-reduce] -> Adam,
replayed from a hipGraph.  Inputs (several batches, rotated) are resident in HBM before the timed region.

  python bench.py --gpus 1 --steps 200 --warmup 20
  python bench.py --gpus 8                      # starts 8 ranks itself (torch.distributed.run), before any GPU call
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

Protocol: W untimed warm-up steps, then `--repeats` (default 1) timed blocks of EXACTLY K steps,
each bracketed by a barrier + torch.cuda.synchronize() on both sides and reduced with MAX over ranks; `value` and
`ms_per_step` come from the MEDIAN block, min / max are reported beside it.  With the default, `--steps K` is the number of
timed steps of the run (`timed_steps` in the line).  Rank 0 prints ONE JSON line.
`--dump-outputs DIR`: after the timed blocks, what the timed path computed in its last step is written as DIR/<name>.npy
(see dump_outputs); the inputs are seeded, so two builds run with the same arguments can be compared output for output.
A plain run does only what the headline figure needs: set-up, warm-up, the timed blocks, the dump, the line.
`--full` adds everything else the benchmark measures or checks, each still subject to its `--no-*` switch: `roofline`
(live HIP-event timing of the kernels; for the per-op path the per-kernel table), `parity` against the oracle in the run,
`cpu_baseline` (the oracle on the host cores, up to 2 x --cpu-seconds) and, for the data-parallel step,
`config.collective` (the all-reduce timed over 20 eager steps).  `roofline.traffic` is measured in a `--full` run: before touching the GPU the
script runs itself twice as a child under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (a few seconds each;
`--no-live-pmc` skips them).
Data: synthetic (seeded WDN topology with C-Town's size, N(0,1) pressures, PyG-style random-init weights); the
reference's C-Town files are not shipped.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402   (importing torch does not initialise the GPU)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
# TEST-ONLY switches (tests/test_gpu_launcher.py drives `bench.py --gpus 2` end to end on the ONE GPU a test box has):
#   GATRES_DIST_BACKEND=gloo      process-group backend instead of nccl (= RCCL), which needs one GPU per rank
#   GATRES_BENCH_SHARE_GPU=1      every rank uses cuda:(local_rank % visible devices)
# A line produced under either says so in config.test_overrides; the driver never sets them.
DIST_BACKEND = os.environ.get("GATRES_DIST_BACKEND", "nccl")
SHARE_GPU = os.environ.get("GATRES_BENCH_SHARE_GPU", "") not in ("", "0")

MODELS = {"gatres_small": (15, 32), "gatres_large": (25, 128)}     # ConfigModels.py:22-42


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="gatres_small", choices=sorted(MODELS))
    ap.add_argument("--batch-size", type=int, default=32, help="snapshots per GPU per step")
    ap.add_argument("--nodes", type=int, default=388)
    ap.add_argument("--pipes", type=int, default=430)
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--per-op", action="store_true", help="one launch per stage instead of the fused per-snapshot kernel")
    ap.add_argument("--force-collective-path", action="store_true",
                    help="run the multi-GPU sequence (backward | RCCL all-reduce | Adam) even at world size 1")
    ap.add_argument("--fused-buckets", type=int, default=1, choices=[1, 2],
                    help="data-parallel step of the fused path: 1 = the single-GPU step's launches + ONE all-reduce of the flat "
                         "gradient + the Adam launch; 2 = the parameter gradients as two range launches, the upper blocks' bucket "
                         "on the wire under the lower blocks' launch (GATResTrainer.fused_buckets)")
    ap.add_argument("--host-batches", action="store_true",
                    help="batches start in pinned host memory: the timed step includes the H2D copy (PCIe-inclusive "
                         "rate for DESIGN.md; never the headline value)")
    ap.add_argument("--fused-adam", action="store_true",
                    help="with --drop-in: FusedAdam (one native launch) instead of torch.optim.Adam")
    ap.add_argument("--flat-adam", action="store_true",
                    help="with --drop-in: torch.optim.Adam(model.optimizer_parameters()) -- torch's own Adam on ONE flat leaf "
                         "parameter instead of the 124 named tensors (the optimizer line of train.py:348 changes, the loop body "
                         "does not)")
    ap.add_argument("--eval", action="store_true",
                    help="inference line instead of the training step: forward-only through the drop-in module under the "
                         "reference's Timer protocol (utils/timer.py:22-66: 10 warm-up calls, one event pair + synchronize per "
                         "call), test_time (ms/graph) and test_throughput (graphs/s) as evaluation.py:346-347 computes them")
    ap.add_argument("--drop-in", action="store_true",
                    help="time the reference loop body verbatim (train.py:160-188): nn.Module forward, loss.backward(), "
                         "torch.optim.Adam, host-side numpy mask, a fresh edge_index tensor every batch")
    ap.add_argument("--copy-batches", action="store_true",
                    help="stage every batch into the trainer's buffer (GATResTrainer.step(x, y): one more launch per step) "
                         "instead of training on the resident batches in place (bind_batches / step_bound)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure, everything else the benchmark measures or checks: the roofline (with "
                         "its rocprofv3 counter passes), in-run parity against the oracle, the CPU baseline, the all-reduce "
                         "timing of a data-parallel run; the --no-* switches below leave parts of it out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not run the two rocprofv3 --pmc child passes (FETCH_SIZE, WRITE_SIZE) that measure roofline.traffic "
                         "in this run; the committed counter file of the round is used instead (accepted only inside its "
                         "duration band)")
    ap.add_argument("--repeats", type=int, default=1, help="timed blocks of --steps steps; the median block is reported")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--shuffle-nodes", action="store_true",
                    help="randomly relabel the nodes of the synthetic topology (a junction order with no locality, as an "
                         "EPANET file may have): the plan's reverse Cuthill-McKee relabelling has to restore the row windows")
    ap.add_argument("--from-store", action="store_true",
                    help="batches come from a device-resident SnapshotStore through GATResTrainer.fit_epoch (shuffled row "
                         "gathers; the epoch loop of train.py:159-198) instead of pre-collated rotating batches")
    ap.add_argument("--graph-steps", type=int, default=20,
                    help="steps per hipGraph launch on the bound-batch path (GATResTrainer.steps_bound): every step is the full "
                         "iteration, consecutive steps share one graph launch; 1 = one launch per step")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                    help="storage / MFMA type of the projections (bf16: gatres_large per-op path, BASELINE config 3)")
    return ap.parse_args()


def self_launch(args):
    """`bench.py --gpus N` without a launcher: start N ranks with torch.distributed.run as a CHILD process (never exec a
    process that may have touched the GPU) and hand its output and exit code through."""
    n_dev = torch.cuda.device_count()                 # (counting devices does not initialise the GPU on this image)
    if n_dev < args.gpus and not SHARE_GPU:
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {n_dev} GPU(s) visible; refusing to report a smaller job")
    import socket
    with socket.socket() as s:                        # a free port (bind to 0), not one derived from the pid
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    log(f"no WORLD_SIZE in the environment: launching {args.gpus} ranks: {' '.join(cmd)}")
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


# ------------------------------------------------------------------------------------------------------------------
# per-kernel timing (HIP events on the launch stream) and algorithmic bytes -- DESIGN.md section 4
# ------------------------------------------------------------------------------------------------------------------
def kernel_table(G, model, plan, nc):
    """[(name, calls_per_step, algorithmic_bytes_per_launch, launcher)] for the kernels of one training step, through the
    typed per-op entry points of include/gatres.h in the model's storage type (s = 4 or 2 bytes per activation element)."""
    lib = G._native.load()
    N, Eg, E = plan.num_nodes, plan.num_edges_gat, plan.num_edges_mean
    nb = model.num_blocks
    dev = plan.device
    dt = int(model._cmodel.act_dtype)
    s = 2 if dt == G._native.DTYPE_BF16 else 4
    adt = torch.bfloat16 if dt == G._native.DTYPE_BF16 else torch.float32
    f = lambda *sh: torch.randn(*sh, dtype=torch.float32, device=dev)
    a = lambda *sh: torch.randn(*sh, dtype=torch.float32, device=dev).to(adt)          # activation-sized tensors
    st = lambda: G._native.current_stream(dev)
    S = int(lib.gatres_num_slabs(model._cmodel_ref(), N))
    rows = []

    def conv(tag, K, H):
        HC = H * nc
        x, W, Wt = a(N, K), a(HC, K), a(K, HC)
        att_s, att_d, bias = f(HC), f(HC), f(HC)
        h, a_s, a_d = a(N, HC), f(N, H), f(N, H)
        out, alpha = a(N, HC), torch.rand(Eg, H, device=dev)
        g_out, g_e, g_ad, g_as, g_h, g_x = a(N, HC), f(Eg, H), f(N, H), f(N, H), a(N, HC), a(N, K)
        slab = torch.empty(S * (HC * K + 3 * HC), device=dev)
        gp = plan.ref()
        idx = 4 * (N + 1) + 4 * Eg
        rows.append((f"proj_attn_fwd[{tag}]", nb, s * (N * K + HC * K + N * HC) + 4 * (2 * HC + 2 * N * H),
                     lambda: lib.gatres_t_proj_attn_fwd(x.data_ptr(), W.data_ptr(), att_s.data_ptr(), att_d.data_ptr(),
                                                        h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), N, K, H, nc, dt, st())))
        rows.append((f"gat_aggregate_fwd[{tag}]", nb,
                     idx + 4 * (Eg * H + N * H + HC + Eg * H) + s * (Eg * HC + N * HC),
                     lambda: lib.gatres_t_gat_aggregate_fwd(gp, h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(),
                                                            bias.data_ptr(), out.data_ptr(), alpha.data_ptr(), H, nc, 1,
                                                            dt, st())))
        rows.append((f"gat_aggregate_bwd_dst[{tag}]", nb,
                     idx + s * (N * HC + Eg * HC) + 4 * (Eg * H + Eg * H + N * H + Eg * H + N * H),
                     lambda: lib.gatres_t_gat_aggregate_bwd_dst(gp, g_out.data_ptr(), h.data_ptr(), alpha.data_ptr(),
                                                                a_s.data_ptr(), a_d.data_ptr(), g_e.data_ptr(),
                                                                g_ad.data_ptr(), H, nc, dt, st())))
        rows.append((f"gat_aggregate_bwd_src[{tag}]", nb,
                     4 * (N + 1) + 8 * Eg + s * (Eg * HC + N * HC) + 4 * (2 * Eg * H + N * H + 2 * HC + N * H),
                     lambda: lib.gatres_t_gat_aggregate_bwd_src(gp, g_out.data_ptr(), alpha.data_ptr(), g_e.data_ptr(),
                                                                g_ad.data_ptr(), att_s.data_ptr(), att_d.data_ptr(),
                                                                g_h.data_ptr(), g_as.data_ptr(), H, nc, dt, st())))
        rows.append((f"proj_bwd_dx[{tag}]", nb, s * (N * HC + HC * K + 3 * N * K),
                     lambda: lib.gatres_t_proj_bwd_dx(g_h.data_ptr(), Wt.data_ptr(), g_x.data_ptr(), x.data_ptr(),
                                                      g_x.data_ptr(), N, K, HC, dt, st())))
        # the weight partials and the attention-vector / bias column sums exactly as the step launches them: ONE co-launched
        # kernel where that form applies (gatres_t_conv_partials = model_driver.hip's conv_partials), else two launches
        Sw = 64 if (dt == G._native.DTYPE_BF16 and nc == 128 and S > 64) else S      # model_driver.hip: dw_slab_rows
        rows.append((f"conv_partials[{tag}]", nb,
                     s * (N * HC + N * K) + 4 * Sw * HC * K + s * 2 * N * HC + 4 * (2 * N * H + 3 * S * HC),
                     lambda: lib.gatres_t_conv_partials(g_h.data_ptr(), x.data_ptr(), slab.data_ptr() + 12 * HC, Sw,
                                                        HC * K + 3 * HC, N, K, HC, h.data_ptr(), g_as.data_ptr(),
                                                        g_ad.data_ptr(), g_out.data_ptr(), slab.data_ptr(),
                                                        slab.data_ptr() + 4 * HC, slab.data_ptr() + 8 * HC, S, H, nc, dt, st())))

    conv("conv1", nc, 2)
    conv("conv2", 2 * nc, 1)
    y, x0, o = a(N, nc), a(N, nc), a(N, nc)
    gp = plan.ref()
    rows.append(("mean_residual_relu_fwd", nb, 4 * (N + 1) + 4 * E + s * (E * nc + 2 * N * nc),
                 lambda: lib.gatres_t_mean_residual_relu_fwd(gp, y.data_ptr(), x0.data_ptr(), o.data_ptr(), nc, dt, st())))
    rows.append(("mean_bwd", nb, 8 * (N + 1) + 4 * E + s * (E * nc + N * nc),
                 lambda: lib.gatres_t_mean_bwd(gp, y.data_ptr(), o.data_ptr(), nc, dt, st())))
    return rows


def algorithmic_bytes_per_step(rows, N, nc, P, S, nb):
    """Compulsory-traffic model: every stage's inputs read once and outputs written once at
    full row width, no cache credit.  Returns (fused per-snapshot kernel, deferred parameter-gradient kernel): the
    dW / attention-vector gradient stages run in the second launch, the bias column sums stay in the first."""
    deferred = sum(r[1] * r[2] for r in rows if r[0].startswith(("proj_bwd_dw", "conv_param_grads", "conv_partials")))
    bias = nb * 4 * ((N * 2 * nc + S * 2 * nc) + (N * nc + S * nc))       # g_out tables read, slab rows written
    deferred -= bias
    stages = sum(r[1] * r[2] for r in rows) - deferred
    small = 4 * (N + 2 * N * nc) * 2 + 4 * (2 * N * nc + 2 * N) + 4 * 4 * N     # lin0 / lin1 (+bwd) / loss
    return stages + small, deferred


def survey_bytes_per_snapshot(nb, nc, n_g, e_g, s):
    """SURVEY.md section 8(d), "Algorithmic bytes per unit of work", restated term by term: per training SNAPSHOT, forward +
    backward, compulsory traffic (gathers at full row width, no cache credit); s = bytes per activation element, index
    words 4 B; N, E per snapshot, E' = E + N (self loops)."""
    N, E, Ep = n_g, e_g, e_g + n_g

    def gatconv(F, H, C, concat):
        HC, D = H * C, (H * C if concat else C)
        fwd_p = N * F * s + N * HC * s + 2 * N * H * s + F * HC * s
        fwd_a = 4 * (N + 1) + 4 * Ep + Ep * H * s + N * H * s + Ep * HC * s + N * D * s + Ep * H * s
        bwd_a = 12 * Ep + 8 * (N + 1) + Ep * HC * s + Ep * D * s + 3 * Ep * H * s + N * D * s + N * HC * s + 2 * N * H * s
        bwd_p = 2 * (N * HC * s + N * F * s) + 2 * F * HC * s
        return fwd_p + fwd_a + bwd_a + bwd_p, fwd_p + fwd_a

    (conv1, conv1_f), (conv2, conv2_f) = gatconv(nc, 2, nc, True), gatconv(2 * nc, 1, nc, False)
    mean_f = 4 * (N + 1) + 4 * E + E * nc * s + 2 * N * nc * s
    mean = 2 * mean_f
    lin = 6 * (N * s + N * nc * s)
    lin_f = 2 * (N * s + N * nc * s)                 # (lin0 reads x, writes [N, nc]; lin1 reads [N, nc], writes out)
    return dict(total=nb * (conv1 + conv2 + mean) + lin, conv1=conv1, conv2=conv2, mean_conv=mean, lin0_lin1=lin,
                forward=nb * (conv1_f + conv2_f + mean_f) + lin_f,
                inputs=dict(num_blocks=nb, nc=nc, N=N, E=E, E_prime=Ep, bytes_per_element=s, index_bytes=4))


# The figure SURVEY.md section 8(d) / BASELINE.md state for the headline config (gatres_small fp32 on a 388-node /
# 860-edge snapshot).  The formula above evaluates to 51.37 MB; the survey's table says 50.6 MB.  `roofline.achieved`
# uses the STATED (smaller) figure so that the fraction is never flattered; the formula value rides along.
SURVEY_STATED_BYTES = {("gatres_small", 388, 860, "fp32"): 50.6e6, ("gatres_large", 388, 860, "bf16"): 163e6}


PMC_FILE = "r06_fused_pmc_raw.json"      # written by tests/micro/profile_r06.sh from the round's own counter passes


LIVE_PMC = {}          # filled by live_pmc() before this process touches the GPU

DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs: ``arrays`` (name -> tensor) as ``d/<name>.npy``, float64 tensors as float64, everything else as float32.
    While all of them fit in DUMP_LIMIT_BYTES they are written whole; otherwise every array larger than an equal share of the
    limit is cut to a fixed sample of its flat entries (seeded by the array's name and size, sorted indices: the same entries
    in every run of the same arguments)."""
    import numpy as np
    import zlib
    os.makedirs(d, exist_ok=True)
    host = {k: v.detach().reshape(-1).cpu().numpy().astype(np.float64 if v.dtype == torch.float64 else np.float32)
            for k, v in arrays.items()}
    share = DUMP_LIMIT_BYTES // max(1, len(host))
    sampled = sum(a.nbytes for a in host.values()) > DUMP_LIMIT_BYTES
    for k, a in host.items():
        if sampled and a.nbytes > share:
            rng = np.random.default_rng(zlib.crc32(f"{k}:{a.size}".encode()))
            a = a[np.sort(rng.choice(a.size, share // a.itemsize, replace=False))]
        np.save(os.path.join(d, k + ".npy"), a)
    log(f"--dump-outputs: {', '.join(sorted(host))} -> {d}" + (" (sampled)" if sampled else ""))


def live_pmc(args):
    """roofline.traffic MEASURED IN THIS RUN: two child passes of this very command under ``rocprofv3 --pmc FETCH_SIZE`` and
    ``--pmc WRITE_SIZE`` (separate passes, the program directly behind ``--``, as MI355X_MICROARCH.md prescribes), started
    BEFORE this process initialises the GPU (a process that has must not start GPU children on this pool), each bounded by a
    timeout.  Returns {kernel substring: {counter: mean KB per launch}} or a reason string."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return "rocprofv3 not found"
    kernels = ("gatres_window_kernel", "param_grads_reg_kernel")
    out = {k: {} for k in kernels}
    base = ["--steps", "20", "--warmup", "5", "--repeats", "1", "--no-cpu-baseline", "--no-roofline", "--model", args.model,
            "--batch-size", str(args.batch_size), "--nodes", str(args.nodes), "--pipes", str(args.pipes),
            "--graph-steps", str(args.graph_steps)]
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="gatres_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                   os.path.abspath(__file__)] + base
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp", GATRES_BENCH_CHILD="1"),
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
            if r.returncode != 0:
                return f"the rocprofv3 --pmc {counter} child pass exited with {r.returncode}"
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return f"the rocprofv3 --pmc {counter} child pass left no counter file"
            acc = {}
            for path in files:
                for row in csv.DictReader(open(path)):
                    if row.get("Counter_Name") != counter:
                        continue
                    for k in kernels:
                        if k in row.get("Kernel_Name", ""):
                            key = (k, path, row.get("Dispatch_Id"))
                            acc[key] = acc.get(key, 0.0) + float(row["Counter_Value"])      # (one row per XCD: summed)
            for k in kernels:
                vals = [v for (kk, _, _), v in acc.items() if kk == k]
                if not vals:
                    return f"no {k} launch in the {counter} pass"
                out[k][counter] = sum(vals) / len(vals)
                out[k]["launches"] = len(vals)
        except subprocess.TimeoutExpired:
            return f"the rocprofv3 --pmc {counter} child pass timed out"
        except Exception as e:      # noqa: BLE001
            return f"live counter pass failed ({type(e).__name__}: {e})"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return out


def pmc_traffic(args, us_main, us_second):
    """HBM-side bytes per step of the two heavy launches from the committed rocprofv3 --pmc passes of THIS round
    (profiles/r06_fused_pmc_raw.json: FETCH_SIZE and WRITE_SIZE collected in separate runs of this script, KB per launch;
    FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for wide coalesced reads on gfx950), plus the wait counters of the
    dominant kernel.  Only for the workload they were taken on, and only while the kernels still are the kernels that were
    counted: the file records each kernel's average duration in the profiled run, and a file whose figures differ from
    this run's live HIP-event durations by more than 5 % (dominant kernel; 10 % for the second launch, see below) is REFUSED
    (traffic = null, the reason in traffic_source) -- no falling back to another round's file."""
    live_data = LIVE_PMC.get("data")
    if isinstance(live_data, dict):
        live = live_data
        b = lambda c: int((2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024)
        main_b, pg_b = b(live["gatres_window_kernel"]), b(live["param_grads_reg_kernel"])
        wait = None
        try:      # (the wait / issue ratios still come from the round's SQ counter pass: they are evidence, not a roofline input)
            with open(os.path.join(ROOT, "profiles", PMC_FILE)) as f:
                wait = json.load(f).get("wait")
        except Exception:      # noqa: BLE001
            pass
        src = (f"MEASURED IN THIS RUN: two child passes of this command under rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE before "
               f"the timed run (mean over {live['gatres_window_kernel']['launches']} launches of the window kernel), 2 x FETCH + WRITE "
               f"per launch, window kernel + parameter-gradient launch")
        return main_b + (pg_b if us_second is not None else 0), src, wait, (pg_b if us_second is not None else None)
    if args.model != "gatres_small" or args.batch_size != 32 or args.nodes != 388 or args.per_op or args.shuffle_nodes:
        return None, "no counter passes were taken for this workload" + (f" ({live_data})" if isinstance(live_data, str) else ""), None, None
    path = os.path.join(ROOT, "profiles", PMC_FILE)
    try:
        with open(path) as f:
            raw = json.load(f)
        rec = [raw["kernel_avg_us"], (raw.get("second_kernel") or {}).get("kernel_avg_us")]
    except Exception as e:      # noqa: BLE001
        return None, f"profiles/{PMC_FILE} unusable ({type(e).__name__}: {e})", None, None
    # (the second launch is timed back to back here, 36.8 - 37.3 us, and inside the step by rocprof, 38.7 - 39.4 us with the
    # window kernel's tables freshly evicted from L2: the same kernel reads 4 - 7 % apart between the two set-ups, so its
    # band is 10 %; the dominant kernel, which carries 3/4 of the traffic, stays at 5 %)
    for what, live, was, tol in (("dominant kernel", us_main, rec[0], 0.05),
                                 ("parameter-gradient launch", us_second, rec[1], 0.10)):
        if live is None or was is None:
            continue
        if abs(live - was) > tol * was:
            return None, (f"profiles/{PMC_FILE} REFUSED: its {what} averaged {was:.1f} us in the profiled run, this run "
                          f"measures {live:.1f} us (> {int(tol * 100)} % apart): the counters describe other kernels; rerun "
                          f"tests/micro/profile_r06.sh"), None, None
    val = int((2.0 * raw["FETCH_SIZE"]["mean_counter_value_KB"] + raw["WRITE_SIZE"]["mean_counter_value_KB"]) * 1024)
    sk = raw.get("second_kernel")
    val_second = None
    if sk:           # the parameter gradients (+ update) run as a launch of their own: both launches, like counted_us
        val_second = int((2.0 * sk["FETCH_SIZE"]["mean_counter_value_KB"] + sk["WRITE_SIZE"]["mean_counter_value_KB"]) * 1024)
        val += val_second
    src = ((f"live counter passes unavailable ({live_data}); " if isinstance(live_data, str) else "") +
           f"profiles/{PMC_FILE}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, 2 x FETCH + WRITE "
           f"per launch{' (window kernel + parameter-gradient launch)' if sk else ''}; a committed constant, NOT measured in "
           f"this run; accepted because the recorded kernel durations ({rec[0]:.1f}"
           f"{'' if rec[1] is None else ' + %.1f' % rec[1]} us) agree with this run's within 5 % (dominant kernel) / 10 % (second launch)")
    return val, src, raw.get("wait"), val_second


def time_fused(G, trainer, device, reps=50):
    """Average duration of the fused per-snapshot kernel (forward + loss + backward in ONE launch), HIP events on
    the launch stream."""
    import ctypes as C
    lib = G._native.load()
    m, plan = trainer.model, trainer.plan
    L = trainer
    PH = 2 | 16 | 4
    lp = torch.zeros(8 * plan.num_segments + 1, dtype=torch.float32, device=device)
    gref = plan.ref(m._cmodel_ref())          # (the struct that carries the part tables of this model's split)
    args = (m._cmodel_ref(), gref, m.flat_parameters.data_ptr(), L.x.data_ptr(), L.mask.data_ptr(),
            L.y.data_ptr(), L.out.data_ptr(), L.g_out.data_ptr(), lp.data_ptr(), None, L.saved.data_ptr(),
            L.scratch.data_ptr(), PH)
    st = lambda: G._native.current_stream(device)
    G._native.check(lib.gatres_fused_prepare_backward(m._cmodel_ref(), gref, m.flat_parameters.data_ptr(),
                                                      L.scratch.data_ptr(), st()), "prepare")
    for _ in range(5):
        G._native.check(lib.gatres_fused_run(*args, st()), "fused_run")
    torch.cuda.synchronize(device)

    def avg_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(device))
        for _ in range(reps):
            fn()
        e1.record(torch.cuda.current_stream(device))
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    pg = (m._cmodel_ref(), gref, L.saved.data_ptr(), L.scratch.data_ptr())
    second = lambda: lib.gatres_fused_param_grads(*pg, st())          # (the step's second launch)
    G._native.check(second(), "param_grads")
    return avg_us(lambda: lib.gatres_fused_run(*args, st())), avg_us(second)


def time_kernels(rows, device, reps=200):
    out = []
    for name, calls, nbytes, fn in rows:
        for _ in range(10):
            rc = fn()
            assert rc == 0, (name, rc)
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(device))
        for _ in range(reps):
            fn()
        e1.record(torch.cuda.current_stream(device))
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        gbs = nbytes / us * 1e-3
        # `gbs` prices ALGORITHMIC bytes (every gathered neighbour row at full width, no cache credit): for the sparse kernels
        # most of those bytes are served by L2, so the figure is an L2-SIDE rate and can exceed the HBM peak; it is not a
        # roofline fraction.  The HBM-side rate of the same kernels (FETCH_SIZE / WRITE_SIZE counters) is attached to the line
        # as `hbm_side_rates` where a counter file of this round exists for the workload.
        out.append(dict(kernel=name, calls_per_step=calls, avg_us=us, algorithmic_bytes=nbytes, gbs=gbs,
                        gbs_kind="L2-side (algorithmic bytes, gathers at full row width, no cache credit)",
                        exceeds_hbm_peak=bool(gbs > HBM_PEAK_GBS)))
    return out


PEROP_PMC_FILES = {("gatres_large", 128, 388, "bf16"): "r06_large_ctown_bs128_bf16_pmc.json"}


def hbm_side_rates(args):
    """Counter-based HBM-side traffic of the per-op kernels ((2 x FETCH_SIZE + WRITE_SIZE) x 1024 bytes per launch, separate
    rocprofv3 --pmc passes of this command, tests/micro/profile_r06.sh) over their rocprof average durations: what HBM (or
    the Infinity Cache in front of it) physically moved, per kernel symbol -- beside the L2-side `gbs` of the kernel table."""
    name = PEROP_PMC_FILES.get((args.model, args.batch_size, args.nodes, args.dtype))
    if name is None:
        return None
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            raw = json.load(f)
        out = {}
        for sym, c in raw["mean_per_launch"].items():
            if "FETCH_SIZE" in c and "WRITE_SIZE" in c and c.get("avg_us"):
                nbytes = (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0
                out[sym] = {"hbm_bytes_per_launch": int(nbytes), "avg_us": c["avg_us"],
                            "hbm_gbs": round(nbytes / c["avg_us"] * 1e-3, 1),
                            "hbm_frac_of_peak": round(nbytes / c["avg_us"] * 1e-3 / HBM_PEAK_GBS, 4)}
        return {"source": f"profiles/{name} (a committed constant of this round, NOT measured in this run)", "kernels": out}
    except Exception as e:      # noqa: BLE001
        return {"source": f"profiles/{name} unusable ({type(e).__name__}: {e})", "kernels": {}}


def in_run_parity(args, nb, nc, device):
    """BASELINE.md section 3 / north_star: "predicted node pressures match the reference CPU path within 1e-5 relative on
    identical snapshots ... in the same run".  The SAME batch (wdn_synth.make_batch, its host mask), the SAME seed-3
    parameters and the SAME loop body (train.py:174-188) go through the oracle on the host and through the benchmarked
    trainer configuration (same kernels, same plan, hipGraph replay) on the GPU; reported: max-abs error over max-abs value
    of the predictions, the loss and the flat gradient of that step.  The checker is the oracle -- a restatement of the
    PyG algorithm that is itself NOT pinned against PyG output: "parity unpinned"."""
    from oracle import gatres_oracle as O
    import gnn_pressure_estimation_amd as G
    x, y, ei, mask = G.wdn_synth.make_batch(args.batch_size, args.nodes, args.pipes)
    p = O.init_params(nb, nc, seed=3)
    ref = O.OracleTrainer(p)
    l_ref, o_ref = ref.step(x.clone(), y, ei, mask)
    model = G.GATResMeanConv(num_blocks=nb, nc=nc)
    sd = {}
    for k, v in p.items():
        sd[k] = v
        if k.endswith("lin_src.weight"):
            sd[k.replace("lin_src", "lin_dst")] = v
    model.load_state_dict(sd)
    model = model.to(device)
    if args.dtype == "bf16":
        model.set_compute_dtype("bf16")
    tr = G.GATResTrainer(model, ei.to(device), x.shape[0], nodes_per_graph=[args.nodes] * args.batch_size,
                         use_graph=not args.no_graph, fused=not args.per_op)
    loss = tr.step(x.to(device), y.to(device), mask.to(device))
    torch.cuda.synchronize(device)

    def rel(a, b):
        a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    return {"out_rel": rel(tr.out, o_ref), "loss_rel": rel(loss, l_ref), "grad_rel": rel(tr.grads, ref.flat("grads")),
            "tolerance": {"out_rel": 1e-5 if args.dtype == "fp32" else None, "note": "north_star: 1e-5 relative fp32"},
            "checker": "oracle/gatres_oracle.py (torch-CPU restatement of the PyG 2.3 path; parity unpinned: never held "
                       "to PyG output)",
            "sample": f"one full training step on make_batch(bs={args.batch_size}) with its host mask, seed-3 parameters, "
                      f"the benchmarked trainer configuration"}


def cpu_baseline(args, nb, nc):
    """The oracle (a torch-CPU restatement of the PyG path; PyG itself is not installable here) timed on the host
    cores for the same step: at the benchmark's batch size (like for like) and at bs = 8 (BASELINE.json config 1, the
    reference's own CPU-runnable case).  A bounded sample: about --cpu-seconds of CPU work per leg."""
    from oracle import gatres_oracle as O
    import gnn_pressure_estimation_amd as G
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1

    def leg(bs, seconds, cores=None):
        x, y, ei, mask = G.wdn_synth.make_batch(bs, args.nodes, args.pipes)
        tr = O.OracleTrainer(O.init_params(nb, nc, seed=3))
        # These are ~2400 tiny ops per step: an OpenMP team as wide as a 256-thread host makes every one of them
        # slower, so the thread count is chosen by a short calibration (one step each) and reported as `cores`.
        cands = sorted({c for c in (8, 16, 32) if c <= avail} or {avail})
        if cores is None:
            torch.set_num_threads(cands[0])
            tr.step(x, y, ei, mask)                           # warm-up (thread pool, autograd graph)
            best = None
            for c in cands:
                torch.set_num_threads(c)
                t0 = time.perf_counter()
                tr.step(x, y, ei, mask)
                dt1 = time.perf_counter() - t0
                log(f"cpu baseline calibration (bs {bs}): {c} threads -> {dt1:.3f} s/step")
                if best is None or dt1 < best:
                    best, cores = dt1, c
        torch.set_num_threads(cores)
        for _ in range(2):
            tr.step(x, y, ei, mask)
        t0, n = time.perf_counter(), 0
        while n < 5 or (time.perf_counter() - t0 < seconds and n < 200):
            tr.step(x, y, ei, mask)
            n += 1
        dt = time.perf_counter() - t0
        return bs * n / dt, cores, n, cands

    v, cores, n, cands = leg(args.batch_size, args.cpu_seconds)
    out = dict(value=v, unit="snapshots/s", cores=cores, kind="port",
               sample=f"{n} full training steps (mask->fwd->MSE->bwd->Adam) of {args.model} on one "
                      f"bs={args.batch_size} batch after warm-up, torch {torch.__version__} CPU ops, {cores} threads "
                      f"(best of {cands} on a host with {avail} hardware threads)")
    if args.batch_size != 8:
        v8, c8, n8, _ = leg(8, min(args.cpu_seconds, 8.0))
        out["config1_bs8"] = dict(value=v8, unit="snapshots/s", cores=c8,
                                  sample=f"{n8} steps at batch_size=8 (BASELINE.json configs[0]: the reference's own "
                                         f"CPU case; synthetic C-Town-shaped batch, the oracle standing in for PyG)")
    return out


def drop_in_loop(args, G, model, topo, device, nb, nc):
    """The reference's loop body on the drop-in module (single GPU): what a user gets by only swapping the import."""
    import numpy as np
    if args.fused_adam:
        opt = G.FusedAdam(model, lr=5e-4, weight_decay=6e-6)
    elif args.flat_adam:
        opt = torch.optim.Adam(model.optimizer_parameters(), lr=5e-4, weight_decay=6e-6)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=5e-4, weight_decay=6e-6)
    crit = torch.nn.MSELoss()
    bs, npg = args.batch_size, args.nodes
    snaps = G.wdn_synth.make_snapshots(8 * bs, npg, seed=100)
    ei_cpu = G.wdn_synth.collate_edge_index(topo, npg, bs)
    rng = np.random.RandomState(0)

    def step(i):
        opt.zero_grad()
        y = G.wdn_synth.collate_snapshots(snaps, range((i % 8) * bs, (i % 8 + 1) * bs))
        x, yd, ei = y.clone().to(device), y.to(device), ei_cpu.clone().to(device)       # train.py:162-164
        batch_mask = G.wdn_synth.generate_batch_mask([npg] * bs, 0.95, rng)             # auxil.py:166-182
        x[batch_mask] = 0
        out = model(x, ei, None, None)
        loss = crit(out[batch_mask], yd[batch_mask])
        loss.backward()
        opt.step()
        step.out = out.detach()
        return float(loss)                                                               # train.py:190 (sync)

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for i in range(args.steps):
        last = step(i)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"loss": torch.tensor([last], dtype=torch.float64), "out": step.out,
                                         "params": torch.cat([p.detach().reshape(-1) for p in model.parameters()])})
    print(json.dumps({"metric": "train snapshots/sec", "value": bs * args.steps / dt, "unit": "snapshots/s", "n_gpus": 1,
                      "steps": args.steps, "timed_steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                      "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                      "data": "synthetic",
                      "config": {"workload": f"{args.model}, drop-in nn.Module + "
                                             f"{'FusedAdam' if args.fused_adam else 'torch.optim.Adam on the flat parameter' if args.flat_adam else 'torch.optim.Adam'} + host numpy mask, "
                                             f"reference loop body verbatim (train.py:160-190), batch_size={bs}",
                                 "final_loss": last}}))


def eval_loop(args, G, model, topo, device, nb, nc):
    """The reference's inference measurement (evaluation.py:298,324-347) on the drop-in module: every batch is one call of
    ``Timer.auto_measure(model)(x1, edge_index, None, None)`` under ``torch.no_grad()`` -- 10 untimed warm-up calls, then one
    event pair and a synchronize per call -- and the two figures the reference reports, ``test_time`` (mean milliseconds per
    graph) and ``test_throughput`` (graphs per second), from the Timer's own formulas.  Roofline: the FORWARD share of
    SURVEY.md 8(d)'s bytes per snapshot over the mean event-pair duration of a call."""
    import numpy as np
    bs, npg = args.batch_size, args.nodes
    model.eval()
    ei = G.wdn_synth.collate_edge_index(topo, npg, bs).to(device)
    snaps = G.wdn_synth.make_snapshots(8 * bs, npg, seed=100)
    rng = np.random.RandomState(0)
    timer = G.evaluation.Timer()
    n_batches = max(args.steps, 1)
    t0 = time.perf_counter()
    with torch.no_grad():
        for i in range(n_batches):
            y = G.wdn_synth.collate_snapshots(snaps, range((i % 8) * bs, (i % 8 + 1) * bs)).to(device)
            mask = G.wdn_synth.generate_batch_mask([npg] * bs, 0.95, rng)                 # evaluation.py:312-317
            x1 = y.clone()
            x1[mask] = 0
            out = timer.auto_measure(model, bs, 10)(x1, ei, None, None)                   # evaluation.py:321-323
    wall = time.perf_counter() - t0
    n_graphs = n_batches * bs
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"out": out})
    # The reference's two figures, by its own formulas (utils/timer.py:43-66).  Both carry a quirk of that file: compute_time
    # divides the sum of (batch time x graphs in the batch) by the NUMBER OF GRAPHS, which is the mean time of a BATCH, and
    # compute_throughput divides (batches x batch size) by that mean batch time in seconds -- N times the rate at which graphs
    # are processed.  They are reported as the reference would print them; `value` is the plain rate: graphs / summed call time.
    ms_graph, thr = timer.compute_time(n_graphs), timer.compute_throughput(n_graphs)
    ms_call = float(np.mean(timer.timings))
    rate = n_graphs / (float(np.sum(timer.timings)) * 1e-3)
    sb = survey_bytes_per_snapshot(nb, nc, npg, 2 * args.pipes, 2 if args.dtype == "bf16" else 4)
    ach = sb["forward"] * bs / (ms_call * 1e-3) * 1e-9
    assert bool(torch.isfinite(out).all())
    print(json.dumps({"metric": "inference graphs/sec (forward only, Timer protocol)", "value": rate, "unit": "graphs/s", "n_gpus": 1,
                      "steps": n_batches, "timed_steps": n_batches, "warmup": 10, "ms_per_step": ms_call, "higher_is_better": True, "scaling": "weak",
                      "vs_baseline": None, "dtype": "bf16" if args.dtype == "bf16" else "f32", "data": "synthetic",
                      "reference_figures": {"test_time (evaluation.py:346, timer.py:43-51)": ms_graph,
                                            "test_throughput (evaluation.py:347, timer.py:53-66)": thr,
                                            "note": "as the reference computes them: test_time is the mean milliseconds of a BATCH "
                                                    "(weighted by graph count), test_throughput is batches x batch_size / that time"},
                      "ms_per_graph": ms_call / bs,
                      "ms_per_call": {"mean": ms_call, "min": float(np.min(timer.timings)), "max": float(np.max(timer.timings))},
                      "wall_graphs_per_s_incl_host": n_graphs / wall,
                      "config": {"workload": f"{args.model} ({nb} blocks, nc={nc}), forward only, drop-in nn.Module under "
                                             f"torch.no_grad(), {npg}-node WDN, batch_size={bs}, {args.dtype}; Timer protocol of "
                                             f"utils/timer.py:22-66 (10 warm-up calls, one event pair + synchronize per call)"},
                      "roofline": {"bound": "hbm", "kernel": "forward launch(es) of one model call",
                                   "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                                   "traffic": None, "algorithmic_bytes_per_snapshot": sb["forward"],
                                   "bytes_per_snapshot_source": "forward terms of the SURVEY.md 8(d) formula"}}))


def main():
    args = parse()
    nb, nc = MODELS[args.model]
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args)                                  # (does not return)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: the job that runs must be the job that is reported")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if (args.full and world == 1 and rank == 0
            and not (args.no_roofline or args.no_live_pmc or args.per_op or args.drop_in or args.eval
                     or args.force_collective_path or args.dtype == "bf16" or args.model != "gatres_small")
            and not os.environ.get("GATRES_BENCH_CHILD") and torch.cuda.device_count() > 0):
        # (device_count() does not initialise the GPU on this image; the child passes must come before anything that does)
        log("two rocprofv3 --pmc child passes (FETCH_SIZE, WRITE_SIZE) for roofline.traffic ...")
        t0 = time.perf_counter()
        LIVE_PMC["data"] = live_pmc(args)
        log(f"... {time.perf_counter() - t0:.0f} s: " + (LIVE_PMC["data"] if isinstance(LIVE_PMC["data"], str) else "ok"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP engine has no CPU path")
    # host-side tensor ops here are tiny (collation, masks): a 256-wide OpenMP team makes each of them ~20 ms
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    device = torch.device("cuda", local_rank % max(torch.cuda.device_count(), 1) if SHARE_GPU else local_rank)
    torch.cuda.set_device(device)
    if world > 1 or args.force_collective_path:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if DIST_BACKEND == "nccl":
            torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            torch.distributed.init_process_group(DIST_BACKEND, rank=rank, world_size=world)
        if torch.distributed.get_world_size() != args.gpus:
            raise SystemExit(f"{torch.distributed.get_world_size()} ranks joined, --gpus {args.gpus} were asked for")

    import gnn_pressure_estimation_amd as G
    torch.manual_seed(3 + rank)            # replicas start DIFFERENT on purpose: the trainer broadcasts rank 0's parameters
    model = G.GATResMeanConv(name=args.model, num_blocks=nb, nc=nc).to(device)
    if args.dtype == "bf16":
        if not hasattr(model, "set_compute_dtype"):
            raise SystemExit("--dtype bf16: the bf16 projection path is not built in this tree")
        model.set_compute_dtype("bf16")
    N = args.nodes * args.batch_size
    topo = G.wdn_synth.make_wdn_topology(args.nodes, args.pipes, seed=0)
    if args.shuffle_nodes:
        g = torch.Generator().manual_seed(12345)
        topo = torch.randperm(args.nodes, generator=g)[topo]
    ei = G.wdn_synth.collate_edge_index(topo, args.nodes, args.batch_size).to(device)
    if args.drop_in:
        return drop_in_loop(args, G, model, topo, device, nb, nc)
    if args.eval:
        return eval_loop(args, G, model, topo, device, nb, nc)
    trainer = G.GATResTrainer(model, ei, N, nodes_per_graph=[args.nodes] * args.batch_size, seed=1000,
                              use_graph=not args.no_graph, fused=not args.per_op,
                              force_collective_path=args.force_collective_path,
                              targets_are_inputs=True)        # synthetic snapshots: y is x before masking
    trainer.fused_buckets = args.fused_buckets
    nbatches = 8
    snaps = G.wdn_synth.make_snapshots(nbatches * args.batch_size, args.nodes, seed=100 + rank).to(device)
    batches = [snaps[i * args.batch_size:(i + 1) * args.batch_size].reshape(-1).contiguous() for i in range(nbatches)]
    store = None
    if args.from_store:
        # one epoch of the store == one timed block of --steps steps
        store = G.SnapshotStore(G.wdn_synth.make_snapshots(args.steps * args.batch_size, args.nodes, seed=100 + rank),
                                topo, device=device)
    if args.host_batches:
        batches = [b.cpu().pin_memory() for b in batches]
        trainer.prefetch_batch(batches[0])
    G_ = max(1, args.graph_steps)

    def chunks(k):                                  # the bound-batch indices of k consecutive steps, G_ per graph launch
        return [tuple((i0 + j) % nbatches for j in range(min(G_, k - i0))) for i0 in range(0, k, G_)]

    if not (args.host_batches or args.copy_batches):
        # the captured steps read the resident batches in place (no staging copy); every graph the run will replay -- single
        # steps and the multi-step sequences of the warm-up and of a timed block -- is captured here, before any timing
        seqs = sorted({c for c in chunks(args.steps) + chunks(args.warmup) if len(c) > 1})
        trainer.bind_batches(batches, sequences=seqs)

    def one_step(i):
        if args.host_batches:                       # batch i was prefetched during step i - 1; start fetching i + 1
            trainer.step_prefetched()               # (trains on the staging slot in place: no device copy, mask sampled ahead)
            trainer.prefetch_batch(batches[(i + 1) % nbatches])
        elif args.copy_batches:                     # device-resident batch through the reference-shaped call (train.py:159-190):
            b = batches[i % nbatches]               # staged into the trainer's own buffer by one extra launch
            trainer.step(b, b)
        else:
            trainer.step_bound(i % nbatches)

    bound_path = not (args.host_batches or args.copy_batches or args.from_store)

    def run_steps(k):
        if bound_path and G_ > 1:
            for c in chunks(k):
                trainer.steps_bound(c) if len(c) > 1 else trainer.step_bound(c[0])
        else:
            for i in range(k):
                one_step(i)

    def fence():
        torch.cuda.synchronize(device)
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(device)


    def timed_block(k):
        fence()
        t0 = time.perf_counter()
        if store is not None:
            trainer.fit_epoch(store, args.batch_size, shuffle=True)
        else:
            run_steps(k)
        fence()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=device)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    log(f"model/trainer ready on {device}; warm-up {args.warmup} steps")
    run_steps(args.warmup)
    if store is not None:
        trainer.fit_epoch(store, args.batch_size, shuffle=True)      # (untimed: captures the epoch's k-step sequence, steps_rows)
    # Every hipGraph the timed steps replay exists BEFORE the first timed block, whatever --warmup is: bind_batches() captured
    # the steady-state step of every (batch, mask buffer) pair (GATResTrainer.precapture_bound).  Checked, not assumed: the
    # number of captured graphs must not move across the timed blocks (block 1 used to hold four captures).
    graphs_before = trainer.num_captured_graphs
    times = [timed_block(args.steps) for _ in range(max(1, args.repeats))]
    graphs_after = trainer.num_captured_graphs
    if bound_path and not args.no_graph and graphs_after != graphs_before:
        raise SystemExit(f"bench.py: {graphs_after - graphs_before} hipGraph capture(s) happened INSIDE the timed region "
                         f"({graphs_before} -> {graphs_after} graphs): the measurement is invalid")
    dt = statistics.median(times)
    if args.dump_outputs and rank == 0:
        # the state the last timed step left, before anything below launches more work on the trainer
        torch.cuda.synchronize(device)
        dump_outputs(args.dump_outputs, {"loss": trainer.loss, "out": trainer.out, "mask": trainer.mask, "grads": trainer.grads,
                                         "params": model.flat_parameters, "adam_exp_avg": trainer.exp_avg,
                                         "adam_exp_avg_sq": trainer.exp_avg_sq})
    coll = None
    if args.full and trainer.split and trainer.reducer is not None and trainer.reducer.active and trainer._one_piece():
        # what the all-reduce itself takes: 20 more steps as EAGER launches with an event pair around the collective (events
        # inside a captured step cannot be read); untimed, after the timed blocks
        was = trainer.use_graph
        trainer.use_graph = False
        trainer.reducer.time_collective = True
        for i in range(20):
            trainer.step_bound(i % nbatches) if bound_path else one_step(i)
        ms = trainer.reducer.collective_ms()
        trainer.reducer.time_collective = False
        trainer.use_graph = was
        if ms:
            coll = {"all_reduce_us_mean": 1e3 * sum(ms) / len(ms), "all_reduce_us_min": 1e3 * min(ms), "all_reduce_us_max": 1e3 * max(ms),
                    "samples": len(ms), "bytes": 4 * trainer.P,
                    "how": "event pair on the launch stream around the synchronous all-reduce of the flat gradient, eager steps "
                           "after the timed blocks (rank 0)"}
    loss = float(trainer.loss.item())
    log(f"timed {len(times)} x {args.steps} steps: median {dt:.4f}s (min {min(times):.4f}, max {max(times):.4f}), loss {loss:.5f}")
    # GATRES_BENCH_TIMING_ONLY=1: probe builds of the library that give WRONG results on purpose (tests/micro/ab_libs.sh); the line
    # then says so in config.timing_only and is never a result
    timing_only = os.environ.get("GATRES_BENCH_TIMING_ONLY", "") not in ("", "0")
    if (not (loss == loss) or loss > 1e6) and not timing_only:
        raise SystemExit(f"training diverged (loss={loss}; dropped steps: {trainer.fault_count})")
    dropped = trainer.fault_count + trainer.dropped_steps
    if dropped > 0 and not timing_only:
        # a dropped step did no work: a rate that counts it would be inflated.  The per-snapshot kernel needs its whole grid
        # co-resident (one workgroup per CU); on a shared / partitioned / CU-masked device partners time out instead.
        raise SystemExit(f"bench.py: {dropped} training step(s) were DROPPED (a split launch gave up waiting for a partner "
                         f"workgroup: is the GPU shared?): refusing to report a rate")

    lib = G._native.load()
    cus = lib.gatres_fused_cus_per_segment(model._cmodel_ref(), trainer.plan.ref()) if trainer.fused else 0
    window = bool(lib.gatres_fused_window_kernel(model._cmodel_ref(), trainer.plan.ref())) if trainer.fused else False
    per_snap = lambda t: world * args.batch_size * args.steps / t
    result = {
        "metric": "train snapshots/sec", "value": per_snap(dt), "unit": "snapshots/s",
        "n_gpus": world, "steps": args.steps, "timed_steps": args.steps * len(times), "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" if args.dtype == "bf16" else "f32", "data": "synthetic",
        "repeats": {"blocks": len(times), "statistic": "median", "ms_per_step_min": min(times) / args.steps * 1e3,
                    "ms_per_step_max": max(times) / args.steps * 1e3, "value_min": per_snap(max(times)),
                    "value_max": per_snap(min(times))},
        "config": {"workload": f"{args.model} ({nb} blocks, nc={nc}), C-Town-sized WDN ({args.nodes} nodes, "
                               f"{2 * args.pipes} directed edges{', randomly relabelled nodes' if args.shuffle_nodes else ''}), "
                               f"batch_size={args.batch_size} per GPU, {args.dtype}, "
                               f"full training step (device mask 0.95 -> fwd -> masked MSE -> bwd -> "
                               f"{'RCCL all-reduce -> ' if trainer.split else ''}Adam), "
                               f"{'per-op kernels' if not trainer.fused else f'fused per-snapshot kernel ({cus} CUs per snapshot, ' + ('row-window' if window else 'whole-segment') + ' tables)'}, "
                               f"{'eager launches' if args.no_graph else 'hipGraph replay' + (f' ({G_} steps per graph launch)' if bound_path and G_ > 1 else '')}"
                               f"{', batches from SnapshotStore.fit_epoch' if store is not None else ''}"
                               f"{', batches staged by copy' if args.copy_batches else ''}",
                   "global_batch": world * args.batch_size, "parallelism": f"dp{world}",
                   "plan_relabelled": trainer.plan.perm_host is not None, "row_window": trainer.plan.window_rows(cus) if cus >= 2 else None,
                   "fused_buckets": trainer.fused_buckets if trainer.split else None, "collective": coll,
                   "dropped_steps": dropped, "final_loss": loss,
                   "captured_graphs": graphs_after, "captures_in_timed_region": graphs_after - graphs_before},
    }
    if timing_only:
        result["config"]["timing_only"] = "GATRES_BENCH_TIMING_ONLY=1: a probe build with wrong results; NOT a measurement of the product"
        result["config"]["final_loss"] = None if loss != loss else loss
    if DIST_BACKEND != "nccl" or SHARE_GPU:
        result["config"]["test_overrides"] = {"backend": DIST_BACKEND, "ranks_share_gpu": SHARE_GPU}

    if rank == 0 and args.full and not args.no_roofline:
        sb = survey_bytes_per_snapshot(nb, nc, args.nodes, 2 * args.pipes, 2 if args.dtype == "bf16" else 4)
        stated = SURVEY_STATED_BYTES.get((args.model, args.nodes, 2 * args.pipes, args.dtype))
        unit_bytes = stated if stated is not None else sb["total"]
        table = kernel_table(G, model, trainer.plan, nc)
        if trainer.fused:
            log("timing the fused per-snapshot kernel ...")
            nbytes_model, nbytes_pg = algorithmic_bytes_per_step(table, N, nc, trainer.P, trainer.plan.num_segments, nb)
            us, us_pg = time_fused(G, trainer, device)
            inline_pg = us_pg < 10.0         # a no-op call: the deferred gradients ran on consumer workgroups of the same launch
            if inline_pg:
                nbytes_model += nbytes_pg
            # achieved = algorithmic bytes per snapshot x snapshots per launch / the launch's duration.  The
            # survey's per-snapshot figure covers the whole step; when the deferred parameter gradients run as a second
            # launch their time is added (one "launch" = everything that carries the snapshot's forward + backward).
            us_all = us + (0.0 if inline_pg else us_pg)
            # what the parameter-gradient items stream (k_fused_dev.h: param_grads_item_reg): per (block, conv) g_h [N, HC],
            # x [N, K], g_a_src / g_a_dst [N, H] read once, one slab row block [HC, K + 2] written per segment
            S_ = trainer.plan.num_segments
            pg_streamed = nb * 4 * ((N * (2 * nc + nc + 4) + S_ * 2 * nc * (nc + 2)) + (N * (nc + 2 * nc + 2) + S_ * nc * (2 * nc + 2)))
            nbytes = unit_bytes * args.batch_size
            traffic, traffic_source, wait, traffic_pg = pmc_traffic(args, us, None if inline_pg else us_pg)
            result["roofline"] = {"bound": "hbm", "kernel": ("gatres_window_kernel" if window else "gatres_fused_kernel") +
                                                            " (forward + loss + backward, one launch)",
                                  "achieved": nbytes / us_all * 1e-3, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": nbytes / us_all * 1e-3 / HBM_PEAK_GBS, "traffic": traffic,
                                  "traffic_source": traffic_source,
                                  # what HBM physically moved (counter bytes / counted_us): `achieved` above prices the
                                  # ALGORITHMIC bytes of SURVEY 8(d), most of which the kernel serves from LDS / L2
                                  "hbm_measured_gbs": None if traffic is None else traffic / us_all * 1e-3,
                                  "hbm_measured_frac": None if traffic is None else traffic / us_all * 1e-3 / HBM_PEAK_GBS,
                                  "limiter": "latency",
                                  "limiter_evidence": (wait or "the dominant kernel is a chain of dependent stages on every CU "
                                                       "(DESIGN.md section 3.1); no counter file accepted for this run"),
                                  "avg_launch_us": us, "counted_us": us_all,
                                  "counted_us_note": "frac = algorithmic bytes / counted_us / peak; counted_us = avg_launch_us of the "
                                                     "dominant kernel + second_kernel.avg_launch_us when the deferred parameter "
                                                     "gradients run as a launch of their own",
                                  "algorithmic_bytes_per_launch": nbytes,
                                  "algorithmic_bytes_per_snapshot": unit_bytes,
                                  "bytes_per_snapshot_source": ("SURVEY.md 8(d) / BASELINE.md stated figure" if stated is not None
                                                                else "SURVEY.md 8(d) formula"),
                                  "survey_formula": sb,
                                  "frac_with_formula_bytes": sb["total"] * args.batch_size / us_all * 1e-3 / HBM_PEAK_GBS,
                                  "frac_of_step_time": unit_bytes * args.batch_size / (dt / args.steps * 1e6) * 1e-3 / HBM_PEAK_GBS,
                                  "per_op_byte_model": {"algorithmic_bytes_per_launch": nbytes_model,
                                                        "frac": nbytes_model / us * 1e-3 / HBM_PEAK_GBS,
                                                        "note": "round-1 accounting (slab partials, index reads, per-op "
                                                                "intermediates): fatter than SURVEY 8(d); kept for comparison only"},
                                  "second_kernel": None if inline_pg else
                                  {"kernel": "param_grads_reg_kernel (deferred dW / att gradients)",
                                   "avg_launch_us": us_pg, "algorithmic_bytes_per_launch": nbytes_pg,
                                   "achieved": nbytes_pg / us_pg * 1e-3,
                                   # NOT a roofline fraction: the per-op byte model prices conv_partials' reads of h and g_out
                                   # (attention-vector and bias gradients); this launch forms the attention-vector gradients from
                                   # T = [g_a]^T x without reading h and finds the bias partials in the part slabs, so it moves
                                   # the bytes below -- its own rate is hbm_side_gbs
                                   "achieved_kind": "per-op byte model over the launch's duration (may exceed the HBM peak: the "
                                                    "launch does not read the h tables the model prices)",
                                   "exceeds_hbm_peak": nbytes_pg / us_pg * 1e-3 > HBM_PEAK_GBS,
                                   "streamed_bytes_per_launch": pg_streamed,
                                   "streamed_gbs": pg_streamed / us_pg * 1e-3,
                                   "hbm_side_bytes_per_launch": traffic_pg,
                                   "hbm_side_gbs": None if traffic_pg is None else traffic_pg / us_pg * 1e-3}}
        else:
            log("per-kernel timing ...")
            rows = time_kernels(table, device)
            for r in rows:
                r["step_share_us"] = r["avg_us"] * r["calls_per_step"]
            dom = max(rows, key=lambda r: r["step_share_us"])
            # Per-op configurations: the step is some hundred launches, so the ONE roofline figure is SURVEY 8(d)'s algorithmic
            # bytes per snapshot x batch over the whole STEP time (`frac` == `frac_of_step_time`).  The per-kernel `gbs` of the
            # kernel table are L2-side rates (see time_kernels) and are not roofline fractions.
            step_us = dt / args.steps * 1e6
            ach = unit_bytes * args.batch_size / step_us * 1e-3
            result["roofline"] = {"bound": "hbm", "kernel": f"whole step ({sum(r['calls_per_step'] for r in rows)} launches of the "
                                                            f"kernel table + slab reductions); largest share: {dom['kernel']}",
                                  "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                                  "traffic": None, "traffic_source": None, "avg_launch_us": dom["avg_us"],
                                  "counted_us": step_us,
                                  "algorithmic_bytes_per_launch": unit_bytes * args.batch_size,
                                  "algorithmic_bytes_per_snapshot": unit_bytes, "survey_formula": sb,
                                  "frac_of_step_time": ach / HBM_PEAK_GBS,
                                  "dominant_kernel": {k: dom[k] for k in ("kernel", "avg_us", "calls_per_step", "gbs", "gbs_kind")}}
            result["kernels"] = [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()} for r in rows]
            hs = hbm_side_rates(args)
            if hs is not None:
                result["hbm_side_rates"] = hs
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        result["parity"] = in_run_parity(args, nb, nc, device)
        log(f"in-run parity vs the oracle: {result['parity']['out_rel']:.2e} (out) {result['parity']['loss_rel']:.2e} (loss) "
            f"{result['parity']['grad_rel']:.2e} (grad)")
        result["cpu_baseline"] = cpu_baseline(args, nb, nc)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if rank == 0:
        # RCCL writes a version banner to the C-level stdout buffer; push it out first so that the JSON line is the LAST line
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(result), flush=True)
        if (world > 1 or args.force_collective_path) and not os.environ.get("GATRES_BENCH_NO_HARD_EXIT"):
            os._exit(0)           # (nothing may follow the JSON line: skip exit handlers that print, e.g. RCCL's; a profiler
                                  #  that writes its files at exit needs GATRES_BENCH_NO_HARD_EXIT=1)


if __name__ == "__main__":
    main()
