"""Kernel time of the staging launches (csrc/k_stage.hip), symbol by symbol, for a kernel trace of the process.

Every staging symbol is launched ``--launches`` times in a row on raw device buffers (no store, no trainer, so the script runs
against any checkout that exports the symbols: ``--root <checkout>``), at the project's own size -- 388 nodes, batch 32, 20
sensors, rate 0.95 -- and at 387 nodes, where source rows and destination graphs fall on changing 16-byte phases; the
multi-network symbols with two networks (388 and 150 nodes, 16 graphs each).  Nothing else touches the device between the
first and the last launch, and the cases run in the order of ``CASES``, so the staging kernels of the trace, in start order,
are the cases' launches in that order.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o kt -- python tests/micro/stage_cost.py [--root <checkout>]
    python tests/micro/stage_cost.py --summarize <dir> [--label parent]

``--summarize`` needs no device: it cuts the trace's staging kernels into the cases and prints one JSON line per case (kernel
name, launches, average / median / minimum in microseconds).  The same kernel serves several symbols (``mask_generate_kernel``
served three before k_stage.hip), which is why the averages are taken per case and not from the stats table.  Not collected by
pytest.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BS, SENSORS, RATE, SNAPSHOTS, SEED = 32, 20, 0.95, 256, 9
SIZES = (388, 387)
MULTI_NETS, MULTI_EACH, GATHER_BATCHES = (388, 150), 16, 8
STAGING_KERNELS = ("mask_generate_kernel", "stage_rows_mask", "stage_multi_rows_mask_kernel", "gather_multi_rows_kernel")
CASES = [f"{sym}@{n}" for n in SIZES for sym in ("mask_generate", "stage_batch_mask", "stage_rows_mask", "stage_rows_mask_required:0",
                                                 f"stage_rows_mask_required:{SENSORS}", "stage_rows_mask_sensors:0,1",
                                                 "stage_rows_mask_sensors:0.1,0.7")]
CASES += ["stage_multi_rows_mask_required@388+150", "gather_multi_rows@388+150"]


def launch(G, args):
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    lib = G._native.load()
    gen = torch.Generator().manual_seed(1)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    calls = {}
    keep = []
    for n in SIZES:
        data = torch.randn(SNAPSHOTS, n, generator=gen).to(dev)
        rows = torch.randperm(SNAPSHOTS, generator=gen)[:BS].to(dev)
        xs, x, y = (torch.randn(BS * n, generator=gen).to(dev) for _ in range(3))
        mask = torch.empty(BS * n, dtype=torch.uint8, device=dev)
        ptr = torch.arange(0, (BS + 1) * n, n, dtype=torch.int32, device=dev)
        obs = torch.randperm(n, generator=gen)[:SENSORS].sort().values.to(torch.int32).to(dev)
        keep += [data, rows, xs, x, y, mask, ptr, obs]
        D, R, X, M, P, C, O = (t.data_ptr() for t in (data, rows, x, mask, ptr, ctr, obs))
        calls[f"mask_generate@{n}"] = lambda P=P, M=M, C=C: lib.gatres_mask_generate(P, BS, RATE, SEED, C, M, None)
        calls[f"stage_batch_mask@{n}"] = lambda XS=xs.data_ptr(), X=X, n=n, P=P, M=M, C=C: lib.gatres_stage_batch_mask(
            XS, None, X, None, BS * n, P, BS, RATE, SEED, C, M, None)
        calls[f"stage_rows_mask@{n}"] = lambda D=D, R=R, n=n, X=X, P=P, M=M, C=C: lib.gatres_stage_rows_mask(
            D, R, n, X, None, P, BS, RATE, SEED, C, M, None)
        for r in (0, SENSORS):
            calls[f"stage_rows_mask_required:{r}@{n}"] = lambda D=D, R=R, n=n, X=X, P=P, M=M, C=C, O=O, r=r: \
                lib.gatres_stage_rows_mask_required(D, R, n, X, None, P, BS, RATE, SEED, C, O if r else None, r, M, None)
        for drop, share in ((0.0, 1.0), (0.1, 0.7)):
            calls[f"stage_rows_mask_sensors:{drop:g},{share:g}@{n}"] = lambda D=D, R=R, n=n, X=X, P=P, M=M, C=C, O=O, drop=drop, share=share: \
                lib.gatres_stage_rows_mask_sensors(D, R, n, X, None, P, BS, O, SENSORS, drop, share, RATE, SEED, C, M, None)
    mats = [torch.randn(SNAPSHOTS, n, generator=gen).to(dev) for n in MULTI_NETS]
    table = torch.tensor([m.data_ptr() for m in mats], dtype=torch.int64, device=dev)
    sizes = [n for n in MULTI_NETS for _ in range(MULTI_EACH)]
    nog = torch.tensor([k for k in range(len(MULTI_NETS)) for _ in range(MULTI_EACH)], dtype=torch.int32, device=dev)
    ptr = torch.tensor([0] + [sum(sizes[:i + 1]) for i in range(len(sizes))], dtype=torch.int32, device=dev)
    total = sum(sizes)
    rows = torch.randint(0, SNAPSHOTS, (GATHER_BATCHES * len(sizes),), generator=gen).to(dev)
    x = torch.empty(GATHER_BATCHES * total, device=dev)
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    keep += [mats, table, nog, ptr, rows, x, mask]
    T, NG, R, P, X, M, C = (t.data_ptr() for t in (table, nog, rows, ptr, x, mask, ctr))
    calls["stage_multi_rows_mask_required@388+150"] = lambda: lib.gatres_stage_multi_rows_mask_required(
        T, len(MULTI_NETS), NG, R, P, len(sizes), X, None, RATE, SEED, C, None, None, M, None)
    calls["gather_multi_rows@388+150"] = lambda: lib.gatres_gather_multi_rows(
        T, len(MULTI_NETS), NG, R, P, len(sizes), GATHER_BATCHES, X, total, None)
    assert list(calls) == CASES, (list(calls), CASES)
    torch.cuda.synchronize()                     # (every torch kernel of the set-up lies before the first staging kernel)
    for name in CASES:
        for _ in range(args.launches):
            assert calls[name]() == 0, name
    torch.cuda.synchronize()
    import socket
    print(json.dumps({"launched": CASES, "launches_each": args.launches, "label": args.label, "host": socket.gethostname(),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def summarize(args):
    files = sorted(glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"want one *kernel_trace.csv under {args.summarize}, found {files}")
    rows = [r for r in csv.DictReader(open(files[0])) if any(k in r["Kernel_Name"] for k in STAGING_KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(CASES) * args.launches:
        raise SystemExit(f"{len(rows)} staging kernels in the trace, want {len(CASES)} x {args.launches}")
    for i, name in enumerate(CASES):
        part = rows[i * args.launches:(i + 1) * args.launches]
        kernels = sorted({r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for r in part})
        if len(kernels) != 1:
            raise SystemExit(f"{name}: its launches are not one kernel: {kernels}")
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part[args.skip:]]     # (the first ones load code)
        print(json.dumps({"case": name, "label": args.label, "kernel": kernels[0], "launches": len(us),
                          "avg_us": round(statistics.fmean(us), 3), "median_us": round(statistics.median(us), 3),
                          "min_us": round(min(us), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--skip", type=int, default=20, help="--summarize: launches of each case left out of its figures (warm-up)")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="change")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    sys.path.insert(0, os.path.abspath(args.root))
    import gnn_pressure_estimation_amd as G
    launch(G, args)


if __name__ == "__main__":
    main()
