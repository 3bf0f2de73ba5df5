"""``GATResTrainer.fit`` at world size 2 on one GPU (fresh processes forked from conftest's fork server, gloo, eager launches,
like tests/test_gpu_two_ranks.py): the epoch's four sums are all-reduced, so both ranks take the SAME decision every epoch --
identical histories, bit-identical parameters, the same learning rate on the device -- although each rank's own validation
shard, taken alone, would have decided otherwise."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, PIPES = 388, 430
BS, EPOCHS, LR, PATIENCE, MIN_DELTA, SP = 4, 8, 5e-3, 3, 1e-3, 0


def _rank_main(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gnn_pressure_estimation_amd as G
        torch.cuda.set_device(0)
        ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
        snaps = G.wdn_synth.make_snapshots(2 * 3 * BS, NODES, seed=3) * 12.5 + 50.0
        mean, std = float(snaps.mean()), float(snaps.std(unbiased=False))
        rows = G.dp.shard_graphs(snaps.shape[0], rank, world)
        train = G.SnapshotStore(snaps[list(rows)], ei, device="cuda:0", mean=mean, std=std)
        # validation shards that differ in kind: rank 1's snapshots are far noisier than anything the model trains on
        val_raw = G.wdn_synth.make_snapshots(BS + 2, NODES, seed=40 + rank) * (12.5 if rank == 0 else 60.0) + 50.0
        val = G.SnapshotStore(val_raw, ei, device="cuda:0", mean=mean, std=std)
        torch.manual_seed(21 + rank)                                            # (rank 0's weights are broadcast)
        model = G.GATResMeanConv(num_blocks=4, nc=32).cuda()
        tr = G.GATResTrainer(model, train.edge_index(BS), BS * NODES, nodes_per_graph=[NODES] * BS, targets_are_inputs=True,
                             use_graph=False, lr=LR, seed=5)
        assert tr.world == world and tr.rank == rank
        local = []
        orig = G.dp.all_reduce_sums_

        def spy(sums, group=None):
            local.append(sums.clone().cpu())                                    # this rank's own four sums of the epoch
            return orig(sums, group)

        G.dp.all_reduce_sums_ = spy
        h = tr.fit(train, val, EPOCHS, batch_size=BS, patience=PATIENCE, min_delta=MIN_DELTA, scheduler_patience=SP,
                   generator=torch.Generator().manual_seed(7), val_seed=3)
        torch.cuda.synchronize()
        torch.save({"tr_loss": h.tr_loss, "val_loss": h.val_loss, "lr": h.lr, "improved": h.improved, "best_loss": h.best_loss,
                    "best_epoch": h.best_epoch, "stopped_epoch": h.stopped_epoch, "final_lr": h.final_lr,
                    "records": [r.tolist() for r in h.records], "params": model.flat_parameters.detach().cpu(),
                    "hp": tr.hp.cpu(), "host_lr": tr.hparams["lr"], "local": torch.stack(local), "faults": tr.fault_count,
                    "steps": tr.optimizer_step}, os.path.join(out_dir, f"r{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_all(procs, timeout=600):
    """Start, join, and never leave a child behind."""
    try:
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout)
        codes = [p.exitcode for p in procs]
        assert all(c == 0 for c in codes), f"rank processes failed or timed out (exit codes {codes})"
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
                if p.is_alive():
                    p.kill()
                    p.join(10)


def _decisions(pkg, val_losses):
    ctl = pkg.epoch_control.EpochController(LR, patience=PATIENCE, min_delta=MIN_DELTA, scheduler_patience=SP)
    out = []
    for v in val_losses:
        ctl.step(0.0, v)
        out.append((ctl.lr, ctl.stopped, ctl.improved))
        if ctl.stopped:
            break
    return out


def test_fit_at_world_size_two_takes_one_decision(pkg, tmp_path, fork_ctx):
    world = 2
    port = _free_port()
    _run_all([fork_ctx.Process(target=_rank_main, args=(r, world, port, str(tmp_path))) for r in range(world)])
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt") for r in range(world))
    n = len(r0["tr_loss"])
    # about the inputs: each rank's own validation loss, taken alone, leads the controller elsewhere
    own = [[float(l[2] / l[3]) for l in r["local"][:n]] for r in (r0, r1)]
    assert _decisions(pkg, own[0]) != _decisions(pkg, own[1])
    # ... and yet: one history, one set of parameters, one learning rate
    for k in ("tr_loss", "val_loss", "lr", "improved", "best_loss", "best_epoch", "stopped_epoch", "final_lr", "records", "steps"):
        assert r0[k] == r1[k], k
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["hp"], r1["hp"])
    assert r0["faults"] == r1["faults"] == 0
    assert float(r0["hp"][0]) == r0["final_lr"] == r0["host_lr"] == r1["host_lr"]
    # the decision is the mirror's on the all-reduced sums
    glob = r0["local"][:n] + r1["local"][:n]
    val = [float(g[2] / g[3]) for g in glob]
    assert val == r0["val_loss"] and [float(g[0] / g[1]) for g in glob] == r0["tr_loss"]
    dec = _decisions(pkg, val)
    assert [d[0] for d in dec][-1] == r0["final_lr"] and [d[2] for d in dec] == r0["improved"]
    assert (r0["stopped_epoch"] is not None) == dec[-1][1]
    assert r0["final_lr"] < LR                                                 # the rate dropped on the way
