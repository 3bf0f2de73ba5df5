"""fit_epoch(metric_fn_dict=..., device_metrics=True): the training metrics from the masked-metric moments launch inside
every step -- with the in-place epoch and the captured k-step sequences on -- leave training bit-identical and agree with
the host-metrics epoch."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NODES, PIPES = 388, 430


def make(pkg, S, bs, kseq, in_place):
    ei = pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    store = pkg.SnapshotStore(pkg.wdn_synth.make_snapshots(S, NODES, seed=3) * 12.5 + 50.0, ei, device="cuda:0")
    torch.manual_seed(21)
    model = pkg.GATResMeanConv(num_blocks=15, nc=32).cuda()
    tr = pkg.GATResTrainer(model, store.edge_index(bs), bs * NODES, nodes_per_graph=[NODES] * bs, targets_are_inputs=True)
    tr.epoch_graph_steps = kseq
    if not in_place:
        tr.epoch_copy_limit_bytes = 0          # the epoch goes through steps_rows sequences instead of the in-place copy
    return store, model, tr


@pytest.mark.parametrize("in_place", [True, False])
def test_device_metrics_leave_training_bit_identical_and_match_host_metrics(pkg, in_place):
    S, bs, kseq = 8 * 9 + 5, 8, 4              # 9 full batches (sequences of 4) and a ragged batch of 5
    fns = pkg.evaluation.get_metric_fn_collection("train")
    runs = {}
    for mode in ("none", "device", "host"):
        store, model, tr = make(pkg, S, bs, kseq, in_place)
        gen = torch.Generator().manual_seed(7)
        res = []
        for _ in range(2):
            if mode == "none":
                res.append(tr.fit_epoch(store, bs, generator=gen))
            elif mode == "device":
                res.append(tr.fit_epoch(store, bs, generator=gen, metric_fn_dict=fns, device_metrics=True))
            else:
                res.append(tr.fit_epoch(store, bs, generator=gen, metric_fn_dict=fns))
        torch.cuda.synchronize()
        runs[mode] = dict(res=res, params=model.flat_parameters.detach().clone(), m=tr.exp_avg.clone(),
                          v=tr.exp_avg_sq.clone(), graphs=tr.num_captured_graphs, buf=getattr(tr, "_epoch_buf", None),
                          ragged=5 in tr._siblings)
    none, dev, host = runs["none"], runs["device"], runs["host"]
    # the metrics epoch took the captured paths, the ragged sibling included
    assert dev["graphs"] > 0 and dev["ragged"]
    assert (dev["buf"] is not None) == in_place
    # training is untouched, bit for bit
    assert [r[0] for r in dev["res"]] == [r[0] for r in none["res"]]
    assert torch.equal(dev["params"], none["params"])
    assert torch.equal(dev["m"], none["m"]) and torch.equal(dev["v"], none["v"])
    # the host-metrics epoch trains on the same masks (same parameters after two epochs), so its metrics are comparable
    assert torch.equal(host["params"], none["params"])
    for (_, md), (_, mh) in zip(dev["res"], host["res"]):
        assert list(md) == list(fns)
        for k in fns:
            if math.isnan(mh[k]):
                assert math.isnan(md[k]), k
            else:
                assert md[k] == pytest.approx(mh[k], rel=1e-5, abs=1e-7), k
    assert dev["res"][0][1] != dev["res"][1][1]           # two epochs, two sets of metrics


def test_device_metrics_refuse_other_collections(pkg):
    store, model, tr = make(pkg, 16, 8, 4, True)
    with pytest.raises(ValueError, match="get_metric_fn_collection"):
        tr.fit_epoch(store, 8, device_metrics=True)
    fns = pkg.evaluation.get_metric_fn_collection("train")
    fns["train_mae"] = pkg.evaluation.calculate_rmse
    with pytest.raises(ValueError, match="get_metric_fn_collection"):
        tr.fit_epoch(store, 8, metric_fn_dict=fns, device_metrics=True)
