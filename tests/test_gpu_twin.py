"""Undirected explanations on the MI355X: the HIP reverse-edge map (cal_edge_twin) and pair ranking (cal_explain_rank_pairs)
against the oracle and the host twins at every group size, at the LDS capacity and on the chunked path, their launch counts,
and the ``undirected`` keyword of explain / fidelity on engine-backed models."""
import argparse
import random

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch
from cal_amd.explain import _Layout, _log_probs, _untiled, edge_twins, explain, extract_subgraph, fidelity
from tests.test_twin import _Cols, _ungrouped, check_pairs, check_twins, same_bits
from tests.twin_oracle import make_batch, make_scores, pair_rank_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257]


def _both(sizes, seed, max_edges=None, ranking=True):
    """Device twins == oracle == host twins; then the three reduces of the pair ranking the same way."""
    ei, ptr, eptr = make_batch(sizes, seed=seed)
    twin = check_twins(ei, ptr, eptr, max_edges, dev=DEV)
    assert np.array_equal(twin, check_twins(ei, ptr, eptr, max_edges))
    if not ranking:
        return
    s, gt = make_scores(twin, seed=seed)
    for reduce, kw in (("mean", dict(k="gt")), ("max", dict(ratio=0.3)), ("min", dict(k=5))):
        d = check_pairs(s, eptr, twin, reduce, max_seg=max_edges, dev=DEV, gt=gt, **kw)
        h = check_pairs(s, eptr, twin, reduce, max_seg=max_edges, gt=gt, **kw)
        assert torch.equal(d[0], h[0]) and torch.equal(d[1], h[1]) and same_bits(d[3].numpy(), h[3].numpy())
        assert torch.allclose(d[2], h[2], atol=0, rtol=0, equal_nan=True)


@pytest.mark.parametrize("sizes", [SIZES, [0, 1, 2, 63, 64, 30, 17, 64, 5], [0, 1, 2, 65, 128, 127, 3]],
                         ids=["to-257", "four-per-workgroup", "two-per-workgroup"])
def test_hip_twin_group_sizes(sizes):
    _both(sizes, seed=len(sizes))


def test_hip_twin_at_the_lds_cap():
    assert int(_lib.query("cal_explain_lds_cap")) == 2048
    _both([2048, 5, 300, 1025], seed=2)


@pytest.mark.parametrize("sizes", [[5, 2049, 100], [70, 4500, 3, 2048]], ids=["two-chunks", "three-chunks"])
def test_hip_twin_chunked_segments(sizes):
    _both(sizes, seed=sizes[1])


def test_hip_twin_empty_batches_and_ties():
    empty = np.zeros((2, 0), dtype=np.int64)
    check_twins(empty, [0], [0], dev=DEV)                                         # B = 0
    check_twins(empty, [0, 3, 3], [0, 0, 0], dev=DEV)                             # E = 0
    check_pairs(np.zeros(0, dtype=np.float32), [0, 0, 0], np.zeros(0, dtype=np.int32), "mean", dev=DEV, k=1)
    ei, ptr, eptr = make_batch([40, 7, 130], seed=9)
    twin = check_twins(ei, ptr, eptr, dev=DEV)
    for reduce in ("mean", "max", "min"):                                         # every score tied: the column index decides
        check_pairs(np.full(len(twin), 0.5, dtype=np.float32), eptr, twin, reduce, dev=DEV, ratio=0.5)


def test_hip_twin_segment_longer_than_max_edges():
    _both([6, 300, 9, 64], seed=4, max_edges=64)
    _both([6, 2500, 9], seed=5, max_edges=2100)


def test_launch_counts_within_the_cap():
    ei, ptr, eptr = make_batch([2048, 5, 300], seed=2)
    data = _Cols(ei, ptr, eptr, dev=DEV)
    lay = _Layout(data)
    n0 = _lib.query("cal_launch_count")
    twin = lay.twins(data.edge_index)[0]
    n1 = _lib.query("cal_launch_count")
    assert n1 - n0 == 1                                                            # cal_edge_twin: one kernel
    s = torch.rand(ei.shape[1], device=DEV)
    lay.rank_edges(s, k=3)
    n2 = _lib.query("cal_launch_count")
    lay.rank_edge_pairs(s, data.edge_index, "mean", k=3)
    n3 = _lib.query("cal_launch_count")
    assert n2 - n1 == 1 and 0 < (n3 - n2) - (n2 - n1) <= 3                         # at most three beyond the rank launch
    assert twin.is_cuda


def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _model(name, deterministic=False):
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    torch.manual_seed(1)
    m = getattr(M, name)(10, 4, _args()).to(DEV)
    if deterministic:                                       # repeated forwards agree bit for bit: exact comparisons below
        object.__setattr__(m, "_engine", StepEngine(m, deterministic=True))
    return m


def _batch():
    return Batch.from_data_list(spmotif.train_mix(8, seed=3)).to(DEV)


def test_ungrouped_columns_agree_with_the_grouped_batch():
    m, b = _model("CausalGCN"), _batch()
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1)).to(DEV)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(E, device=DEV)
    twin = edge_twins(b)[0]
    f = _ungrouped(b, perm)
    assert torch.equal(edge_twins(f)[0].long(), inv[twin.long()[perm]])
    # (the foreign batch runs the engine's unfused route: scores agree to the 1e-4 test_gpu_explain.py allows between routes)
    ex, exf = explain(m, b, ratio=0.5, undirected="mean"), explain(m, f, ratio=0.5, undirected="mean")
    assert exf.edge_ptr is None and torch.equal(exf.edge_twin.long(), inv[twin.long()[perm]])
    assert torch.allclose(exf.edge_score, ex.edge_score[perm], atol=1e-4)
    assert torch.equal(exf.edge_mask, exf.edge_mask[exf.edge_twin.long()])
    assert torch.equal(exf.edge_mask.sum(), ex.edge_mask.sum())


@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
def test_model_explain_and_fidelity_undirected(name):
    m, b = _model(name, deterministic=True), _batch()
    node_gt, edge_gt = spmotif.ground_truth(b)
    d = explain(m, b, k="gt", edge_gt=edge_gt, node_gt=node_gt)
    ex = explain(m, b, k="gt", edge_gt=edge_gt, node_gt=node_gt, undirected="mean")
    twin, n_unp, _ = edge_twins(b)
    assert int(n_unp) == 0 and torch.equal(twin, ex.edge_twin)
    assert torch.equal(ex.edge_mask, ex.edge_mask[twin.long()]) and torch.equal(ex.edge_rank, ex.edge_rank[twin.long()])
    om, orank, omet, osym = pair_rank_oracle(d.edge_score.cpu().numpy(), ex.edge_ptr.cpu().numpy(), twin.cpu().numpy(), "mean",
                                             k="gt", gt=edge_gt.cpu().numpy())
    assert np.array_equal(ex.edge_mask.cpu().numpy(), om) and np.array_equal(ex.edge_rank.cpu().numpy(), orank)
    assert same_bits(ex.edge_score.cpu().numpy(), osym)
    met = ex.metrics["edge"].cpu().numpy()
    assert np.array_equal(met[:, :3], omet[:, :3])
    np.testing.assert_allclose(met[:, 3], omet[:, 3], atol=1e-12, rtol=0, equal_nan=True)
    assert torch.equal(ex.node_mask, d.node_mask)

    # fidelity: symmetric subgraphs on both sides, and the report of the same masks assembled here
    rep = fidelity(m, b, ratio=0.5, undirected="mean")
    ex = explain(m, b, ratio=0.5, undirected="mean")
    lay = _Layout(b)
    was = m.training
    m.eval()
    with torch.no_grad():
        full = _log_probs(m, _untiled(b, lay))
        y = b.y.view(-1)
        yhat = full.argmax(-1, keepdim=True)
        pf = full.gather(-1, yhat).exp()
        hits, gaps = [(yhat.squeeze(-1) == y).sum(-1)], []
        for comp in (False, True):
            sub = extract_subgraph(b, edge_mask=ex.edge_mask, complement=comp, relabel=False)
            t, unp, _ = edge_twins(sub)
            assert int(unp) == 0 and bool((t >= 0).all())
            lp = _log_probs(m, sub)
            hits.append((lp.argmax(-1) == y).sum(-1))
            gaps.append((pf - lp.gather(-1, yhat).exp()).sum((1, 2)))
    m.train(was)
    n = float(y.numel())
    for h, head in enumerate(("c", "o", "co")):
        for key, v in (("acc_full", hits[0]), ("acc_keep", hits[1]), ("acc_drop", hits[2]), ("fid_plus", gaps[1]),
                       ("fid_minus", gaps[0])):
            assert rep["%s_%s" % (key, head)] == v.double()[h].item() / n, (key, head)
    assert rep["sparsity"] == 1.0 - ex.edge_mask.sum().double().item() / float(ex.edge_mask.numel())
    assert rep["graphs"] == 8


@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
def test_undirected_calls_leave_the_state_untouched(name):
    from cal_amd.engine import StepEngine
    m = _model(name)
    m.train()
    eng = StepEngine(m, lr=1e-3)
    object.__setattr__(m, "_engine", eng)
    b = _batch()
    perm = torch.randperm(8, device=DEV)
    for _ in range(2):
        eng.train_step(b, perm, adam=True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    explain(m, b, ratio=0.3, undirected="max")
    fidelity(m, b, ratio=0.5, undirected="mean")
    assert m.engine() is eng and m.training
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    eng.train_step(b, perm, adam=True)                      # training goes on
    eng.check_status()
