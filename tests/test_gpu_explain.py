"""Causal-subgraph explanations on the MI355X: the HIP ranking (cal_explain_rank) against the numpy oracle and the host
twin at the LDS capacity's bounds and beyond, engine-backed explain() against the fp64 oracle's soft masks on every
route, the operator-level path, state left untouched after training steps, and eval_explanation's aggregation."""
import argparse
import random

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif, synth
from cal_amd.data import Batch
from cal_amd.explain import eval_explanation, explain, rank_segments
from oracle import cal_oracle as O
from tests.explain_oracle import rank_oracle
from tests.helpers import random_graph_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATT_TOL = 1e-4


def _cap():
    return int(_lib.query("cal_explain_lds_cap"))


def _both(score, sizes, k=None, ratio=None, gt=None, stride=1):
    """HIP ranking == numpy oracle (masks, ranks bit for bit; metrics 1e-12) == host twin."""
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.long)
    max_seg = max(sizes) if len(sizes) else 0
    s = torch.as_tensor(score, dtype=torch.float32)
    g = None if gt is None else torch.as_tensor(gt, dtype=torch.bool)
    if stride == 2:
        sd = torch.stack([torch.zeros_like(s), s], 1).to(DEV)[:, 1]
    else:
        sd = s.to(DEV)
    dm, dr, dmet = rank_segments(sd, seg.to(DEV), max_seg, k=k, ratio=ratio, gt=None if g is None else g.to(DEV), metrics=True)
    hm, hr, hmet = rank_segments(s, seg, max_seg, k=k, ratio=ratio, gt=g, metrics=True)
    om, orank, omet = rank_oracle(s.numpy(), seg.numpy(), k=k, ratio=ratio, gt=None if g is None else g.numpy())
    assert np.array_equal(dr.cpu().numpy(), orank)
    assert np.array_equal(dm.cpu().numpy(), om)
    np.testing.assert_allclose(dmet.cpu().numpy(), omet, atol=1e-12, rtol=0, equal_nan=True)
    assert torch.equal(dr.cpu(), hr) and torch.equal(dm.cpu(), hm)
    assert torch.allclose(dmet.cpu(), hmet, atol=0, rtol=0, equal_nan=True)


@pytest.mark.parametrize("which", ["cap-1", "cap", "cap+1", "20000"])
def test_hip_rank_at_the_lds_bounds(which):
    S = _cap()
    m = {"cap-1": S - 1, "cap": S, "cap+1": S + 1, "20000": 20000}[which]
    rng = np.random.default_rng(m)
    sizes = [m, 3, m // 2 + 1]
    M = sum(sizes)
    gt = rng.random(M) < 0.1
    s = np.round(rng.standard_normal(M) * 64) / 64               # ties
    s[rng.random(M) < 0.01] = np.nan
    _both(s, sizes, ratio=0.1, gt=gt)
    _both(s, sizes, k="gt", gt=gt, stride=2)
    _both(np.full(M, 0.5), sizes, k=17, gt=gt)


def test_hip_rank_mixed_and_packed_segments():
    rng = np.random.default_rng(7)
    sizes = [0, 1, 5, 20000, 2, 0, 300, 4097, 31]
    M = sum(sizes)
    gt = rng.random(M) < 0.2
    _both(rng.standard_normal(M).astype(np.float32), sizes, k=10, gt=gt)
    sizes = [28 + int(v) for v in rng.integers(0, 6, 128)]            # 128 graphs of ~30 nodes: packed groups
    M = sum(sizes)
    gt = rng.random(M) < 0.3
    for kw in (dict(k=0), dict(k=7), dict(ratio=0.5), dict(k="gt")):
        _both(np.round(rng.standard_normal(M) * 4) / 4, sizes, gt=gt, **kw)
    _both(np.zeros(0), [0, 0], k=1)


def _args(**kw):
    d = dict(layers=3, hidden=128, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _gpu_model(name, feat, ncls, args, seed=0):
    from cal_amd import model as M
    torch.manual_seed(seed)
    sd = O.init_state(name, feat, ncls, hidden=args.hidden, layers=args.layers, heads=4, cat_or_add=args.cat_or_add)
    m = getattr(M, name)(feat, ncls, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")          # (GINConv's eps buffers are not part of the oracle's state)
    return m.to(DEV), sd


def _check_against_oracle(name, m, sd, b, args, ratio=0.3):
    bd = b.to(DEV)
    eng = m.engine()
    assert eng is not None
    ex = explain(m, bd, ratio=ratio)
    x = (b.x if b.x is not None else b.feat).cpu().double()
    sd64 = {k: v.double() for k, v in sd.items()}
    kw = {}
    if name == "CausalGCN":
        kw = dict(without_edge_attention=args.without_edge_attention, without_node_attention=args.without_node_attention)
    _, inter = O.causal_forward(name, sd64, x, b.edge_index.cpu(), b.batch.cpu(), layers=args.layers, heads=4,
                                cat_or_add=args.cat_or_add, num_graphs=int(b.num_graphs), return_intermediates=True, **kw)
    es, ns = ex.edge_score.cpu().double(), ex.node_score.cpu().double()
    assert (es - inter["edge_att"][:, 1]).abs().max().item() <= ATT_TOL
    assert (ns - inter["node_att"][:, 1]).abs().max().item() <= ATT_TOL
    if kw.get("without_edge_attention"):
        assert (ex.edge_score == 0.5).all()
    if kw.get("without_node_attention"):
        assert (ex.node_score == 0.5).all()
    ptr = ex.ptr.cpu().numpy()
    om, orank, _ = rank_oracle(ex.node_score.cpu().numpy(), ptr, ratio=ratio)
    assert np.array_equal(ex.node_mask.cpu().numpy(), om) and np.array_equal(ex.node_rank.cpu().numpy(), orank)
    eptr = ex.edge_ptr.cpu().numpy()
    om, orank, _ = rank_oracle(ex.edge_score.cpu().numpy(), eptr, ratio=ratio)
    assert np.array_equal(ex.edge_mask.cpu().numpy(), om) and np.array_equal(ex.edge_rank.cpu().numpy(), orank)
    return ex


@pytest.mark.parametrize("name,node_num,B,kw", [
    ("CausalGCN", 7, 128, {}),                                  # headline: packed tiles
    ("CausalGCN", 15, 32, {}),                                  # 230-247-node graphs: wide routes
    ("CausalGAT", 7, 64, {}),
    ("CausalGIN", 7, 64, {}),
    ("CausalGCN", 7, 64, {"cat_or_add": "cat"}),
    ("CausalGCN", 7, 64, {"without_edge_attention": True}),
    ("CausalGCN", 15, 16, {"without_node_attention": True}),
])
def test_engine_explain_matches_oracle(name, node_num, B, kw):
    args = _args(**kw)
    m, sd = _gpu_model(name, 10, 4, args)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=node_num, seed=11))
    _check_against_oracle(name, m, sd, b, args)


def test_engine_explain_self_loops_and_small_graphs():
    args = _args(layers=2, hidden=64)
    for name in ("CausalGCN", "CausalGAT"):
        m, sd = _gpu_model(name, 6, 4, args)
        b = random_graph_batch(num_graphs=12, n_lo=3, n_hi=40, feat=6, seed=4, self_loops=True)
        assert bool((b.edge_index[0] == b.edge_index[1]).any())
        _check_against_oracle(name, m, sd, b, args)


def test_engine_explain_big_graphs():
    args = _args(layers=2, hidden=64)
    m, sd = _gpu_model("CausalGCN", 10, 4, args)
    b = Batch.from_data_list(synth.ba_graphs(3, n=5000, seed=1))
    _check_against_oracle("CausalGCN", m, sd, b, args, ratio=0.05)


def test_engine_path_equals_operator_path():
    args = _args(layers=2, hidden=64)
    for name in ("CausalGCN", "CausalGAT"):
        m, _ = _gpu_model(name, 10, 4, args)
        b = Batch.from_data_list(spmotif.train_mix(48, seed=5)).to(DEV)
        a = explain(m, b, k=8)
        m.use_engine = False
        c = explain(m, b, k=8)
        m.use_engine = True
        assert (a.edge_score - c.edge_score).abs().max().item() <= ATT_TOL
        assert (a.node_score - c.node_score).abs().max().item() <= ATT_TOL


def test_explain_after_training_leaves_the_engine_state_untouched():
    from cal_amd.engine import StepEngine
    args = _args(layers=2, hidden=64)
    m, _ = _gpu_model("CausalGCN", 10, 4, args)
    m.train()
    eng = StepEngine(m, lr=1e-3)
    object.__setattr__(m, "_engine", eng)
    b = Batch.from_data_list(spmotif.train_mix(64, seed=2)).to(DEV)
    perm = torch.randperm(64, device=DEV)
    for _ in range(2):
        eng.train_step(b, perm, adam=True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0 = random.getstate(), torch.get_rng_state()
    node_gt, edge_gt = spmotif.ground_truth(b)
    ex = m.explain(b, k="gt", edge_gt=edge_gt, node_gt=node_gt)
    assert m.engine() is eng and m.training
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    assert ex.metrics["edge"].shape == (64, 4)
    eng.train_step(b, perm, adam=True)                      # training goes on
    eng.check_status()


def test_eval_explanation_equals_per_batch_explain():
    from cal_amd.data import DataLoader
    from cal_amd.train_causal import eval_acc_causal
    args = _args(layers=2, hidden=64, eval_random=False)
    m, _ = _gpu_model("CausalGCN", 10, 4, args)
    gs = spmotif.train_mix(96, seed=9)
    loader = DataLoader(gs, batch_size=32, shuffle=False)
    res = eval_explanation(m, loader, DEV)
    eval_acc_causal(m, loader, DEV, args)                     # same loader, the classifier's evaluation
    sums = {k: [] for k in res}
    for data in DataLoader(gs, batch_size=32, shuffle=False):
        data = data.to(DEV)
        node_gt, edge_gt = spmotif.ground_truth(data)
        ex = explain(m, data, k="gt", edge_gt=edge_gt, node_gt=node_gt)
        for part, eptr, gt in (("edge", ex.edge_ptr, edge_gt), ("node", ex.ptr, node_gt)):
            score = (ex.edge_score if part == "edge" else ex.node_score).cpu().numpy()
            _, _, om = rank_oracle(score, eptr.cpu().numpy(), k="gt", gt=gt.cpu().numpy())
            np.testing.assert_allclose(ex.metrics[part].cpu().numpy(), om, atol=1e-12, rtol=0, equal_nan=True)
            for row in om:
                kg, hits, P, auc = row
                sums[part + "_precision"].append(hits / kg if kg > 0 else np.nan)
                sums[part + "_recall"].append(hits / P if P > 0 else np.nan)
                sums[part + "_auc"].append(auc)
    for key, vals in sums.items():
        assert abs(res[key] - np.nanmean(vals)) < 1e-12, key
