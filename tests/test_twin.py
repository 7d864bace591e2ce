"""Undirected explanations on the CPU: the host twins of cal_edge_twin and cal_explain_rank_pairs against the oracle
(tests/twin_oracle.py), and the ``undirected`` keyword of explain / eval_explanation / fidelity on CPU models."""
import argparse
import random

import numpy as np
import pytest
import torch

from cal_amd import spmotif
from cal_amd.data import Batch
from cal_amd.explain import edge_twins, eval_explanation, explain, fidelity, rank_segment_pairs
from tests.twin_oracle import make_batch, make_scores, pair_rank_oracle, symmetrise, twin_oracle


class _Cols:
    """The fields the explanation layout reads, from plain arrays."""

    def __init__(self, ei, ptr, eptr=None, max_edges=None, dev="cpu"):
        ptr = torch.as_tensor(ptr, dtype=torch.long)
        self.edge_index = torch.as_tensor(ei, dtype=torch.long).to(dev)
        self.num_graphs = ptr.numel() - 1
        self.batch = torch.repeat_interleave(torch.arange(self.num_graphs), ptr[1:] - ptr[:-1]).to(dev)
        self.ptr = ptr.to(dev)
        self.x = self.feat = None
        self.no_self_loops = False
        if eptr is not None:
            eptr = torch.as_tensor(eptr, dtype=torch.long)
            self.edge_ptr = eptr.to(dev)
            self.max_nodes = int((ptr[1:] - ptr[:-1]).max()) if self.num_graphs else 0
            self.max_edges = max_edges if max_edges is not None else (int((eptr[1:] - eptr[:-1]).max()) if self.num_graphs else 0)


def check_twins(ei, ptr, eptr, max_edges=None, dev="cpu"):
    """edge_twins on ``dev`` == the oracle, exactly; the involution; -> twin (numpy)."""
    twin, n_unp, n_self = edge_twins(_Cols(ei, ptr, eptr, max_edges, dev))
    want, (w_unp, w_self) = twin_oracle(ei, ptr, eptr, max_edges)
    got = twin.cpu().numpy()
    assert twin.dtype == torch.int32 and np.array_equal(got, want)
    assert (int(n_unp), int(n_self)) == (w_unp, w_self)
    has = got >= 0
    assert np.array_equal(got[got[has]], np.nonzero(has)[0])                     # twin[twin[e]] == e
    return got


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int32), b[~nan].view(np.int32))


def check_pairs(score, eptr, twin, reduce, max_seg=None, dev="cpu", gt=None, **kw):
    """rank_segment_pairs on ``dev`` == the oracle: integers exactly, the score bit for bit, AUC 1e-12; -> the four results."""
    seg = torch.as_tensor(eptr, dtype=torch.long)
    bound = max_seg if max_seg is not None else (int((seg[1:] - seg[:-1]).max()) if seg.numel() > 1 else 0)
    s = torch.as_tensor(score, dtype=torch.float32).to(dev)
    g = None if gt is None else torch.as_tensor(gt, dtype=torch.bool).to(dev)
    res = rank_segment_pairs(s, seg.to(dev), bound, torch.as_tensor(twin).to(dev), reduce, gt=g, metrics=True, **kw)
    om, orank, omet, osym = pair_rank_oracle(score, eptr, twin, reduce, gt=gt, max_seg=max_seg, **kw)
    mask, rank, met, sym = (t.cpu() for t in res)
    assert np.array_equal(rank.numpy(), orank)
    assert np.array_equal(mask.numpy(), om)
    assert same_bits(sym.numpy(), osym)
    assert np.array_equal(met[:, :3].numpy(), omet[:, :3], equal_nan=True)
    np.testing.assert_allclose(met[:, 3].numpy(), omet[:, 3], atol=1e-12, rtol=0, equal_nan=True)
    t = np.asarray(twin)
    has = t >= 0
    assert np.array_equal(mask.numpy()[has], mask.numpy()[t[has]]) and np.array_equal(rank.numpy()[has], rank.numpy()[t[has]])
    return mask, rank, met, sym


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257]


def test_host_twin_pairing_rule_by_hand():
    # graph 0 (nodes 0-2): 3 x (0,1) against 1 x (1,0), a duplicated self loop, a directed column; graph 1 (nodes 3-4): one
    # pair and a column whose endpoint lies in graph 0
    ei = [[0, 1, 0, 2, 0, 2, 1, 3, 4, 3], [1, 0, 1, 2, 1, 2, 2, 4, 3, 0]]
    twin = check_twins(ei, [0, 3, 5], [0, 7, 10])
    assert twin.tolist() == [1, 0, -1, 3, -1, 5, -1, 8, 7, -1]


def test_host_twin_matches_oracle():
    check_twins(*make_batch(SIZES, seed=1))
    check_twins(*make_batch([2048, 5, 300], seed=2))
    check_twins(*make_batch([5, 2049, 100], seed=3))
    check_twins(np.zeros((2, 0), dtype=np.int64), [0], [0])                       # B = 0
    check_twins(np.zeros((2, 0), dtype=np.int64), [0, 3, 3], [0, 0, 0])           # E = 0


def test_host_twin_segment_longer_than_max_edges():
    ei, ptr, eptr = make_batch([6, 40, 9], seed=4)
    twin = check_twins(ei, ptr, eptr, max_edges=10)
    assert (twin[6:46] == -1).all() and (twin[:6] >= 0).any()


@pytest.mark.parametrize("reduce", ["mean", "max", "min"])
def test_host_pair_ranking_matches_oracle(reduce):
    ei, ptr, eptr = make_batch(SIZES, seed=5)
    twin, _ = twin_oracle(ei, ptr, eptr)
    s, gt = make_scores(twin, seed=5)
    for kw in (dict(k=0), dict(k=3), dict(k=1000), dict(ratio=0.25), dict(ratio=0.5), dict(ratio=1.0), dict(k="gt")):
        check_pairs(s, eptr, twin, reduce, gt=gt, **kw)
    _, _, met, _ = check_pairs(np.full(len(twin), 0.5, dtype=np.float32), eptr, twin, reduce, k=4, gt=gt)       # all tied
    # m'_g: a ratio of 1 selects every representative
    mask, rank, met, _ = check_pairs(s, eptr, twin, reduce, ratio=1.0, gt=gt)
    idx = np.arange(len(twin))
    reps = (twin < 0) | (twin >= idx)
    for g in range(len(SIZES)):
        assert met[g, 0].item() == reps[eptr[g]:eptr[g + 1]].sum()
    assert mask.all()
    check_pairs(s, eptr, twin, reduce, max_seg=100, k=2, gt=gt)                   # three segments are not ranked


def test_host_symmetrised_score_is_torch_fp32():
    twin = np.array([1, 0, 2, -1, 5, 4], dtype=np.int32)
    s = np.array([0.1, 0.7, 0.3, np.nan, np.nan, 2.5], dtype=np.float32)
    for reduce in ("mean", "max", "min"):
        _, _, _, sym = check_pairs(s, [0, 6], twin, reduce, k=2)
        assert same_bits(sym.numpy(), symmetrise(s, twin, reduce))
        assert torch.isnan(sym[3:]).all()         # NaN on one side of a pair: NaN for both
    a, b = torch.tensor(0.1), torch.tensor(0.7)
    assert check_pairs(s, [0, 6], twin, "mean", k=2)[3][0] == (a + b) * 0.5


def test_argument_checks():
    s, seg, twin = torch.ones(2), torch.tensor([0, 2]), torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(ValueError):
        rank_segment_pairs(s, seg, 2, twin, "median", k=1)
    with pytest.raises(ValueError):
        rank_segment_pairs(s, seg, 2, twin, "mean")                                # neither k nor ratio
    from cal_amd import model as M
    m = M.CausalGCN(10, 4, _args())
    b = Batch.from_data_list(_graphs())
    for fn in (explain, fidelity):
        with pytest.raises(ValueError):
            fn(m, b, ratio=0.5, undirected="sum")
    with pytest.raises(ValueError):
        eval_explanation(m, [b], "cpu", undirected="sum")


def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add")
    d.update(kw)
    return argparse.Namespace(**d)


def _graphs(seed=0):
    rng = np.random.default_rng(seed)
    return [spmotif.make_graph(ctx, shape, 7, rng, label=label)
            for ctx in ("tree", "ba") for label, shape in enumerate(spmotif.CLASS_LIST)]


def _ungrouped(b, perm):
    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x, b.feat, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    return f


def test_edge_twins_of_ungrouped_columns_map_back():
    b = Batch.from_data_list(_graphs())
    twin, n_unp, n_self = edge_twins(b)
    assert int(n_unp) == 0 and int(n_self) == 0 and (twin >= 0).all()             # SPMotif stores both directions
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1))
    tf, u, s = edge_twins(_ungrouped(b, perm))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(E)
    assert torch.equal(tf.long(), inv[twin.long()[perm]])                         # the same pairs, in the foreign numbering
    assert int(u) == 0 and int(s) == 0


@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
def test_cpu_explain_undirected(name):
    from cal_amd import model as M
    torch.manual_seed(3)
    m = getattr(M, name)(10, 4, _args())
    m.train()
    b = Batch.from_data_list(_graphs(seed=2))
    node_gt, edge_gt = spmotif.ground_truth(b)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    py0, t0 = random.getstate(), torch.get_rng_state()
    d = explain(m, b, k="gt", edge_gt=edge_gt, node_gt=node_gt)
    n = explain(m, b, k="gt", edge_gt=edge_gt, node_gt=node_gt, undirected=None)
    ex = explain(m, b, k="gt", edge_gt=edge_gt, node_gt=node_gt, undirected="mean")
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for key, v in m.state_dict().items():
        assert torch.equal(v, sd0[key]), key
    # undirected=None: today's tensors, no twin map
    assert n.edge_twin is None and d.edge_twin is None
    for f in ("edge_score", "node_score", "edge_mask", "node_mask", "edge_rank", "node_rank"):
        assert torch.equal(getattr(n, f), getattr(d, f)), f
    assert torch.equal(n.metrics["edge"], d.metrics["edge"])
    # undirected: the oracle's pair ranking of the model's own directed scores; nodes as before
    twin = ex.edge_twin.numpy()
    assert np.array_equal(twin, twin_oracle(b.edge_index.numpy(), ex.ptr.numpy(), ex.edge_ptr.numpy())[0]) and (twin >= 0).all()
    om, orank, omet, osym = pair_rank_oracle(d.edge_score.numpy(), ex.edge_ptr.numpy(), twin, "mean", k="gt", gt=edge_gt.numpy())
    assert np.array_equal(ex.edge_mask.numpy(), om) and np.array_equal(ex.edge_rank.numpy(), orank)
    assert same_bits(ex.edge_score.numpy(), osym)
    assert np.array_equal(ex.metrics["edge"][:, :3].numpy(), omet[:, :3])
    np.testing.assert_allclose(ex.metrics["edge"][:, 3].numpy(), omet[:, 3], atol=1e-12, rtol=0, equal_nan=True)
    assert torch.equal(ex.edge_mask, ex.edge_mask[ex.edge_twin.long()])
    assert torch.equal(ex.metrics["edge"][:, 2] * 2, d.metrics["edge"][:, 2])     # every motif edge counted once, not twice
    assert torch.equal(ex.node_mask, d.node_mask) and torch.equal(ex.node_rank, d.node_rank)
    # ungrouped columns: the same explanation after mapping back
    perm = torch.randperm(b.edge_index.size(1), generator=torch.Generator().manual_seed(2))
    exf = explain(m, _ungrouped(b, perm), k="gt", edge_gt=edge_gt[perm], node_gt=node_gt, undirected="mean")
    assert exf.edge_ptr is None
    assert torch.allclose(exf.edge_score, ex.edge_score[perm], atol=1e-6)
    assert torch.equal(exf.edge_mask, exf.edge_mask[exf.edge_twin.long()])
    assert torch.equal(exf.metrics["edge"][:, :3], ex.metrics["edge"][:, :3])


def test_cpu_fidelity_and_eval_explanation_undirected():
    from cal_amd import model as M
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, _args())
    b = Batch.from_data_list(_graphs(seed=4))
    ex = explain(m, b, ratio=0.5, undirected="max")
    for comp in (False, True):
        sub = ex.to_batch(b, complement=comp)
        twin, n_unp, _ = edge_twins(sub)
        assert int(n_unp) == 0 and (twin >= 0).all()                              # a symmetric graph on both sides
    rep = fidelity(m, b, ratio=0.5, undirected="max")
    assert rep["graphs"] == b.num_graphs
    assert abs(rep["sparsity"] - (1.0 - float(ex.edge_mask.sum()) / ex.edge_mask.numel())) < 1e-12
    res = eval_explanation(m, [b], "cpu", undirected="mean")
    node_gt, edge_gt = spmotif.ground_truth(b)
    e2 = explain(m, b, k="gt", edge_gt=edge_gt, node_gt=node_gt, undirected="mean")
    met = e2.metrics["edge"]
    assert abs(res["edge_precision"] - float((met[:, 1] / met[:, 0]).mean())) < 1e-12
    assert abs(res["edge_auc"] - float(met[:, 3].mean())) < 1e-12
