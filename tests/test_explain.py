"""Causal-subgraph explanations on the CPU: the host twin of cal_explain_rank against a numpy oracle, SPMotif ground
truth, explain() on CPU models against the fp64 oracle's soft masks, and explain() leaving every state untouched."""
import argparse
import random

import numpy as np
import pytest
import torch

from cal_amd import spmotif
from cal_amd.data import Batch
from cal_amd.explain import explain, rank_segments
from oracle import cal_oracle as O
from tests.explain_oracle import rank_oracle
from tests.helpers import random_graph_batch


def _check(score, seg_ptr, max_seg=None, k=None, ratio=None, gt=None):
    score = torch.as_tensor(score, dtype=torch.float32)
    seg = torch.as_tensor(seg_ptr, dtype=torch.long)
    if max_seg is None:
        max_seg = int((seg[1:] - seg[:-1]).max()) if seg.numel() > 1 else 0
    g = None if gt is None else torch.as_tensor(gt, dtype=torch.bool)
    mask, rank, met = rank_segments(score, seg, max_seg, k=k, ratio=ratio, gt=g, metrics=True)
    om, orank, omet = rank_oracle(score.numpy(), seg.numpy(), k=k, ratio=ratio, gt=None if g is None else g.numpy())
    assert np.array_equal(mask.numpy(), om)
    assert np.array_equal(rank.numpy(), orank)
    np.testing.assert_allclose(met.numpy(), omet, atol=1e-12, rtol=0, equal_nan=True)
    return mask, rank, met


def _segments(rng, sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_empty_inputs():
    _check([], [0], k=3)                                  # B = 0
    _check([], [0, 0, 0], k=3)                            # M = 0, two empty segments
    _, _, met = _check([1.0, 2.0], [0, 0, 2, 2], k=1, gt=[1, 0])
    assert met[0, 0].item() == 0 and np.isnan(met[0, 3].item())


def test_random_segments_with_ties_nan_and_singletons():
    rng = np.random.default_rng(0)
    sizes = [1, 0, 5, 17, 1, 64, 33, 0, 200, 3]
    seg = _segments(rng, sizes)
    M = int(seg[-1])
    gt = rng.random(M) < 0.3
    for score in (rng.standard_normal(M),
                  np.round(rng.standard_normal(M) * 2) / 2,     # heavy ties
                  np.full(M, 0.5),
                  np.where(rng.random(M) < 0.2, np.nan, rng.standard_normal(M))):
        s = score.astype(np.float32)
        for kw in (dict(k=0), dict(k=3), dict(k=1000), dict(ratio=0.0), dict(ratio=1.0), dict(ratio=0.25),
                   dict(ratio=0.3), dict(k="gt")):
            _check(s, seg, k=kw.get("k"), ratio=kw.get("ratio"), gt=gt)


def test_ratio_at_an_integer_and_signed_zero():
    # ratio * m exactly integral: ceil keeps it (0.25 * 8 = 2), and -0.0 ranks as +0.0 (index decides)
    s = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 2.0, np.inf], dtype=np.float32)
    mask, rank, _ = _check(s, [0, 8], ratio=0.25)
    assert int(mask.sum()) == 2
    _check(s, [0, 4, 8], ratio=0.5)
    _check(np.array([-np.inf, np.nan, np.inf, 3.0], dtype=np.float32), [0, 4], k=2)


def test_stride_two_reads_the_causal_column():
    rng = np.random.default_rng(1)
    att = torch.from_numpy(rng.random((40, 2)).astype(np.float32))
    seg = torch.tensor([0, 7, 7, 25, 40])
    gt = torch.from_numpy(rng.random(40) < 0.4)
    a = rank_segments(att[:, 1], seg, 18, k=4, gt=gt, metrics=True)
    b = rank_segments(att[:, 1].contiguous(), seg, 18, k=4, gt=gt, metrics=True)
    assert att[:, 1].stride(0) == 2
    for u, v in zip(a, b):
        assert torch.equal(u, v) or torch.allclose(u, v, equal_nan=True)
    _check(att[:, 1].contiguous().numpy(), seg, k="gt", gt=gt.numpy())


def test_segment_longer_than_max_seg_is_not_ranked():
    mask, rank, met = rank_segments(torch.ones(6), torch.tensor([0, 2, 6]), 3, k=1, metrics=True)
    assert rank[:2].tolist() == [0, 1] and rank[2:].tolist() == [-1] * 4
    assert not mask[2:].any() and torch.isnan(met[1]).all()


def test_argument_checks():
    with pytest.raises(ValueError):
        rank_segments(torch.ones(3), torch.tensor([0, 3]), 3)              # neither k nor ratio
    with pytest.raises(ValueError):
        rank_segments(torch.ones(3), torch.tensor([0, 3]), 3, k="gt")      # k = "gt" without gt


def _spmotif_graphs(seed=0, node_num=7):
    rng = np.random.default_rng(seed)
    gs = []
    for ctx in ("tree", "ba"):
        for label, shape in enumerate(spmotif.CLASS_LIST):
            for _ in range(2):
                gs.append(spmotif.make_graph(ctx, shape, node_num, rng, label=label))
    return gs


@pytest.mark.parametrize("pack", [False, True])
def test_spmotif_ground_truth(pack):
    gs = _spmotif_graphs()
    b = Batch.from_data_list(gs, pack=pack)
    node_gt, edge_gt = spmotif.ground_truth(b)
    assert node_gt.dtype == torch.bool and edge_gt.dtype == torch.bool
    ptr, ei = b.ptr.tolist(), b.edge_index
    for g in range(b.num_graphs):
        shape = spmotif.CLASS_LIST[int(b.y[g])]
        n_s, motif = spmotif._MOTIFS[shape]
        lo, hi = ptr[g], ptr[g + 1]
        assert int(node_gt[lo:hi].sum()) == n_s
        assert node_gt[hi - n_s:hi].all()
        sel = (ei[0] >= lo) & (ei[0] < hi)
        assert int(edge_gt[sel].sum()) == 2 * len(motif)
        base = hi - n_s
        pairs = {(a, c) for a, c in motif} | {(c, a) for a, c in motif}
        for u, v in ei[:, edge_gt & sel].t().tolist():
            assert (u - base, v - base) in pairs


def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add")
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.mark.parametrize("name,kw", [("CausalGCN", {}), ("CausalGAT", {}), ("CausalGCN", {"without_edge_attention": True}),
                                     ("CausalGCN", {"without_node_attention": True}), ("CausalGIN", {})])
@pytest.mark.parametrize("loops", [False, True])
def test_cpu_explain_matches_oracle_soft_masks(name, kw, loops):
    from cal_amd import model as M
    torch.manual_seed(3)
    feat = 6
    sd = O.init_state(name, feat, 4, hidden=32, layers=2, heads=4)
    m = getattr(M, name)(feat, 4, _args(**kw))
    m.load_state_dict(sd, strict=name != "CausalGIN")          # (GINConv's eps buffers are not part of the oracle's state)
    b = random_graph_batch(num_graphs=6, feat=feat, seed=5, self_loops=loops)
    if loops:
        assert bool((b.edge_index[0] == b.edge_index[1]).any())
    ex = explain(m, b, ratio=0.3)
    sd64 = {k: v.double() for k, v in sd.items()}
    _, inter = O.causal_forward(name, sd64, b.x.double(), b.edge_index, b.batch, layers=2, heads=4,
                                num_graphs=b.num_graphs, return_intermediates=True, **kw)
    assert torch.allclose(ex.edge_score.double(), inter["edge_att"][:, 1], atol=1e-5)
    assert torch.allclose(ex.node_score.double(), inter["node_att"][:, 1], atol=1e-5)
    if kw.get("without_edge_attention") and name == "CausalGCN":
        assert (ex.edge_score == 0.5).all()
    if kw.get("without_node_attention") and name == "CausalGCN":
        assert (ex.node_score == 0.5).all()
    # masks / ranks are the oracle's ranking of the model's own scores
    om, orank, _ = rank_oracle(ex.node_score.numpy(), ex.ptr.numpy(), ratio=0.3)
    assert np.array_equal(ex.node_mask.numpy(), om) and np.array_equal(ex.node_rank.numpy(), orank)
    om, orank, _ = rank_oracle(ex.edge_score.numpy(), ex.edge_ptr.numpy(), ratio=0.3)
    assert np.array_equal(ex.edge_mask.numpy(), om) and np.array_equal(ex.edge_rank.numpy(), orank)


def test_cpu_explain_leaves_state_untouched_and_reorders_foreign_batches():
    from cal_amd import model as M
    torch.manual_seed(0)
    m = M.CausalGAT(10, 4, _args())
    m.train()
    gs = _spmotif_graphs(seed=2)
    b = Batch.from_data_list(gs)
    node_gt, edge_gt = spmotif.ground_truth(b)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    py0, t0 = random.getstate(), torch.get_rng_state()
    ex = m.explain(b, k="gt", edge_gt=edge_gt, node_gt=node_gt)
    assert m.training
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for key, v in m.state_dict().items():
        assert torch.equal(v, sd0[key]), key
    assert ex.metrics["edge"].shape == (b.num_graphs, 4)
    assert torch.equal(ex.metrics["edge"][:, 0], ex.metrics["edge"][:, 2])           # k = "gt": k_g = P
    nodes, edges = ex.subgraph(3)
    assert nodes.numel() == int(ex.metrics["node"][3, 0]) and edges.size(1) == int(ex.metrics["edge"][3, 0])
    # a foreign batch: the same graphs with their edge columns shuffled across graphs
    perm = torch.randperm(b.edge_index.size(1), generator=torch.Generator().manual_seed(1))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = None, b.feat, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    exf = explain(m, f, k="gt", edge_gt=edge_gt[perm], node_gt=node_gt)
    assert exf.edge_ptr is None
    assert torch.allclose(exf.edge_score, ex.edge_score[perm], atol=1e-6)
    # ranked within each graph in the foreign column order (ties by that order), scattered back to the foreign columns
    order = torch.argsort(b.batch[f.edge_index[0]], stable=True)
    om, orank, omet = rank_oracle(exf.edge_score[order].numpy(), b.edge_ptr.numpy(), k="gt", gt=edge_gt[perm][order].numpy())
    assert np.array_equal(exf.edge_rank[order].numpy(), orank) and np.array_equal(exf.edge_mask[order].numpy(), om)
    np.testing.assert_allclose(exf.metrics["edge"].numpy(), omet, atol=1e-12, rtol=0, equal_nan=True)
    n3, e3 = exf.subgraph(3)
    assert n3.numel() == nodes.numel() and e3.size(1) == edges.size(1)
    assert bool((b.batch[e3[0]] == 3).all())
