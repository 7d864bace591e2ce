"""Subgraph extraction and fidelity on the CPU: the host twin of cal_subgraph_extract against the plain-torch restatement
(every integer output, the gathered rows and the totals bit for bit), structural properties of the result, fidelity() of a
CPU-resident model against the fp64 oracle, and fidelity() leaving every state untouched."""
import argparse
import random

import pytest
import torch

from cal_amd.data import Batch
from cal_amd.explain import Explanation, eval_fidelity, explain, extract_subgraph, fidelity
from oracle import cal_oracle as O
from tests.subgraph_oracle import case_batches, check_extraction, check_fidelity, extract_oracle, fidelity_oracle

CASES = case_batches()


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("complement", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_restatement(name, complement, relabel):
    b, em, nm = CASES[name]
    sub = extract_subgraph(b, edge_mask=em, node_mask=nm, complement=complement, relabel=relabel)
    check_extraction(sub, b, em, nm, complement, relabel)


def test_all_kept_is_the_input_and_all_dropped_is_empty():
    b, em, nm = CASES["all_kept"]
    for relabel in (False, True):
        sub = extract_subgraph(b, edge_mask=em, node_mask=nm, relabel=relabel)
        assert torch.equal(sub.edge_index, b.edge_index) and torch.equal(sub.ptr, b.ptr) and torch.equal(sub.edge_ptr, b.edge_ptr)
        assert torch.equal(sub.batch, b.batch) and torch.equal(sub.x, b.x)
        assert (sub.max_nodes, sub.max_edges) == (b.max_nodes, b.max_edges)
        sub = extract_subgraph(b, edge_mask=em, node_mask=nm, complement=True, relabel=relabel)     # = all dropped
        assert sub.edge_index.shape == (2, 0) and sub.num_graphs == b.num_graphs and sub.max_edges == 0
        assert bool((sub.edge_ptr == 0).all())
        if relabel:
            assert sub.batch.numel() == 0 and sub.x.shape == (0, b.x.size(1)) and bool((sub.ptr == 0).all()) and sub.max_nodes == 0
        else:
            assert torch.equal(sub.ptr, b.ptr)
    sub = extract_subgraph(b)                                     # no mask at all: everything stays
    assert torch.equal(sub.edge_index, b.edge_index) and sub.x is b.x and sub.batch is b.batch


@pytest.mark.parametrize("name", ["edge", "both", "spmotif"])
def test_keep_and_complement_partition_the_edges(name):
    b, em, _ = CASES[name]
    keep = extract_subgraph(b, edge_mask=em)
    drop = extract_subgraph(b, edge_mask=em, complement=True)
    both = torch.cat([keep.edge_map, drop.edge_map])
    assert torch.equal(both.sort().values, torch.arange(b.edge_index.size(1)))
    assert torch.equal(em[keep.edge_map], torch.ones_like(keep.edge_map, dtype=torch.bool))
    assert not em[drop.edge_map].any()


def test_relabel_from_edges_keeps_the_touched_nodes():
    b, em, _ = CASES["edge"]
    sub = extract_subgraph(b, edge_mask=em, relabel=True)
    touched = torch.unique(b.edge_index[:, em])
    assert torch.equal(sub.node_map, touched)
    assert torch.equal(sub.x, b.x[touched])


def test_ungrouped_edge_index_is_reordered_by_graph():
    b, em, nm = CASES["both"]
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x, None, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    order = torch.argsort(b.batch[f.edge_index[0]], stable=True)
    for complement in (False, True):
        for relabel in (False, True):
            sub = extract_subgraph(f, edge_mask=em[perm], node_mask=nm, complement=complement, relabel=relabel)
            r = extract_oracle(f.edge_index[:, order], b.ptr, b.edge_ptr, b.batch.numel(), em[perm][order], nm, complement,
                               relabel, b.x)
            assert torch.equal(sub.edge_index, r["edge_index"]) and torch.equal(sub.edge_ptr, r["edge_ptr"])
            assert torch.equal(sub.ptr, r["ptr"]) and torch.equal(sub.batch, r["batch"]) and torch.equal(sub.x, r["x"])
            assert torch.equal(sub.edge_map, order[r["edge_map"]]) and torch.equal(sub.node_map, r["node_map"])
            assert [sub.batch.numel(), sub.edge_index.size(1), sub.max_nodes, sub.max_edges] == r["totals"]
            src = f.edge_index[:, sub.edge_map]                   # edge_map names the foreign batch's own columns
            assert torch.equal(sub.node_map[sub.edge_index] if relabel else sub.edge_index, src)


def test_edges_leaving_their_graph_are_dropped_and_nothing_is_written_out_of_range():
    ei = torch.tensor([[0, 1, 2, 3, 9, 4], [1, 0, 3, 5, 0, -1]])
    b = Batch()
    b.x, b.edge_index, b.batch = torch.randn(6, 2), ei, torch.tensor([0, 0, 0, 1, 1, 1])
    b.ptr, b.edge_ptr, b.num_graphs, b.max_nodes, b.max_edges = torch.tensor([0, 3, 6]), torch.tensor([0, 3, 6]), 2, 3, 3
    b.y = torch.tensor([0, 1])
    sub = extract_subgraph(b, relabel=True)
    assert sub.edge_map.tolist() == [0, 1, 3] and sub.node_map.tolist() == [0, 1, 3, 5]
    assert sub.edge_index.tolist() == [[0, 1, 2], [1, 0, 3]]
    check_extraction(sub, b, None, None, False, True)


def test_argument_checks():
    b, em, nm = CASES["both"]
    with pytest.raises(ValueError):
        extract_subgraph(b, edge_mask=em[:-1])
    with pytest.raises(ValueError):
        extract_subgraph(b, node_mask=nm[:-1])
    with pytest.raises(ValueError):
        fidelity(None, b, ratio=0.5, k=1)
    with pytest.raises(ValueError):
        fidelity(None, b, ratio=0.5, use="graphs")


def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add")
    d.update(kw)
    return argparse.Namespace(**d)


def _cpu_model(name, feat, seed=3):
    from cal_amd import model as M
    torch.manual_seed(seed)
    sd = O.init_state(name, feat, 4, hidden=32, layers=2, heads=4)
    m = getattr(M, name)(feat, 4, _args())
    m.load_state_dict(sd, strict=name != "CausalGIN")
    return m, sd


def test_to_batch_uses_the_explanations_masks():
    m, _ = _cpu_model("CausalGCN", 5)
    b = CASES["edge"][0]
    ex = explain(m, b, ratio=0.4)
    assert isinstance(ex, Explanation)
    for use, em, nm in (("edges", ex.edge_mask, None), ("nodes", None, ex.node_mask), ("both", ex.edge_mask, ex.node_mask)):
        for complement in (False, True):
            for relabel in (False, True):
                sub = ex.to_batch(b, complement=complement, relabel=relabel, use=use)
                check_extraction(sub, b, em, nm, complement, relabel)
    with pytest.raises(ValueError):
        ex.to_batch(b, use="none")


FID_KEYS = [k + "_" + h for h in ("c", "o", "co") for k in ("acc_full", "acc_keep", "acc_drop", "fid_plus", "fid_minus")]


@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
@pytest.mark.parametrize("use", ["edges", "nodes", "both"])
def test_cpu_fidelity_matches_the_oracle(name, use):
    """The selection is the model's own (the ranking is pinned bit for bit in test_explain); the three forwards and the
    metrics are restated through the fp64 oracle.  fp32 operator-level forward vs fp64: 1e-5 on probabilities (the bound
    test_explain applies to the soft masks); hit counts only on graphs whose oracle top-two gap exceeds ten times that."""
    tol = 1e-5
    m, sd = _cpu_model(name, 5)
    b = CASES["edge"][0]
    ex = explain(m, b, ratio=0.4)
    res = fidelity(m, b, ratio=0.4, use=use)
    ref = fidelity_oracle(name, sd, b, ex.edge_mask if use != "nodes" else None, ex.node_mask if use != "edges" else None,
                          layers=2, heads=4)
    check_fidelity(res, ref, tol)
    assert set(res) == set(FID_KEYS) | {"sparsity", "graphs"}


def test_cpu_fidelity_identities_and_eval_fidelity():
    from cal_amd.data import DataLoader
    from cal_amd import spmotif
    m, _ = _cpu_model("CausalGCN", 10)
    gs = spmotif.train_mix(24, node_num=7, seed=4)
    b = Batch.from_data_list(gs)
    one = fidelity(m, b, ratio=1.0)
    zero = fidelity(m, b, k=0)
    for h in ("c", "o", "co"):
        assert one["fid_minus_" + h] == 0.0 and one["acc_keep_" + h] == one["acc_full_" + h]
        assert zero["fid_plus_" + h] == 0.0 and zero["acc_drop_" + h] == zero["acc_full_" + h]
    assert one["sparsity"] == 0.0 and zero["sparsity"] == 1.0
    # over a loader: the graph-weighted mean of the per-batch reports
    res = eval_fidelity(m, DataLoader(gs, batch_size=8, shuffle=False), "cpu", ratios=(0.25, 0.5))
    assert sorted(res) == [0.25, 0.5]
    for r in res:
        parts = [fidelity(m, Batch.from_data_list(gs[i:i + 8]), ratio=r) for i in (0, 8, 16)]
        for key in FID_KEYS:
            assert abs(res[r][key] - sum(p[key] for p in parts) / 3) < 1e-9, key
        assert res[r]["graphs"] == 24
        ex_kept = sum(int(explain(m, Batch.from_data_list(gs[i:i + 8]), ratio=r).edge_mask.sum()) for i in (0, 8, 16))
        assert abs(res[r]["sparsity"] - (1 - ex_kept / b.edge_index.size(1))) < 1e-12


def test_cpu_fidelity_leaves_state_untouched():
    from cal_amd import model as M
    torch.manual_seed(0)
    m = M.CausalGAT(5, 4, _args())
    m.train()
    b = CASES["edge"][0]
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    py0, t0 = random.getstate(), torch.get_rng_state()
    x0, ei0 = b.x.clone(), b.edge_index.clone()
    res = fidelity(m, b, ratio=0.3, use="both")
    assert m.training and res["graphs"] == b.num_graphs
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for key, v in m.state_dict().items():
        assert torch.equal(v, sd0[key]), key
    assert torch.equal(b.x, x0) and torch.equal(b.edge_index, ei0)
