"""Occlusion attributions on the CPU: the host twin of cal_occlude_count / cal_occlude_write against the plain-torch restatement
(every integer output, the copied rows and the totals bit for bit), cal_rank_agreement's host twin against the numpy counts, the
exported symbols, the Python layer's argument errors and reordering, and occlusion() / faithfulness() of a CPU-resident model
against the fp64 oracle."""
import argparse
import random
import subprocess

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import edge_twins, explain
from cal_amd.occlude import eval_faithfulness, faithfulness, occlude_batch, occlusion, rank_agreement
from oracle import cal_oracle as O
from tests.occlude_oracle import (agreement_inputs, check_agreement, check_faith, check_occlude, faith_from_scores, occlude_cases,
                                  occlude_oracle, occlusion_oracle)

CASES = occlude_cases()
SYMBOLS = ("cal_occlude_ws", "cal_occlude_count", "cal_occlude_write", "cal_rank_agreement_ws", "cal_rank_agreement")


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_restatement(name):
    b, rg, re, use, twin = CASES[name]
    check_occlude(occlude_batch(b, rg, re, use=use, twin=twin), b, rg, re, use, twin)


def test_abi_symbols_are_exported_by_both_libraries():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_occlude_count"][1]) == 17 and len(protos["cal_occlude_write"][1]) == 25
    assert len(protos["cal_rank_agreement"][1]) == 13


def test_the_pieces_of_a_result():
    b, _, _, _, twin = CASES["mix_edges_twin"]
    B = b.num_graphs
    # control replicas of every graph in order: the batch itself
    res = occlude_batch(b, torch.arange(B), torch.full((B,), -1))
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "x", "y"):
        assert torch.equal(getattr(res, key), getattr(b, key)), key
    assert (res.max_nodes, res.max_edges, res.empty_graphs) == (b.max_nodes, b.max_edges, 0)
    # the self loop is its own twin: one column goes; a pair: two; a column without a twin: one
    for e, gone in ((0, [0]), (1, [1, 2]), (4, [3, 4]), (5, [5])):
        res = occlude_batch(b, torch.tensor([1]), torch.tensor([e]), twin=twin)
        assert sorted(set(range(8)) - set(res.edge_src.tolist())) == gone
    # a node: its row and every incident column
    res = occlude_batch(b, torch.tensor([1]), torch.tensor([2]), use="nodes")
    assert res.node_src.tolist() == [1, 3, 4] and res.edge_src.tolist() == [0, 5] and res.edge_index.tolist() == [[0, 1], [0, 2]]
    assert res.y.tolist() == [1]
    res = occlude_batch(b, torch.tensor([0, 5]), torch.tensor([0, 0]), use="nodes")
    assert res.empty_graphs == 2 and res.y is None and res.ptr.tolist() == [0, 0, 0]


def test_ungrouped_and_foreign_inputs():
    b, rg, re, _, twin = CASES["repeated_edges"]
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x, None, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    order = torch.argsort(b.batch[f.edge_index[0]], stable=True)
    g = Batch()
    g.__dict__.update(b.__dict__)
    g.edge_index = f.edge_index[:, order]                  # the same columns, grouped: what the operator sees
    tg = edge_twins(g)[0]
    ftwin = edge_twins(f)[0]                               # in the caller's column numbering
    fe = order[re]                                         # the caller's ids of the columns at the grouped positions re
    res = occlude_batch(f, rg, fe, twin=ftwin)
    r = occlude_oracle(g, rg, re, "edges", tg)
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "x"):
        assert torch.equal(getattr(res, key), r[key]), key
    assert torch.equal(res.edge_src, order[r["edge_src"]])               # edge_src names the caller's own columns


def test_argument_errors():
    b, rg, re, _, twin = CASES["mix_edges_twin"]
    with pytest.raises(ValueError):
        occlude_batch(b, rg, re[:-1])
    with pytest.raises(TypeError):
        occlude_batch(b, rg.float(), re)
    with pytest.raises(TypeError):
        occlude_batch(b, None, re)
    with pytest.raises(ValueError):
        occlude_batch(b, rg, re, use="both")
    with pytest.raises(ValueError):
        occlude_batch(b, rg, re, twin=twin[:-1])
    with pytest.raises(TypeError):
        c = Batch()
        c.__dict__.update(b.__dict__)
        c.x = b.x.double()
        occlude_batch(c, rg, re)
    for kw in (dict(use="both"), dict(undirected="sum"), dict(head="x"), dict(chunk=0), dict(use="nodes", undirected="mean")):
        with pytest.raises(ValueError):
            occlusion(None, b, **kw)
    for kw in (dict(), dict(ratio=0.5, k=1), dict(k="gt"), dict(ratio=0.5, head="oc")):
        with pytest.raises(ValueError):
            faithfulness(None, b, **kw)
    a = torch.zeros(4)
    with pytest.raises(ValueError):
        rank_agreement(a, a, torch.tensor([0, 4]), 4)
    with pytest.raises(TypeError):
        rank_agreement(a, a.double(), torch.tensor([0, 4]), 4, k=1)
    with pytest.raises(_lib.CalError):
        rank_agreement(a, a, torch.tensor([0, 4]), 1 << 20, k=1)


# ---- rank agreement -----------------------------------------------------------------------------------------------------------
def test_host_rank_agreement_equals_the_numpy_counts():
    a, b, seg = check_agreement("cpu")
    # no segment at all
    counts, met = rank_agreement(a[:0], b[:0], torch.tensor([0]), 0, k=1)
    assert counts.shape == (0, 10) and met.shape == (0, 3)
    # the counts of a small case by hand: a = 1 2 2 3, b = 1 3 2 2
    c, m = rank_agreement(torch.tensor([1., 2., 2., 3.]), torch.tensor([1., 3., 2., 2.]), torch.tensor([0, 4]), 4, k=2)
    assert c.tolist() == [[4, 3, 1, 1, 1, 4 + 25 + 25 + 64, 4 + 64 + 25 + 25, 4 + 40 + 25 + 40, 2, 1]]
    assert abs(m[0, 1].item() - 2 / 5) < 1e-15 and abs(m[0, 2].item() - 1 / 3) < 1e-15


def test_identical_and_reversed_rankings():
    a, _, seg, sel = agreement_inputs()
    counts, met = rank_agreement(a, a.clone(), seg, 5000, sel=sel, ratio=0.3)
    ok = ~met[:, 0].isnan()
    assert bool(ok[3:9].all()) and bool((met[ok] == 1.0).all())          # rho = tau = J = 1, exactly
    assert bool(met[9:11, :2].isnan().all()) and met[9:11, 2].tolist() == [1.0, 1.0]       # a constant ranking: only J
    d = torch.randperm(3000, generator=torch.Generator().manual_seed(1)).float()          # distinct values
    seg = torch.tensor([0, 2, 70, 3000])
    counts, met = rank_agreement(d, -d, seg, 3000, ratio=0.5)
    assert bool((met[:, :2] == -1.0).all()) and counts[:, 1].tolist() == [0, 0, 0]
    assert counts[:, 2].tolist() == [1, 68 * 67 // 2, 2930 * 2929 // 2]


# ---- the scores of a CPU-resident model ---------------------------------------------------------------------------------------
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


def check_scores(got, want, tol):
    got, want = got.cpu().double(), want.cpu()
    assert torch.equal(got.isnan(), want.isnan())
    err = (got - want)[~want.isnan()].abs().max().item() if bool((~want.isnan()).any()) else 0.0
    print("max |score - oracle| = %.3g (tol %.3g)" % (err, tol))
    assert err < tol, err


@pytest.mark.parametrize("use,undirected", [("edges", None), ("edges", "mean"), ("nodes", None)])
def test_cpu_occlusion_and_faithfulness_match_the_oracle(use, undirected):
    """fp32 operator-level forward against fp64: 1e-5 on probabilities (the bound test_subgraph applies to fidelity), a score is
    the difference of two.  The rank figures are recomputed by the numpy counts from the model's own score tensors."""
    tol = 2e-5
    m, sd = _cpu_model("CausalGCN", 10)
    gs = spmotif.train_mix(4, node_num=7, seed=4)
    b = Batch.from_data_list(gs)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    py0, t0 = random.getstate(), torch.get_rng_state()
    occ = m.occlusion(b, use=use, undirected=undirected, chunk=50)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    twin = edge_twins(b)[0] if undirected else None
    assert (occ.twin is None) == (twin is None) and (twin is None or torch.equal(occ.twin, twin))
    M = b.edge_index.size(1) if use == "edges" else b.batch.numel()
    n = int((~((twin >= 0) & (twin < torch.arange(M)))).sum()) if undirected else M
    assert occ.replicas == n and occ.forwards == 1 + -(-n // 50) and occ.score.shape == (M,) and occ.score.dtype == torch.float32
    check_scores(occ.score, occlusion_oracle("CausalGCN", sd, b, occ.yhat, use, twin, layers=2, heads=4), tol)
    # a subset of the elements, another head
    el = torch.rand(M, generator=torch.Generator().manual_seed(2)) < 0.3
    sub = occlusion(m, b, use=use, undirected=undirected, head="co", elements=el)
    check_scores(sub.score, occlusion_oracle("CausalGCN", sd, b, sub.yhat, use, twin, head="co", elements=el, layers=2, heads=4), tol)
    assert int((~sub.score.isnan()).sum()) < M
    # faithfulness: the figures from the model's own score tensors
    res = m.faithfulness(b, use=use, undirected=undirected, ratio=0.3)
    ex = explain(m, b, ratio=0.3, undirected=undirected)
    causal, top = (ex.edge_score, ex.edge_mask) if use == "edges" else (ex.node_score, ex.node_mask)
    seg, mx = (b.edge_ptr, b.max_edges) if use == "edges" else (b.ptr, b.max_nodes)
    sel = None if twin is None else ~((twin >= 0) & (twin < torch.arange(M)))
    check_faith(res, [faith_from_scores(causal, occ.score, seg, mx, sel, top, ratio=0.3)])
    assert res["replicas"] == n and res["forwards"] == 1 + -(-n // 512)
    for key, v in m.state_dict().items():
        assert torch.equal(v, sd0[key]), key


def test_cpu_eval_faithfulness_sums_the_mini_batches():
    m, _ = _cpu_model("CausalGCN", 10)
    gs = spmotif.train_mix(6, node_num=7, seed=5)
    res = eval_faithfulness(m, DataLoader(gs, batch_size=2, shuffle=False), "cpu", undirected="max", k=3)
    parts = [faithfulness(m, Batch.from_data_list(gs[i:i + 2]), undirected="max", k=3) for i in (0, 2, 4)]
    assert res["graphs"] == 6 and res["replicas"] == sum(p["replicas"] for p in parts)
    for key in ("rho", "tau", "jaccard"):
        ws = [(p[key], p["graphs"] - p[key + "_undefined"]) for p in parts]
        tot = sum(c for _, c in ws)
        assert res[key + "_undefined"] == 6 - tot
        assert abs(res[key] - sum(v * c for v, c in ws if c) / tot) < 1e-12


def test_occlusion_of_ungrouped_columns_answers_in_the_callers_order():
    m, _ = _cpu_model("CausalGCN", 10)
    b = Batch.from_data_list(spmotif.train_mix(3, node_num=7, seed=6))
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(8))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x, b.feat, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    el = torch.rand(E, generator=torch.Generator().manual_seed(9)) < 0.5
    for undirected in (None, "mean"):
        want = occlusion(m, b, undirected=undirected, elements=el)
        got = occlusion(m, f, undirected=undirected, elements=el[perm])          # column j of f is column perm[j] of b
        assert torch.equal(got.score.isnan(), want.score[perm].isnan()) and got.replicas == want.replicas
        ok = ~got.score.isnan()
        assert bool(ok.any()) and (got.score[ok] - want.score[perm][ok]).abs().max().item() < 1e-6      # (another column order)
        if undirected:
            paired = got.twin >= 0
            assert torch.equal(f.edge_index[:, got.twin[paired].long()], f.edge_index[:, paired].flip(0))
            assert torch.equal(paired, want.twin[perm] >= 0)


def test_one_node_graphs_score_nan_in_node_mode():
    from tests.occlude_oracle import hand_batch
    m, _ = _cpu_model("CausalGCN", 3)
    b = hand_batch([(1, []), (3, [(0, 1), (1, 0), (1, 2), (2, 1)])])
    occ = occlusion(m, b, use="nodes")
    assert occ.score.isnan().tolist() == [True, False, False, False] and occ.replicas == 3 and occ.forwards == 2
