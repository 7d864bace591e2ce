"""Coalition replicas, Shapley values and perturbation curves on the CPU: the host twin of cal_coalition_count /
cal_coalition_write against the plain-torch restatement (every integer output, the copied rows and the totals bit for bit), the
exported symbols, the Python layer's argument errors and reordering, and shapley() / perturbation_curve() /
shapley_agreement() of a CPU-resident model against the fp64 oracle, with the exact properties of the estimate."""
import argparse
import random
import subprocess

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.coalition import (coalition_batch, eval_perturbation_curve, perturbation_curve, shapley, shapley_agreement)
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import edge_twins, explain, fidelity
from cal_amd.occlude import occlude_batch, rank_agreement
from oracle import cal_oracle as O
from tests.coalition_oracle import (check_coalition, coalition_cases, coalition_oracle, curve_oracle, random_orders, rank_keys,
                                    representatives, shapley_oracle)
from tests.occlude_oracle import hand_batch

CASES = coalition_cases()
SYMBOLS = ("cal_coalition_ws", "cal_coalition_count", "cal_coalition_write")


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_restatement(name):
    b, rg, rrow, rth, key, use, invert = CASES[name]
    r = check_coalition(coalition_batch(b, rg, rth, key, rep_row=rrow, use=use, invert=invert), b, rg, rrow, rth, key, use, invert)
    if name == "rings_nodes":
        assert r["totals"][4] > 10                                        # graphs that lose every node are counted


def test_abi_symbols_are_exported_by_both_libraries():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_coalition_count"][1]) == 21 and len(protos["cal_coalition_write"][1]) == 29
    assert len(protos["cal_coalition_ws"][1]) == 4


def test_the_pieces_of_a_result():
    b = CASES["rings_edges"][0]
    B = b.num_graphs
    key = CASES["rings_edges"][4]
    # control replicas of every graph in order: the batch itself
    res = coalition_batch(b, torch.arange(B), torch.zeros(B, dtype=torch.long), key, rep_row=torch.full((B,), -1))
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "x", "y"):
        assert torch.equal(getattr(res, k), getattr(b, k)), k
    assert (res.max_nodes, res.max_edges, res.empty_graphs) == (b.max_nodes, b.max_edges, 0)
    # the 4-ring (columns 6 .. 13) under a permutation: threshold t keeps exactly the t columns with key < t; invert the rest
    row = key[0, 6:14].tolist()
    for t in (0, 3, 8):
        res = coalition_batch(b, torch.tensor([1]), torch.tensor([t]), key[0])
        assert sorted(res.edge_src.tolist()) == sorted(6 + i for i, k in enumerate(row) if k < t) and res.node_src.tolist() == [3, 4, 5, 6]
        inv = coalition_batch(b, torch.tensor([1]), torch.tensor([t]), key[0], invert=True)
        assert sorted(res.edge_src.tolist() + inv.edge_src.tolist()) == list(range(6, 14))
    # nodes: the kept nodes are renumbered densely, a column stays iff both endpoints stay
    nk = torch.full((int(b.batch.numel()),), 9, dtype=torch.int32)
    nk[3:7] = torch.tensor([0, 5, 1, 5])                                  # of the 4-ring 3-4-5-6 keep nodes 3 and 5: no edge between
    res = coalition_batch(b, torch.tensor([1, 1]), torch.tensor([2, 6]), nk, use="nodes")
    assert res.node_src.tolist() == [3, 5, 3, 4, 5, 6] and res.ptr.tolist() == [0, 2, 6] and res.edge_ptr.tolist() == [0, 0, 8]
    assert torch.equal(res.edge_index, b.edge_index[:, 6:14] - 3 + 2) and res.y.tolist() == [1, 1]
    res = coalition_batch(b, torch.tensor([1, 7]), torch.tensor([0, 0]), nk, use="nodes")
    assert res.empty_graphs == 2 and res.y is None and res.ptr.tolist() == [0, 0, 0]
    # key = (e != elem), threshold 1: the occlusion replica of elem
    for use, elem in (("edges", 9), ("nodes", 5)):
        M = b.edge_index.size(1) if use == "edges" else b.batch.numel()
        res = coalition_batch(b, torch.tensor([1]), torch.tensor([1]), (torch.arange(M) != elem).int(), use=use, invert=True)
        want = occlude_batch(b, torch.tensor([1]), torch.tensor([elem]), use=use)
        for k in ("edge_index", "ptr", "edge_ptr", "batch", "x", "node_src", "edge_src"):
            assert torch.equal(getattr(res, k), getattr(want, k)), k


def test_ungrouped_and_foreign_inputs():
    b, rg, rrow, rth, key, _, _ = CASES["spmotif_edges"]
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x, b.feat, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    order = torch.argsort(b.batch[f.edge_index[0]], stable=True)
    g = Batch()
    g.__dict__.update(b.__dict__)
    g.edge_index = f.edge_index[:, order]                  # the same columns, grouped: what the operator sees
    fkey = torch.randint(0, 9, (2, E), generator=torch.Generator().manual_seed(6), dtype=torch.int32)    # in the caller's numbering
    res = coalition_batch(f, rg, rth, fkey, rep_row=rrow)
    r = coalition_oracle(g, rg, rrow, rth, fkey[:, order], "edges", False)
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src"):
        assert torch.equal(getattr(res, k), r[k]), k
    assert torch.equal(res.feat if res.x is None else res.x, r["x"])
    assert torch.equal(res.edge_src, order[r["edge_src"]])               # edge_src names the caller's own columns
    assert bool((fkey[rrow[res.batch[res.edge_index[0]]], res.edge_src] < rth[res.batch[res.edge_index[0]]]).all())
    # nodes of a foreign input: max_nodes is derived
    nkey = torch.randint(0, 5, (f.batch.numel(),), generator=torch.Generator().manual_seed(7), dtype=torch.int32)
    rg2 = torch.arange(b.num_graphs)
    res = coalition_batch(f, rg2, torch.full_like(rg2, 3), nkey, use="nodes")
    r = coalition_oracle(g, rg2, torch.zeros_like(rg2), torch.full_like(rg2, 3), nkey.view(1, -1), "nodes", False)
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src"):
        assert torch.equal(getattr(res, k), r[k]), k


def test_argument_errors():
    b, rg, rrow, rth, key, _, _ = CASES["rings_edges"]
    with pytest.raises(ValueError):
        coalition_batch(b, rg, rth[:-1], key, rep_row=rrow)
    with pytest.raises(ValueError):
        coalition_batch(b, rg, rth, key, rep_row=rrow[:-1])
    with pytest.raises(ValueError):
        coalition_batch(b, rg, rth, key)                                  # three rows and no rep_row
    with pytest.raises(TypeError):
        coalition_batch(b, rg.float(), rth, key, rep_row=rrow)
    with pytest.raises(TypeError):
        coalition_batch(b, None, rth, key, rep_row=rrow)
    with pytest.raises(ValueError):
        coalition_batch(b, rg, rth, key, rep_row=rrow, use="both")
    with pytest.raises(ValueError):
        coalition_batch(b, rg, rth, key[:, :-1], rep_row=rrow)
    with pytest.raises(ValueError):
        coalition_batch(b, rg, rth, key, rep_row=rrow, use="nodes")       # one entry per edge column, not per node
    with pytest.raises(TypeError):
        coalition_batch(b, rg, rth, key.float(), rep_row=rrow)
    with pytest.raises(TypeError):
        c = Batch()
        c.__dict__.update(b.__dict__)
        c.x = b.x.double()
        coalition_batch(c, rg, rth, key, rep_row=rrow)
    E = b.edge_index.size(1)
    for fn in (shapley, perturbation_curve, lambda m, d, **kw: shapley_agreement(m, d, ratio=0.5, **kw)):
        for kw in (dict(use="both"), dict(undirected="sum"), dict(head="x"), dict(chunk=0), dict(use="nodes", undirected="mean")):
            with pytest.raises(ValueError):
                fn(None, b, **kw)
    with pytest.raises(ValueError):
        shapley(None, b, perms=0)
    with pytest.raises(TypeError):
        shapley(None, b, perms=2.5)
    with pytest.raises(ValueError):
        perturbation_curve(None, b, ratios=())
    with pytest.raises(ValueError):
        perturbation_curve(None, b, ratios=(0.1, -0.5))
    for kw in (dict(), dict(ratio=0.5, k=1), dict(k="gt")):
        with pytest.raises(ValueError):
            shapley_agreement(None, b, **kw)
    m, _ = _cpu_model("CausalGCN", 3)
    with pytest.raises(ValueError):
        shapley(m, b, perms=torch.zeros(2, E - 1, dtype=torch.int32))
    with pytest.raises(TypeError):
        shapley(m, b, perms=torch.zeros(2, E, dtype=torch.long))
    with pytest.raises(ValueError):
        shapley(m, b, elements=torch.ones(E - 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        perturbation_curve(m, b, order=torch.zeros(E + 1))


# ---- the drivers of a CPU-resident model --------------------------------------------------------------------------------------
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


def _err(got, want):
    got, want = got.cpu().double(), want.cpu().double()
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    return (got - want)[ok].abs().max().item() if bool(ok.any()) else 0.0


TOL = 2e-5          # fp32 operator-level forward against fp64: 1e-5 on a probability (the bound test_subgraph applies to fidelity);
#                     a marginal is the difference of two and a mean of marginals keeps that bound


def _players_sum(score, off, rep):
    """Per graph the sum of ``score`` over the players' representatives (NaN: no player)."""
    s = torch.where(rep & ~score.isnan(), score, torch.zeros_like(score))
    return torch.stack([s[lo:hi].sum() for lo, hi in zip(off[:-1].tolist(), off[1:].tolist())])


@pytest.mark.parametrize("use,undirected,subset", [("edges", None, False), ("edges", "mean", False), ("nodes", None, False),
                                                   ("edges", "max", True), ("nodes", None, True)])
def test_cpu_shapley_matches_the_oracle(use, undirected, subset):
    m, sd = _cpu_model("CausalGCN", 10)
    b = Batch.from_data_list(spmotif.train_mix(3, node_num=6, seed=4))
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    twin = edge_twins(b)[0] if undirected else None
    off = b.edge_ptr if use == "edges" else b.ptr
    M = int(off[-1])
    el = (torch.rand(M, generator=torch.Generator().manual_seed(2)) < 0.4) if subset else None
    keys = random_orders(b, 3, use, twin, el, seed=7)
    m.train()
    py0, t0 = random.getstate(), torch.get_rng_state()
    sh = m.shapley(b, use=use, undirected=undirected, perms=keys, elements=el, chunk=37)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    want, p_full, p_empty, reps = shapley_oracle("CausalGCN", sd, b, sh.yhat, keys, use, layers=2, heads=4)
    assert sh.replicas == reps and sh.forwards == 1 + -(-reps // 37) and sh.forwards >= 3
    assert sh.score.dtype == torch.float64 and sh.stderr.dtype == torch.float64 and sh.score.shape == (M,)
    assert torch.equal(sh.keys, keys) and (sh.twin is None) == (twin is None) and (twin is None or torch.equal(sh.twin, twin))
    err = _err(sh.score, want)
    print("max |score - oracle| = %.3g over %d replicas (tol %.3g)" % (err, reps, TOL))
    assert err < TOL and _err(sh.p_full, p_full) < TOL and _err(sh.p_empty, p_empty) < TOL
    assert int((~sh.score.isnan()).sum()) == int((keys[0] >= 0).sum()) and bool((sh.stderr[~sh.score.isnan()] >= 0).all())
    # the scores of a graph's players sum to p_full - p_empty: the telescoping sum of fp32 values taken in fp64
    rep = representatives(twin, M)
    n = torch.stack([(rep & (keys[0] >= 0))[lo:hi].sum() for lo, hi in zip(off[:-1].tolist(), off[1:].tolist())])
    gap = (_players_sum(sh.score, off, rep) - (sh.p_full.double() - sh.p_empty)).abs()
    assert bool((gap <= (n + 1) * 2.0 ** -50).all()), gap
    if twin is not None:                                                  # both columns of an undirected edge receive the score
        pair = twin >= 0
        assert torch.equal(sh.score[pair].nan_to_num(7.0), sh.score[twin[pair].long()].nan_to_num(7.0))
    if use == "nodes" and not subset:                                     # the empty replica is not run: 1 / C
        assert bool((sh.p_empty == 0.25).all())
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_cpu_shapley_draws_orders_and_leaves_the_rng_alone():
    m, _ = _cpu_model("CausalGCN", 10)
    b = Batch.from_data_list(spmotif.train_mix(3, node_num=6, seed=5))
    twin = edge_twins(b)[0]
    E = b.edge_index.size(1)
    py0, t0 = random.getstate(), torch.get_rng_state()
    one = shapley(m, b, undirected="mean", perms=2, generator=torch.Generator().manual_seed(11))
    two = shapley(m, b, undirected="mean", perms=2, generator=torch.Generator().manual_seed(11))
    free = shapley(m, b, undirected="mean", perms=2)
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    assert torch.equal(one.score, two.score) and torch.equal(one.keys, two.keys) and torch.equal(one.stderr, two.stderr)
    assert not torch.equal(one.keys, free.keys)
    # the keys are per graph a permutation of the undirected edges, both columns of a pair the same
    rep = representatives(twin, E)
    for keys in (one.keys, free.keys):
        assert keys.shape == (2, E) and keys.dtype == torch.int32
        for s in range(2):
            assert torch.equal(keys[s][twin >= 0], keys[s][twin[twin >= 0].long()])
            for lo, hi in zip(b.edge_ptr[:-1].tolist(), b.edge_ptr[1:].tolist()):
                assert sorted(keys[s, lo:hi][rep[lo:hi]].tolist()) == list(range(int(rep[lo:hi].sum())))
    # the drawn orders handed back in give the same estimate; identical orders: no spread; one order: none defined
    again = shapley(m, b, undirected="mean", perms=one.keys)
    assert torch.equal(again.score, one.score)
    same = shapley(m, b, undirected="mean", perms=one.keys[:1].repeat(3, 1))
    assert bool((same.stderr == 0).all()) and torch.equal(same.score, shapley(m, b, undirected="mean", perms=one.keys[:1]).score)
    assert bool(shapley(m, b, undirected="mean", perms=one.keys[:1]).stderr.isnan().all())


def test_cpu_one_player_graphs_and_redundant_edges():
    m, _ = _cpu_model("CausalGCN", 3)
    # a graph with one undirected edge (one player) next to a triangle
    b = hand_batch([(2, [(0, 1), (1, 0)]), (3, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 0), (0, 2)])])
    sh = shapley(m, b, undirected="mean", perms=3)
    assert sh.score[0] == sh.p_full[0].double() - sh.p_empty[0] and sh.score[1] == sh.score[0]
    assert sh.replicas == 3 * (1 + 3) and sh.forwards == 2
    # use="nodes" with a one-node graph: its only replica would be empty, so nothing runs for it
    b = hand_batch([(1, []), (3, [(0, 1), (1, 0), (1, 2), (2, 1)])])
    sh = shapley(m, b, use="nodes", perms=2)
    assert sh.replicas == 2 * 2 and sh.score[0] == sh.p_full[0].double() - 0.25 and sh.p_empty.tolist() == [0.25, 0.25]
    assert not bool(sh.score.isnan().any())


@pytest.mark.parametrize("use,undirected", [("edges", None), ("edges", "mean"), ("nodes", None)])
def test_cpu_perturbation_curve_matches_the_oracle_and_fidelity(use, undirected):
    m, sd = _cpu_model("CausalGCN", 10)
    gs = spmotif.train_mix(4, node_num=6, seed=6)
    b = Batch.from_data_list(gs)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    twin = edge_twins(b)[0] if undirected else None
    ratios = (0.0, 0.25, 0.3, 0.7, 1.0)
    m.train()
    res = m.perturbation_curve(b, use=use, undirected=undirected, ratios=ratios, chunk=7)
    assert m.training
    ex = explain(m, b, ratio=0.5, undirected=undirected)
    score = ex.edge_score if use == "edges" else ex.node_score
    key = rank_keys(score, b, use, twin)
    ins, dele, p_full = curve_oracle("CausalGCN", sd, b, res["yhat"], key, ratios, use, layers=2, heads=4)
    B, T = 4, len(ratios)
    assert res["insertion"].shape == (B, T) and res["deletion"].shape == (B, T) and res["ratios"] == list(ratios)
    err = max(_err(res["insertion"], ins), _err(res["deletion"], dele), _err(res["p_full"], p_full))
    print("max |p - oracle| = %.3g (tol %.3g)" % (err, TOL))
    assert err < TOL
    skipped = 2 * B if use == "nodes" else 0                              # insertion at ratio 0, deletion at ratio 1: no node
    assert res["replicas"] == 2 * T * B - skipped and res["forwards"] == 2 + 2 * -(-(T * B - skipped // 2) // 7)
    # the end points: everything kept is the whole graph, bit for bit on the CPU
    assert torch.equal(res["insertion"][:, -1], res["p_full"]) and torch.equal(res["deletion"][:, 0], res["p_full"])
    if use == "nodes":
        assert bool((res["insertion"][:, 0] == 0.25).all()) and bool((res["deletion"][:, -1] == 0.25).all())
    # means and areas
    assert torch.equal(res["insertion_mean"], res["insertion"].double().mean(0))
    x = torch.tensor(ratios, dtype=torch.float64)
    for name in ("insertion", "deletion"):
        y = res[name].double()
        want = sum((y[:, t + 1] + y[:, t]) / 2 * (x[t + 1] - x[t]) for t in range(T - 1))
        assert (res["auc_" + name] - want).abs().max().item() < 1e-15 and res["auc_" + name].dtype == torch.float64
        assert abs(res["auc_%s_mean" % name].item() - want.mean().item()) < 1e-15
    # an explicit order: the same ranking handed in gives the same curves
    again = perturbation_curve(m, b, use=use, undirected=undirected, ratios=ratios, order=score)
    assert torch.equal(again["insertion"], res["insertion"]) and torch.equal(again["deletion"], res["deletion"])
    assert again["replicas"] == res["replicas"] and again["forwards"] == 1 + 2 * -(-(T * B - skipped // 2) // 512)
    if use == "edges":                                                    # the same graphs as fidelity's two extractions
        for t, r in enumerate(ratios):
            fid = fidelity(m, b, ratio=r, use="edges", undirected=undirected)
            pf = res["p_full"].double().mean().item()
            assert abs(pf - res["insertion_mean"][t].item() - fid["fid_minus_o"]) < TOL
            assert abs(pf - res["deletion_mean"][t].item() - fid["fid_plus_o"]) < TOL
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_cpu_eval_perturbation_curve_sums_the_mini_batches():
    m, _ = _cpu_model("CausalGCN", 10)
    gs = spmotif.train_mix(5, node_num=6, seed=5)
    ratios = (0.0, 0.5, 1.0)
    res = eval_perturbation_curve(m, DataLoader(gs, batch_size=2, shuffle=False), "cpu", undirected="max", ratios=ratios)
    parts = [perturbation_curve(m, Batch.from_data_list(gs[i:i + 2]), undirected="max", ratios=ratios) for i in (0, 2, 4)]
    w = [2, 2, 1]
    assert res["graphs"] == 5 and res["replicas"] == sum(p["replicas"] for p in parts) and res["forwards"] == sum(p["forwards"] for p in parts)
    for name in ("insertion_mean", "deletion_mean"):
        want = sum(p[name] * c for p, c in zip(parts, w)) / 5
        assert (torch.tensor(res[name], dtype=torch.float64) - want).abs().max().item() < 1e-12
    for name in ("auc_insertion_mean", "auc_deletion_mean"):
        assert abs(res[name] - sum(p[name].item() * c for p, c in zip(parts, w)) / 5) < 1e-12
    assert abs(res["p_full_mean"] - sum(p["p_full"].double().sum().item() for p in parts) / 5) < 1e-12


def test_cpu_shapley_agreement_from_the_models_own_scores():
    m, _ = _cpu_model("CausalGCN", 10)
    b = Batch.from_data_list(spmotif.train_mix(4, node_num=6, seed=8))
    for use, undirected in (("edges", "mean"), ("nodes", None)):
        twin = edge_twins(b)[0] if undirected else None
        keys = random_orders(b, 2, use, twin, seed=3)
        res = shapley_agreement(m, b, use=use, undirected=undirected, perms=keys, ratio=0.3)
        sh = shapley(m, b, use=use, undirected=undirected, perms=keys)
        ex = explain(m, b, ratio=0.3, undirected=undirected)
        causal = ex.edge_score if use == "edges" else ex.node_score
        seg, mx = (b.edge_ptr, b.max_edges) if use == "edges" else (b.ptr, b.max_nodes)
        sel = None if twin is None else representatives(twin, twin.numel())
        counts, met = rank_agreement(causal, sh.score.float(), seg, mx, sel=sel, ratio=0.3)
        for j, name in enumerate(("rho", "tau", "jaccard")):
            ok = ~met[:, j].isnan()
            assert res[name + "_undefined"] == int((~ok).sum())
            assert abs(res[name] - met[ok, j].mean().item()) < 1e-12 if bool(ok.any()) else res[name] != res[name]
        assert res["graphs"] == 4 and res["elements"] == int(counts[:, 0].sum()) and res["replicas"] == sh.replicas
        assert res["forwards"] == sh.forwards + 1


def test_shapley_of_ungrouped_columns_answers_in_the_callers_order():
    m, _ = _cpu_model("CausalGCN", 10)
    b = Batch.from_data_list(spmotif.train_mix(3, node_num=6, seed=6))
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(8))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x, b.feat, b.edge_index[:, perm], b.batch, b.num_graphs, b.y
    twin = edge_twins(b)[0]
    keys = random_orders(b, 2, "edges", twin, seed=1)
    want = shapley(m, b, undirected="mean", perms=keys)
    got = shapley(m, f, undirected="mean", perms=keys[:, perm])           # column j of f is column perm[j] of b
    assert torch.equal(got.keys, keys[:, perm]) and (got.score - want.score[perm]).abs().max().item() < 1e-6
    paired = got.twin >= 0
    assert torch.equal(f.edge_index[:, got.twin[paired].long()], f.edge_index[:, paired].flip(0))
    cw = perturbation_curve(m, b, undirected="mean", ratios=(0.3, 0.6), order=want.score)
    cg = perturbation_curve(m, f, undirected="mean", ratios=(0.3, 0.6), order=want.score[perm])
    assert (cw["insertion"] - cg["insertion"]).abs().max().item() < 1e-6 and (cw["deletion"] - cg["deletion"]).abs().max().item() < 1e-6
