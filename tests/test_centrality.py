"""cal_centrality through libcalhost (cal_amd/csrc_host/calhost.cpp) against the exact restatement of tests/centrality_oracle.py:
integers bit-equal, bc / ebc within gamma_k of the exact rationals, pr within the contraction bound of the exact stationary
vector; the oracle tied to networkx; seeded defects that the same inputs and bounds must notice; the drivers
(structural_baseline, explanation_locality) against tests/explain_oracle.py's ranking of the oracle's scores; the reference's
``cent`` feature switch; the ABI.  tests/test_gpu_centrality.py sends the same cases through libcalhip.so."""
import argparse
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.centrality import (KINDS, centrality, eval_explanation_locality, eval_structural_baseline, explanation_locality,
                                hop_distance, structural_baseline, structural_scores)
from cal_amd.data import Batch, Data, DataLoader
from oracle import cal_oracle as CO
from tests import centrality_oracle as O
from tests.explain_oracle import rank_oracle

ALPHA, TOL, MAX_ITER = 0.85, 1e-12, 1000


def batch_of(cs, dev="cpu"):
    """The cases as a batch object (edge columns grouped by graph, ptr / edge_ptr given) and their ``sources`` mask."""
    ei, ptr, eptr, batch, src = O.batch_arrays(cs)
    b = Batch()
    b.x = torch.ones(len(batch), 1)
    b.feat = None
    b.edge_index = torch.from_numpy(ei).reshape(2, -1)
    b.batch = torch.from_numpy(batch)
    b.y = torch.zeros(len(cs), dtype=torch.long)
    b.ptr, b.edge_ptr, b.num_graphs = torch.from_numpy(ptr), torch.from_numpy(eptr), len(cs)
    n, m = np.diff(ptr), np.diff(eptr)
    b.max_nodes, b.max_edges = int(n.max()) if len(cs) else 0, int(m.max()) if len(cs) else 0
    b.no_self_loops = False
    return b.to(dev), torch.from_numpy(src).to(dev)


def run(cs, dev="cpu", with_sources=True, **kw):
    """-> (the outputs of one call as numpy arrays -- ``O.judge``'s ``got`` --, the ``Centrality``)"""
    b, src = batch_of(cs, dev)
    c = centrality(b, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER, sources=src if with_sources else None, **kw)
    got = {k: getattr(c, k).cpu().numpy() for k in ("far", "reach", "ecc", "deg", "bc", "ebc", "pr", "pr_iters", "skipped")}
    got["hop"] = c.hop.cpu().numpy() if c.hop is not None else None
    got["ignored"] = int(c.ignored.cpu())
    got["closeness"] = c.closeness().cpu().numpy()
    return got, c


def same_bits(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert x.dtype == y.dtype and torch.equal(x.cpu().view(torch.uint8), y.cpu().view(torch.uint8))


CASES = O.cases()
SMALL = [c for c in CASES if c["n"] <= 7]
BY_NAME = {c["name"]: c for c in CASES}


# ---- 1. the contract ------------------------------------------------------------------------------------------------------------
def case_all_in_one_batch(dev):
    """Every case in ONE call: a graph's neighbours in the batch must not show."""
    got, _ = run(CASES, dev)
    assert O.judge(CASES, got, ALPHA, TOL, MAX_ITER) == []
    return got


def case_one_by_one(dev):
    for c in SMALL + [c for c in CASES if c["name"] in ("ba65", "k64")]:
        got, _ = run([c], dev)
        assert O.judge([c], got, ALPHA, TOL, MAX_ITER) == [], c["name"]


def case_reverse_and_duplicate_columns(dev):
    """A column, its reverse and its duplicates carry the same bits; self loops and columns that leave carry 0."""
    got, _ = run([BY_NAME["messy"]], dev)                      # the path 0-1-2-3-4 under one-way, doubled and stray columns
    assert got["ebc"].tolist() == [8.0, 8.0, 12.0, 0.0, 12.0, 0.0, 0.0, 0.0, 8.0, 8.0, 8.0] and got["ignored"] == 3
    g = BY_NAME["grid16"]
    got, _ = run([g], dev)
    half = len(g["cols"]) // 2
    assert np.array_equal(got["ebc"][:half].view(np.uint64), got["ebc"][half:].view(np.uint64))


def case_closed_forms(dev):
    """star: the hub's bc is (n - 1)(n - 2) exactly, every edge's raw ebc 2 (n - 1); path: ecc of an end n - 1; K: all bc 0."""
    got, c = run([BY_NAME["star256"], BY_NAME["path256"], BY_NAME["k64"]], dev)
    assert got["bc"][0] == 255.0 * 254.0 and not got["bc"][1:256].any()
    assert (got["ebc"][:510] == 2.0 * 255.0).all()
    assert got["ecc"][256] == 255 and got["ecc"][256 + 128] == 128 and got["far"][256] == 255 * 256 // 2
    assert not got["bc"][512:].any() and (got["ebc"][1020:] == 2.0).all()
    assert torch.equal(c.betweenness()[:1].cpu(), torch.ones(1, dtype=torch.float64))


def case_hop_only(dev):
    b, src = batch_of(CASES, dev)
    hop = hop_distance(b, src)
    want = np.concatenate([np.asarray(O.oracle(c)["hop"] if c["sources"] is not None else [-1] * c["n"], dtype=np.int32)
                           for c in CASES])
    assert hop.dtype == torch.int32 and np.array_equal(hop.cpu().numpy(), want)
    every = hop_distance(b, torch.ones_like(src))
    assert not every.any()


def case_unordered_columns(dev):
    """Columns that are not grouped by graph: reordered inside, ebc handed back in the caller's order."""
    b, src = batch_of([BY_NAME["house"], BY_NAME["path7"], BY_NAME["two-components"]], dev)
    want = centrality(b, sources=src)
    perm = torch.randperm(b.edge_index.size(1), generator=torch.Generator().manual_seed(5)).to(b.edge_index.device)
    u = SimpleNamespace(edge_index=b.edge_index[:, perm].contiguous(), batch=b.batch, num_graphs=b.num_graphs, x=b.x)
    got = centrality(u, sources=src)
    same_bits([got.far, got.bc, got.pr, got.hop], [want.far, want.bc, want.pr, want.hop])
    assert torch.equal(got.ebc, want.ebc[perm]) and torch.equal(got.edge_nodes, want.edge_nodes[perm])


GENERAL = [case_all_in_one_batch, case_one_by_one, case_reverse_and_duplicate_columns, case_closed_forms, case_hop_only,
           case_unordered_columns]


@pytest.mark.parametrize("case", GENERAL, ids=lambda c: c.__name__[5:])
def test_host_twin(case):
    case("cpu")


def test_host_twin_twice_gives_the_same_bits():
    a, b = run(CASES)[1], run(CASES)[1]
    same_bits(a[:11], b[:11])


def test_host_twin_has_no_node_limit():
    n = 300
    got, c = run([O._case("star300", n, O.star(n), O._mask(n, {n - 1}))])
    assert got["skipped"].tolist() == [0] and got["bc"][0] == (n - 1.0) * (n - 2.0) and got["hop"][0] == 1 and got["hop"][5] == 2
    assert got["reach"].tolist() == [n] * n and got["ecc"][0] == 1 and got["deg"][0] == n - 1


def test_argument_checks():
    b, src = batch_of(SMALL)
    for kw in (dict(alpha=1.0), dict(alpha=-0.1), dict(tol=-1.0), dict(max_iter=-1)):
        with pytest.raises(ValueError):
            centrality(b, **kw)
    with pytest.raises(ValueError):
        hop_distance(b, None)
    with pytest.raises((TypeError, ValueError)):
        centrality(b, sources=src[:-1])
    with pytest.raises(ValueError):
        structural_scores(b, "eigenvector")
    with pytest.raises(ValueError):
        structural_scores(b, "edge_betweenness", use="nodes")
    assert centrality(b, max_iter=0).pr_iters.tolist() == [0] * len(SMALL)
    with pytest.raises(_lib.CalError):
        _lib.call("cal_centrality", None, 0, 1, None, None, 1, None, 0.85, 1e-12, 10, *([None] * 11), None, 0, None, host=True)


# ---- 2. the oracle against networkx ---------------------------------------------------------------------------------------------
def _nx_graph(nx, c):
    G = nx.Graph()
    G.add_nodes_from(range(c["n"]))
    G.add_edges_from((u, v) for u, v in c["cols"] if 0 <= u < c["n"] and 0 <= v < c["n"] and u != v)
    return G


@pytest.mark.parametrize("c", [c for c in CASES if 0 < c["n"] <= 129], ids=lambda c: c["name"])
def test_oracle_is_networkx(c):
    """networkx is not the yardstick -- the exact restatement is -- but the two must say the same, within 1e-9."""
    nx = pytest.importorskip("networkx")
    G, n, o = _nx_graph(nx, c), c["n"], O.oracle(c)
    bc, eb, cl = nx.betweenness_centrality(G), nx.edge_betweenness_centrality(G), nx.closeness_centrality(G)
    pr = nx.pagerank(G, alpha=ALPHA, tol=1e-13, max_iter=5000)
    sb = 1.0 / ((n - 1) * (n - 2)) if n > 2 else 0.5
    se = 1.0 / (n * (n - 1)) if n > 1 else 0.5
    for v in range(n):
        assert abs(float(o["bc"][v]) * sb - bc[v]) < 1e-9 and abs(o["closeness"][v] - cl[v]) < 1e-9 and abs(o["pr"][v] - pr[v]) < 1e-9
    for (u, v), x in zip(c["cols"], o["ebc"]):
        if 0 <= u < n and 0 <= v < n and u != v:
            assert abs(float(x) * se - eb[(min(u, v), max(u, v))]) < 1e-9
    for comp in nx.connected_components(G):
        ecc = nx.eccentricity(G.subgraph(comp))
        assert all(o["ecc"][v] == ecc[v] and o["reach"][v] == len(comp) for v in comp)
    if c["sources"] is not None and any(c["sources"]):
        d = nx.multi_source_dijkstra_path_length(G, {v for v in range(n) if c["sources"][v]})
        assert o["hop"] == [d.get(v, -1) for v in range(n)]


# ---- 3. seeded defects: these inputs and these bounds notice each -----------------------------------------------------------------
def _as_got(cs, outs, alpha=ALPHA):
    got = {k: np.concatenate([np.asarray(o[k], dtype=np.int64) for o in outs]) for k in ("far", "reach", "ecc", "deg")}
    got["hop"] = np.concatenate([np.asarray(o["hop"] if o["hop"] is not None else [0] * c["n"], dtype=np.int64) for c, o in zip(cs, outs)])
    got["bc"] = np.asarray([float(x) for o in outs for x in o["bc"]])
    got["ebc"] = np.asarray([float(x) for o in outs for x in o["ebc"]])
    got["pr"] = np.concatenate([np.asarray(o["pr"], dtype=np.float64) for o in outs])
    got["pr_iters"] = np.asarray([o["pr_iters"] for o in outs])
    got["skipped"] = np.zeros(len(cs), dtype=np.int64)
    got["ignored"] = sum(o["ignored"] for o in outs)
    got["closeness"] = np.asarray([x for c, o in zip(cs, outs) for x in o["closeness"]])
    return got


DEFECT_CASES = [c for c in CASES if c["name"] in ("two-components", "house", "path7", "messy", "ba65", "q6")]


def test_the_restatement_rounded_to_fp64_meets_its_own_bounds():
    assert O.judge(DEFECT_CASES, _as_got(DEFECT_CASES, [O.oracle(c) for c in DEFECT_CASES])) == []


@pytest.mark.parametrize("defect", O.DEFECTS)
def test_seeded_defects_are_noticed(defect):
    outs = []
    for c in DEFECT_CASES:
        o = dict(O.brandes(c["n"], c["cols"], c["sources"], defect=defect))
        o["pr"] = O.pagerank_exact(o["adj"], ALPHA, defect=defect)
        o["pr_iters"] = O.oracle(c)["pr_iters"]
        o["closeness"] = O.closeness(o["far"], o["reach"], c["n"], defect=defect)
        outs.append(o)
    bad = O.judge(DEFECT_CASES, _as_got(DEFECT_CASES, outs))
    print(defect, "->", bad)
    assert bad, defect


# ---- 4. the drivers against the oracle's scores under tests/explain_oracle.py's ranking -------------------------------------------
def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add")
    d.update(kw)
    return argparse.Namespace(**d)


def _cpu_model(name="CausalGCN", feat=10, seed=3):
    from cal_amd import model as M
    torch.manual_seed(seed)
    sd = CO.init_state(name, feat, 4, hidden=32, layers=2, heads=4)
    m = getattr(M, name)(feat, 4, _args())
    m.load_state_dict(sd, strict=name != "CausalGIN")
    return m


def _graphs(b):
    """The graphs of a CPU batch as oracle cases (sources: the planted motif's nodes)."""
    node_gt = spmotif.ground_truth(b)[0]
    out = []
    for g in range(int(b.num_graphs)):
        lo, hi, elo, ehi = int(b.ptr[g]), int(b.ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        cols = [(int(u) - lo, int(v) - lo) for u, v in b.edge_index[:, elo:ehi].t().tolist()]
        out.append(O._case("g%d" % g, hi - lo, cols, [int(x) for x in node_gt[lo:hi]]))
    return out


def _oracle_scores(b, kind, use):
    """float32 scores of ``kind`` from the EXACT centralities, normalised as networkx does, in fp64 before the cast."""
    out = []
    for c in _graphs(b):
        n, o = c["n"], O.brandes(c["n"], c["cols"])
        node = {"degree": [float(d) for d in o["deg"]], "closeness": O.closeness(o["far"], o["reach"], n),
                "betweenness": [float(x) / ((n - 1) * (n - 2)) if n > 2 else float(x) / 2 for x in o["bc"]],
                "pagerank": list(O.pagerank_exact(o["adj"], ALPHA))}
        if kind == "edge_betweenness":
            out += [float(x) / (n * (n - 1)) if n > 1 else float(x) / 2 for x in o["ebc"]]
        elif use == "nodes":
            out += node[kind]
        else:
            out += [(node[kind][u] + node[kind][v]) * 0.5 for u, v in c["cols"]]
    return np.asarray(out, dtype=np.float64).astype(np.float32)


def _means(met):
    kg, hits, P, auc = met.T
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"precision": float(np.mean((hits / kg)[kg > 0])), "recall": float(np.mean((hits / P)[P > 0])),
                "auc": float(np.nanmean(auc))}


def _baseline_oracle(m, b, kinds, use, undirected, k):
    from cal_amd.explain import edge_twins, explain
    from tests.occlude_oracle import agreement_counts_np, agreement_metrics_np
    node_gt, edge_gt = spmotif.ground_truth(b)
    ex = explain(m, b, k=k, undirected=undirected, edge_gt=edge_gt, node_gt=node_gt)
    B = int(b.num_graphs)
    if use == "edges":
        att, gt, seg = ex.edge_score.numpy(), edge_gt.numpy().copy(), b.edge_ptr.numpy()
        keep = np.ones(len(gt), bool)
        if undirected is not None:                       # one element per undirected edge: the lower column of a pair
            twin = edge_twins(b)[0].numpy()
            keep = ~((twin >= 0) & (twin < np.arange(len(twin))))
            gt = gt | (gt[np.clip(twin, 0, None)] & (twin >= 0))
    else:
        att, gt, seg, keep = ex.node_score.numpy(), node_gt.numpy(), b.ptr.numpy(), np.ones(int(b.ptr[-1]), bool)
    gid = np.repeat(np.arange(B), np.diff(seg))
    seg_r = np.concatenate([[0], np.cumsum(np.bincount(gid[keep], minlength=B))])
    mx = int(np.diff(seg_r).max())
    amask, _, amet = rank_oracle(att[keep], seg_r, k=k, gt=gt[keep])
    res = {"graphs": B, "chance": float(np.mean(amet[:, 2] / np.diff(seg_r))), "attention": _means(amet), "kinds": {}}
    for kd in kinds:
        name, sign = (kd[1:], -1.0) if kd.startswith("-") else (kd, 1.0)
        s = (sign * _oracle_scores(b, name, use))[keep]
        smask, _, smet = rank_oracle(s, seg_r, k=k, gt=gt[keep])
        d = _means(smet)
        ag = agreement_metrics_np(agreement_counts_np(att[keep], s, seg_r, mx, None, k=0 if k == "gt" else k))
        if k == "gt":
            inter = np.bincount(gid[keep], weights=(amask & smask).astype(float), minlength=B)
            with np.errstate(invalid="ignore", divide="ignore"):
                ag[:, 2] = np.where(amet[:, 0] > 0, inter / (2 * amet[:, 0] - inter), np.nan)
        for j, key in enumerate(("rho", "tau", "jaccard")):
            ok = ~np.isnan(ag[:, j])
            d[key] = float(ag[ok, j].mean()) if ok.any() else float("nan")
            d[key + "_undefined"] = int((~ok).sum())
        res["kinds"][kd] = d
    return res


def _same_report(a, b, tol=1e-12):
    assert a.keys() == b.keys(), (a.keys(), b.keys())
    for key in a:
        if isinstance(a[key], dict):
            _same_report(a[key], b[key], tol)
        elif isinstance(a[key], float):
            assert (a[key] != a[key] and b[key] != b[key]) or abs(a[key] - b[key]) <= tol, (key, a[key], b[key])
        else:
            assert a[key] == b[key], (key, a[key], b[key])


@pytest.fixture(scope="module")
def driver_setup():
    m = _cpu_model()
    m.train()
    gs = spmotif.train_mix(8, node_num=6, seed=4)
    return m, gs, Batch.from_data_list(gs)


@pytest.mark.parametrize("use,undirected,k", [("edges", "mean", "gt"), ("edges", None, 3), ("nodes", None, "gt"), ("edges", "max", 2)])
def test_structural_baseline_is_the_oracles_ranking_of_the_oracles_scores(driver_setup, use, undirected, k):
    m, gs, b = driver_setup
    kinds = KINDS if use == "edges" else KINDS[:4]
    got = structural_baseline(m, b, use=use, undirected=undirected, k=k)
    assert m.training and list(got["kinds"]) == list(kinds)
    _same_report(got, _baseline_oracle(m, b, kinds, use, undirected, k))
    gt = spmotif.ground_truth(b)
    share = gt[1] if use == "edges" else gt[0]
    if undirected is None:                               # chance is the ground-truth share, graph by graph
        seg = (b.edge_ptr if use == "edges" else b.ptr).tolist()
        assert got["chance"] == pytest.approx(np.mean([float(share[lo:hi].float().mean()) for lo, hi in zip(seg, seg[1:])]), abs=1e-7)
    assert 0.0 < got["chance"] < 1.0
    _same_report(m.structural_baseline(b, use=use, undirected=undirected, k=k), got)


def test_a_leading_minus_reverses_the_ranking(driver_setup):
    m, gs, b = driver_setup
    for kind in KINDS:
        s, r = structural_scores(b, kind), structural_scores(b, "-" + kind)
        assert s.dtype == torch.float32 and torch.equal(r, -s)
    assert structural_scores(b, "pagerank", use="nodes").shape == (int(b.ptr[-1]),)
    got = structural_baseline(m, b, kinds=("betweenness", "-betweenness"), k=3)
    up, down = got["kinds"]["betweenness"], got["kinds"]["-betweenness"]
    assert up["auc"] + down["auc"] == pytest.approx(1.0, abs=1e-12)
    assert up["rho"] == pytest.approx(-down["rho"], abs=1e-12) and up["tau"] == pytest.approx(-down["tau"], abs=1e-12)


def test_eval_structural_baseline_is_the_sum_over_its_batches(driver_setup):
    m, gs, b = driver_setup
    ev = eval_structural_baseline(m, DataLoader(gs, 3, shuffle=False), "cpu")
    parts = [structural_baseline(m, Batch.from_data_list(gs[i:i + 3])) for i in range(0, len(gs), 3)]
    G = sum(p["graphs"] for p in parts)
    assert ev["graphs"] == G == len(gs)
    assert ev["chance"] == pytest.approx(sum(p["chance"] * p["graphs"] for p in parts) / G, abs=1e-12)
    for key in ("precision", "recall", "auc"):           # (every SPMotif graph has a motif and a base: all three defined)
        assert ev["attention"][key] == pytest.approx(sum(p["attention"][key] * p["graphs"] for p in parts) / G, abs=1e-12)
        for kd in KINDS:
            assert ev["kinds"][kd][key] == pytest.approx(sum(p["kinds"][kd][key] * p["graphs"] for p in parts) / G, abs=1e-12)
    for kd in KINDS:
        for key in ("rho", "tau", "jaccard"):
            w = [p["graphs"] - p["kinds"][kd][key + "_undefined"] for p in parts]
            assert ev["kinds"][kd][key + "_undefined"] == G - sum(w)
            if sum(w):
                want = sum(p["kinds"][kd][key] * wi for p, wi in zip(parts, w) if wi) / sum(w)
                assert ev["kinds"][kd][key] == pytest.approx(want, abs=1e-12)
    whole = structural_baseline(m, b)
    _same_report(eval_structural_baseline(m, DataLoader(gs, len(gs), shuffle=False), "cpu"), whole)


@pytest.mark.parametrize("undirected,k,ratio", [("mean", "gt", None), (None, 4, None), ("mean", None, 0.3)])
def test_explanation_locality_is_the_oracles_distances_of_the_selected_edges(driver_setup, undirected, k, ratio):
    from cal_amd.explain import edge_twins, explain
    m, gs, b = driver_setup
    got = explanation_locality(m, b, ratio=ratio, k=k, undirected=undirected)
    node_gt, edge_gt = spmotif.ground_truth(b)
    ex = explain(m, b, ratio=ratio, k=k, undirected=undirected, edge_gt=edge_gt, node_gt=node_gt)
    hop = np.concatenate([np.asarray(O.brandes(c["n"], c["cols"], c["sources"])["hop"]) for c in _graphs(b)])
    assert np.array_equal(hop_distance(b, node_gt).numpy(), hop)
    sel, gt = ex.edge_mask.numpy().copy(), edge_gt.numpy().copy()
    if undirected is not None:
        twin = edge_twins(b)[0].numpy()
        sel &= ~((twin >= 0) & (twin < np.arange(len(twin))))
        gt = gt | (gt[np.clip(twin, 0, None)] & (twin >= 0))
    ends = hop[b.edge_index.numpy()]
    d = np.where(ends < 0, 1 << 30, ends).min(0)
    n = int(sel.sum())
    wrong = sel & ~gt & (d < (1 << 30))
    want = {"edges": n, "in_motif": float((sel & gt).sum()) / n, "hop0": float((sel & (d == 0)).sum()) / n,
            "hop1": float((sel & (d == 1)).sum()) / n, "hop2": float((sel & (d == 2)).sum()) / n,
            "hop3plus": float((sel & (d >= 3)).sum()) / n, "wrong": int((sel & ~gt).sum()),
            "wrong_mean_hop": float(d[wrong].mean()) if wrong.any() else float("nan")}
    _same_report(got, want)
    assert got["in_motif"] <= got["hop0"]                # a motif edge joins two motif nodes
    _same_report(m.explanation_locality(b, ratio=ratio, k=k, undirected=undirected), got)


def test_eval_explanation_locality_is_the_sum_over_its_batches(driver_setup):
    m, gs, b = driver_setup
    ev = eval_explanation_locality(m, DataLoader(gs, 3, shuffle=False), "cpu")
    parts = [explanation_locality(m, Batch.from_data_list(gs[i:i + 3]), k="gt") for i in range(0, len(gs), 3)]
    n = sum(p["edges"] for p in parts)
    assert ev["edges"] == n and ev["wrong"] == sum(p["wrong"] for p in parts)
    for key in ("in_motif", "hop0", "hop1", "hop2", "hop3plus"):
        assert ev[key] == pytest.approx(sum(p[key] * p["edges"] for p in parts) / n, abs=1e-12)


# ---- 5. the reference's `cent` switch -------------------------------------------------------------------------------------------
def test_tu_cent_switch(tmp_path):
    nx = pytest.importorskip("networkx")
    from cal_amd import tu
    from tests.test_tu import _write
    _write(str(tmp_path))
    plain = tu.get_dataset("TOY", "deg+odeg4", root=str(tmp_path))
    ds = tu.get_dataset("TOY", "deg+odeg4+cent", root=str(tmp_path))
    assert ds.num_features == plain.num_features + 3
    for g, p in zip(ds, plain):
        assert torch.equal(g.x[:, :-3], p.x) and g.x.dtype == torch.float32
        G = nx.Graph()
        G.add_nodes_from(range(g.num_nodes))
        G.add_edges_from(g.edge_index.t().tolist())
        cl, bc, pr = nx.closeness_centrality(G), nx.betweenness_centrality(G), nx.pagerank(G, tol=1e-13, max_iter=5000)
        want = torch.tensor([[cl[i], bc[i], pr[i]] for i in range(g.num_nodes)], dtype=torch.float64)
        assert (g.x[:, -3:].double() - want).abs().max() <= 2.0 ** -23          # equal to float32
    assert tu.parse_feat_options("deg+odeg4+cent") == {"degree": True, "onehot_maxdeg": 4, "cent": True}
    assert tu.parse_feat_options("deg") == {"degree": True, "onehot_maxdeg": None, "cent": False}
    for bad in ("deg+ak3", "deg+groupd2", "deg+reall", "deg+randa0.5", "deg+randd0.5"):
        with pytest.raises(NotImplementedError):
            tu.parse_feat_options(bad)
    assert tu.parse_feat_str("deg+odeg100") == (True, 100) and tu.parse_feat_str("odeg7") == (True, 7)
    with pytest.raises(NotImplementedError):                                     # the older parser still refuses cent
        tu.parse_feat_str("deg+cent")


# ---- 6. the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi():
    pr = _lib.parse_header()
    assert len(pr["cal_centrality"][1]) == 24 and pr["cal_centrality"][2][:7] == ["edge_index", "E", "N", "ptr", "edge_ptr", "B", "sources"]
    assert pr["cal_centrality"][2][10:] == ["far", "reach", "ecc", "deg", "bc", "ebc", "pr", "pr_iters", "hop", "skipped", "totals",
                                            "ws", "ws_bytes", "stream"]
    assert len(pr["cal_centrality_ws"][1]) == 1
    assert "cal_centrality" in _lib.HOST_SYMBOLS and "cal_centrality_ws" in _lib.HOST_SYMBOLS
    import ctypes
    host = ctypes.CDLL(_lib.HOST_LIB_PATH)
    assert host.cal_centrality and host.cal_centrality_ws
    if os.path.exists(_lib.LIB_PATH):
        hip = ctypes.CDLL(_lib.LIB_PATH)
        assert hip.cal_centrality and hip.cal_centrality_ws
    import cal_amd
    assert cal_amd.centrality.centrality is centrality and cal_amd.structural_baseline is structural_baseline
