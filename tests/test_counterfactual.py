"""Counterfactual explanations on the CPU: the host twins of cal_subset_count / cal_subset_write and cal_beam_step against the
plain-int restatements bit for bit, the exported symbols, subset_batch against occlude_batch and coalition_batch, the seeded
defects the case lists must notice, and counterfactual() / ranking_flip() / eval_counterfactual() of a CPU-resident model: every
found set flips, beam=1 is the greedy loop over occlude_batch, a wide beam finds the brute-force minimum."""
import argparse
import random
import subprocess

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.coalition import coalition_batch
from cal_amd.counterfactual import (Counterfactual, beam_step, counterfactual, counterfactual_report, eval_counterfactual,
                                    pack_bits, ranking_flip, subset_batch, unpack_bits)
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import _Layout, _log_probs, _untiled, edge_twins, extract_subgraph
from cal_amd.occlude import occlude_batch
from oracle import cal_oracle as O
from tests.coalition_oracle import rank_keys, representatives
from tests.counterfactual_oracle import (BEAM_DEFECTS, SUBSET_DEFECTS, balance_head, beam_cases, beam_oracle, binom_ok,
                                         brute_min_flip, check_subset, cut_graphs, greedy_occlude, prefix_flip, run_beam,
                                         same_subset, subset_cases, subset_oracle, subset_want)

CASES = subset_cases()
BEAMS = beam_cases()
SYMBOLS = ("cal_subset_ws", "cal_subset_count", "cal_subset_write", "cal_beam_step")
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: below it a probability margin does not decide a comparison


def _call(c, dev="cpu"):
    t = lambda v: None if v is None else v.to(dev)
    return subset_batch(c["b"], t(c["rg"]), t(c["bits"]), rep_row=t(c["rrow"]), rep_flip=t(c["rflip"]), use=c["use"], twin=t(c["twin"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_restatement(name):
    check_subset(_call(CASES[name]), CASES[name], subset_want(name))


def test_abi_symbols_are_exported_by_both_libraries():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_subset_count"][1]) == 22 and len(protos["cal_subset_write"][1]) == 30
    assert len(protos["cal_subset_ws"][1]) == 4 and len(protos["cal_beam_step"][1]) == 25


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src", "y"):
        assert torch.equal(getattr(u, key), getattr(v, key)), key
    fu, fv = (u.feat if u.x is None else u.x), (v.feat if v.x is None else v.x)
    assert torch.equal(fu, fv) and (u.x is None) == (v.x is None)
    assert (u.max_nodes, u.max_edges, u.empty_graphs, u.num_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs, v.num_graphs)


@pytest.mark.parametrize("use,with_twin", [("edges", False), ("edges", True), ("nodes", False)])
def test_no_bits_and_a_flip_is_occlude_batch(use, with_twin):
    b = CASES["spmotif_edges"]["b"]
    off = b.edge_ptr if use == "edges" else b.ptr
    M = int(off[-1])
    re = torch.cat([torch.arange(0, M, 3), torch.tensor([-1])])           # ... and a control replica
    rg = (torch.searchsorted(off, re.clamp(min=0), right=True) - 1)
    twin = edge_twins(b)[0] if with_twin else None
    got = subset_batch(b, rg, None, rep_flip=torch.where(re >= 0, re - off[rg], re), use=use, twin=twin)
    _same(got, occlude_batch(b, rg, re, use=use, twin=twin))


@pytest.mark.parametrize("use", ["edges", "nodes"])
@pytest.mark.parametrize("invert", [False, True])
def test_bits_packed_from_a_key_is_coalition_batch(use, invert):
    b = CASES["spmotif_edges"]["b"]
    seg, mx = (b.edge_ptr, b.max_edges) if use == "edges" else (b.ptr, b.max_nodes)
    M, B = int(seg[-1]), b.num_graphs
    g = torch.Generator().manual_seed(3)
    key = torch.randint(-1, 9, (3, M), generator=g, dtype=torch.int32)
    rg, rrow, rth = torch.randint(0, B, (40,), generator=g), torch.randint(0, 3, (40,), generator=g), torch.randint(0, 9, (40,), generator=g)
    # one bitset row per replica: the elements of its graph with key < thresh (inverted: >=)
    rows = []
    for r in range(40):
        stay = (key[rrow[r]] >= rth[r]) if invert else (key[rrow[r]] < rth[r])
        rows.append(pack_bits(stay, seg, mx)[rg[r]])
    bits = torch.stack(rows)
    assert torch.equal(unpack_bits(pack_bits(stay, seg, mx), seg, M), stay)
    got = subset_batch(b, rg, bits, rep_row=torch.arange(40), use=use)
    _same(got, coalition_batch(b, rg, rth, key, rep_row=rrow, use=use, invert=invert))


def test_ungrouped_columns_take_the_callers_local_numbering():
    c = CASES["spmotif_edges"]
    b = c["b"]
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
    tw_f = edge_twins(f)[0]                                # in the caller's numbering
    res = subset_batch(f, c["rg"], c["bits"], rep_row=c["rrow"], rep_flip=c["rflip"], twin=tw_f)
    r = subset_oracle(dict(c, b=g, twin=edge_twins(g)[0]))
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src"):
        assert torch.equal(getattr(res, k), r[k]), k
    assert torch.equal(res.edge_src, order[r["edge_src"]])               # edge_src names the caller's own columns


def test_argument_errors():
    c = CASES["spmotif_edges"]
    b, rg, bits = c["b"], c["rg"], c["bits"]
    with pytest.raises(ValueError):
        subset_batch(b, rg, bits)                                         # eight rows and no rep_row
    with pytest.raises(ValueError):
        subset_batch(b, rg, bits, rep_row=c["rrow"][:-1])
    with pytest.raises(ValueError):
        subset_batch(b, rg, bits, rep_row=c["rrow"], rep_flip=c["rflip"][:-1])
    with pytest.raises(TypeError):
        subset_batch(b, None, bits, rep_row=c["rrow"])
    with pytest.raises(TypeError):
        subset_batch(b, rg, bits.long(), rep_row=c["rrow"])
    with pytest.raises(ValueError):
        subset_batch(b, rg, bits, rep_row=c["rrow"], use="both")
    with pytest.raises(ValueError):
        subset_batch(b, rg, bits, rep_row=c["rrow"], twin=torch.zeros(3, dtype=torch.int32))
    for fn in (counterfactual, ranking_flip, counterfactual_report):
        for kw in (dict(use="both"), dict(undirected="sum"), dict(head="x"), dict(chunk=0), dict(use="nodes", undirected="mean"),
                   dict(max_remove=-1)):
            with pytest.raises(ValueError):
                fn(None, b, **kw)
    for beam in (0, 17, 2.5):
        with pytest.raises(ValueError):
            counterfactual(None, b, beam=beam)
    m, _ = _cpu_model("CausalGCN", 10)
    wide = Batch.from_data_list(spmotif.train_mix(2, node_num=7, seed=3))
    with pytest.raises(ValueError, match="beam x players"):              # 16 x the columns of a graph > 2048 candidates
        counterfactual(m, wide, beam=16)
    with pytest.raises(ValueError, match="elements"):                    # a 5000-node graph: more than 2048 elements
        counterfactual(m, CASES["large_edges"]["b"], beam=1)
    with pytest.raises(ValueError):
        ranking_flip(m, b, torch.zeros(5))


# ---- the beam step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BEAMS))
def test_host_beam_step_equals_restatement(name):
    c = BEAMS[name]
    want, got = beam_oracle(c), run_beam(c, "cpu")
    for k in want:
        assert got[k] == want[k], k
    if name == "cap":                                                     # exactly cal_explain_lds_cap() candidates, and one more
        assert want["status"][:2] == [0, 2] and want["n_out"][0] > 0 and want["n_out"][1] == 0
    if "seed" in name:                                                    # exactly max_cand = 40 candidates, and one more
        assert want["status"][10:12] == [0, 2] and want["n_out"][11] == 0 and (want["n_out"][10] > 0 or want["done"][10])


def test_beam_step_rejects_what_it_cannot_hold():
    c = BEAMS["beam4_seed0"]
    with pytest.raises(ValueError):
        run_beam(dict(c, max_cand=2049), "cpu")
    with pytest.raises(ValueError):
        run_beam(dict(c, beam=17), "cpu")


# ---- the case lists notice seeded defects of the restatements -------------------------------------------------------------------
@pytest.mark.parametrize("defect", SUBSET_DEFECTS)
def test_subset_cases_notice_a_seeded_defect(defect):
    assert same_subset(subset_oracle(CASES["twin"]), subset_want("twin"))    # the restatement against itself
    seen = [n for n in sorted(CASES) if not n.startswith("large") and not same_subset(subset_oracle(CASES[n], defect), subset_want(n))]
    print(defect, "noticed by", seen)
    assert seen


@pytest.mark.parametrize("defect", BEAM_DEFECTS)
def test_beam_cases_notice_a_seeded_defect(defect):
    seen = [n for n in sorted(BEAMS) if beam_oracle(BEAMS[n], defect) != beam_oracle(BEAMS[n])]
    print(defect, "noticed by", seen)
    assert seen


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


_SETUP = {}


def _setup():
    """Eight SPMotif graphs cut to at most 8 (four of them: 5) undirected edges and a model balanced on them (shared)."""
    if not _SETUP:
        gs = cut_graphs(4, 8, 0) + cut_graphs(4, 5, 100)
        b = Batch.from_data_list(gs)
        m, _ = _cpu_model("CausalGCN", 10)
        _SETUP.update(gs=gs, b=b, m=balance_head(m, b), twin=edge_twins(b)[0])
    return _SETUP["m"], _SETUP["b"], _SETUP["gs"], _SETUP["twin"]


def _argmax_without(m, b, removed, use="edges", head=1):
    """The argmax of ``b`` without the marked elements, by an independent extraction and forward."""
    sub = extract_subgraph(b, edge_mask=~removed) if use == "edges" else extract_subgraph(b, node_mask=~removed, relabel=True)
    m.eval()
    with torch.no_grad():
        return _log_probs(m, sub)[head].argmax(-1)


@pytest.mark.parametrize("use,undirected,beam", [("edges", "mean", 4), ("edges", None, 2), ("nodes", None, 4), ("edges", "max", 1)])
def test_cpu_found_sets_flip_and_sizes_count_the_removed_players(use, undirected, beam):
    m, b, _, twin = _setup()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    py0, t0 = random.getstate(), torch.get_rng_state()
    cf = m.counterfactual(b, use=use, undirected=undirected, beam=beam, max_remove=4, chunk=97)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    assert isinstance(cf, Counterfactual) and cf.removed.dtype == torch.bool and cf.size.dtype == torch.long
    M = int(b.edge_index.size(1)) if use == "edges" else int(b.batch.numel())
    assert cf.removed.shape == (M,) and cf.size.shape == (8,) and int(cf.found.sum()) >= 3
    assert torch.equal(cf.found, cf.size >= 0) and torch.equal(cf.found, cf.y_cf >= 0) and torch.equal(cf.found, ~cf.p_cf.isnan())
    rep = representatives(twin if undirected else None, M)
    gid = b.batch[b.edge_index[0]] if use == "edges" else b.batch
    count = torch.zeros(8, dtype=torch.long).index_add_(0, gid, (cf.removed & rep).long())
    assert torch.equal(torch.where(cf.found, count, torch.full_like(count, -1)), cf.size)
    assert not bool(cf.removed[~cf.found[gid]].any()) and int(cf.size.max()) <= 4 and cf.rounds <= 4
    if undirected:                                                        # symmetric: both columns of an undirected edge
        pair = twin >= 0
        assert torch.equal(cf.removed[pair], cf.removed[twin[pair].long()]) and torch.equal(cf.twin, twin)
    # every found set really flips: an independent forward of the extraction of ~removed
    after = _argmax_without(m, b, cf.removed, use)
    assert bool((after != cf.yhat)[cf.found].all()) and torch.equal(after[cf.found], cf.y_cf[cf.found])
    assert bool((after == cf.yhat)[~cf.found].all())
    assert cf.forwards >= 1 + cf.rounds and cf.replicas >= cf.rounds
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_cpu_beam_one_is_the_greedy_loop_over_occlude_batch():
    m, b, _, twin = _setup()
    cf = counterfactual(m, b, undirected="mean", beam=1, max_remove=4)
    n = torch.zeros(8, dtype=torch.long).index_add_(0, b.batch[b.edge_index[0]], representatives(twin, twin.numel()).long())
    removed, size, gap = greedy_occlude(m, b, twin, torch.clamp(n, max=4).tolist())
    print("sizes", size, "smallest gap between a round's best two p", min(gap))
    assert cf.size.tolist() == size and torch.equal(cf.removed, removed)
    assert int(cf.found.sum()) >= 3


def test_cpu_a_wide_beam_finds_the_brute_force_minimum():
    """beam = 16 holds every subset of up to two of five or six undirected edges and every single one of eight: where it holds all
    subsets below the brute-force size k (and C(n, k) <= 16 too), the search must return exactly k.  Elsewhere it cannot do
    better than k.  A graph whose decisive brute-force margin |p(ŷ) - p(runner-up)| is below LOGIT_TOL may be left out when it
    disagrees, at most 1 graph in 8; on the CPU the forwards of the search and of the brute force agree and none is."""
    m, b, gs, _ = _setup()
    cf = counterfactual(m, b, undirected="mean", beam=16, max_remove=8)
    left, exact = [], 0
    for g, d in enumerate(gs):
        k, margin, n = brute_min_flip(m, d, int(cf.yhat[g]))
        size = int(cf.size[g])
        print("graph %d: %d undirected edges, brute-force minimum %d (margin %.3g), search %d" % (g, n, k, margin, size))
        must = k > 0 and binom_ok(n, k, 16)
        ok = size == k if (must or k < 0) else (size == -1 or size >= k)
        exact += must
        if not ok:
            assert margin < LOGIT_TOL, (g, k, size, margin)
            left.append(g)
    assert exact >= 4 and len(left) <= len(gs) // 8
    assert not left                                                       # (the CPU run leaves out none)


@pytest.mark.parametrize("use,undirected", [("edges", None), ("edges", "mean"), ("nodes", None)])
def test_cpu_ranking_flip_is_a_loop_over_coalition_prefixes(use, undirected):
    m, b, _, twin = _setup()
    twin = twin if undirected else None
    M = int(b.edge_index.size(1)) if use == "edges" else int(b.batch.numel())
    score = torch.rand(M, generator=torch.Generator().manual_seed(4))
    if twin is not None:
        score = torch.where(twin >= 0, torch.minimum(score, score[twin.clamp(min=0).long()]), score)
    res = m.ranking_flip(b, score, use=use, undirected=undirected, max_remove=5, chunk=13)
    gid = b.batch[b.edge_index[0]] if use == "edges" else b.batch
    n = torch.zeros(8, dtype=torch.long).index_add_(0, gid, representatives(twin, M).long())
    lim = torch.clamp(n, max=5)
    if use == "nodes":
        lim = torch.minimum(lim, b.ptr[1:] - b.ptr[:-1] - 1)
    want = prefix_flip(m, b, rank_keys(score, b, use, twin), lim.tolist(), use)
    assert res["size"].tolist() == want and torch.equal(res["found"], res["size"] >= 0)
    assert res["replicas"] == int(lim.sum()) and res["forwards"] == 1 + -(-int(lim.sum()) // 13)
    # the default order is the causal attention as explain ranks it: one more forward
    att = ranking_flip(m, b, use=use, undirected=undirected, max_remove=5)
    from cal_amd.explain import explain
    ex = explain(m, b, ratio=0.5, undirected=undirected)
    again = ranking_flip(m, b, ex.edge_score if use == "edges" else ex.node_score, use=use, undirected=undirected, max_remove=5)
    assert torch.equal(att["size"], again["size"]) and att["forwards"] == again["forwards"] + 1


def test_cpu_eval_counterfactual_is_the_sum_over_its_batches():
    m, _, gs, _ = _setup()
    kw = dict(undirected="mean", beam=2, max_remove=3)
    res = eval_counterfactual(m, DataLoader(gs, batch_size=3, shuffle=False), "cpu", edge_gt="spmotif", seed=5, **kw)
    parts = []
    for i, lo in enumerate((0, 3, 6)):
        bb = Batch.from_data_list(gs[lo:lo + 3])
        parts.append(counterfactual_report(m, bb, edge_gt=spmotif.ground_truth(bb)[1], seed=5 + i, **kw))
    assert res["graphs"] == 8 and res["replicas"] == sum(p["replicas"] for p in parts)
    assert res["forwards"] == sum(p["forwards"] for p in parts)
    assert res["sums"] == [sum(p["sums"][j] for p in parts) for j in range(len(res["sums"]))]
    found = sum(p["sums"][1] for p in parts)
    assert found >= 2 and res["flip_rate"] == found / 8 and res["size_mean"] == sum(p["sums"][2] for p in parts) / found
    for k in ("attention_flip_rate", "random_flip_rate", "removed_in_motif", "inside_motif_rate"):
        assert k in res and (res[k] != res[k] or 0.0 <= res[k] <= 1.0)
    # the report's figures are those of the drivers it runs
    bb = Batch.from_data_list(gs[:3])
    cf, att = counterfactual(m, bb, **kw), ranking_flip(m, bb, undirected="mean", max_remove=3)
    assert parts[0]["sums"][1:5] == [float(cf.found.sum()), float(cf.size[cf.found].sum()), float(att["found"].sum()),
                                     float(att["size"][att["found"]].sum())]
    without = counterfactual_report(m, bb, seed=5, **kw)
    assert "removed_in_motif" not in without and without["sums"][:7] == parts[0]["sums"][:7]
