"""Coalition replicas, Shapley values and perturbation curves on the MI355X: the HIP replica builder (cal_coalition_count /
cal_coalition_write) against the plain-torch restatement and the host twin bit for bit (the CPU case list; the sizes beyond
it: tests/test_gpu_restrict.py), against occlude_batch and the
composition of splice_batches and extract_subgraph, the replica batch on the engine's per-graph route against the fp64 oracle,
shapley() and perturbation_curve() against the fp64 oracle, the exact properties of the estimate on a deterministic engine,
the curves against fidelity(), and the engine's state left untouched."""
import argparse
import random

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.coalition import (coalition_batch, eval_perturbation_curve, perturbation_curve, shapley, shapley_agreement)
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import _Layout, _log_probs, _untiled, edge_twins, explain, extract_subgraph, fidelity
from cal_amd.occlude import occlude_batch
from cal_amd.splice import splice_batches
from oracle import cal_oracle as O
from tests.coalition_oracle import (check_coalition, coalition_cases, coalition_oracle, curve_oracle, random_orders, rank_keys,
                                    representatives, shapley_oracle)
from tests.subgraph_oracle import oracle_log_probs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: the engine's logits against the oracle at these shapes
CASES = coalition_cases()
SEEDS = {"CausalGCN": 2, "CausalGAT": 1, "CausalGIN": 1}                  # tests/test_gpu_occlude.py
SHAPES = [("CausalGCN", 128), ("CausalGAT", 64), ("CausalGIN", 64)]


def _dev(b):
    """A device copy of a CPU batch (the case list is shared between tests)."""
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src"):
        assert torch.equal(getattr(u, key).cpu(), getattr(v, key).cpu()), key
    assert (u.max_nodes, u.max_edges, u.empty_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs)


def _feat(b):
    return b.feat if b.x is None else b.x


# ---- 1. the builder, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_equals_restatement_and_host_twin(name):
    b, rg, rrow, rth, key, use, invert = CASES[name]
    res = coalition_batch(_dev(b), rg.to(DEV), rth.to(DEV), key.to(DEV), rep_row=rrow.to(DEV), use=use, invert=invert)
    assert res.edge_index.is_cuda and res.ptr.is_cuda and res.node_src.is_cuda
    check_coalition(res, b, rg, rrow, rth, key, use, invert)
    _same(res, coalition_batch(b, rg, rth, key, rep_row=rrow, use=use, invert=invert))


def test_hip_ungrouped_columns():
    b, rg, rrow, rth, key, _, _ = CASES["spmotif_edges"]
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.batch, f.num_graphs, f.y = None, _feat(b).to(DEV), b.batch.to(DEV), b.num_graphs, b.y.to(DEV)
    f.edge_index = b.edge_index[:, perm].to(DEV)
    order = torch.argsort(b.batch[b.edge_index[0, perm]], stable=True)
    g = Batch()
    g.__dict__.update(b.__dict__)
    g.edge_index = b.edge_index[:, perm][:, order]         # the same columns, grouped: what the operator sees
    fkey = torch.randint(0, 9, (2, E), generator=torch.Generator().manual_seed(6), dtype=torch.int32)    # the caller's numbering
    res = coalition_batch(f, rg.to(DEV), rth.to(DEV), fkey.to(DEV), rep_row=rrow.to(DEV))
    r = coalition_oracle(g, rg, rrow, rth, fkey[:, order], "edges", False)
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src"):
        assert torch.equal(getattr(res, k).cpu(), r[k]), k
    assert torch.equal(res.feat.cpu(), r["x"]) and torch.equal(res.edge_src.cpu(), order[r["edge_src"]])


# ---- 3. the builder against the other builders ----------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_hip_reproduces_occlude_batch(use):
    """key[r] = 0 at the element replica r removes (and at its twin column), 1 elsewhere; threshold 1, inverted."""
    b = CASES["spmotif_edges"][0]
    bd = _dev(b)
    off = b.edge_ptr if use == "edges" else b.ptr
    M = int(off[-1])
    re = torch.arange(0, M, 3)[:80]
    rg = torch.searchsorted(off, re, right=True) - 1
    twin = edge_twins(b)[0] if use == "edges" else None
    R = int(re.numel())
    key = torch.ones(R, M, dtype=torch.int32)
    key[torch.arange(R), re] = 0
    if twin is not None:
        assert bool((twin[re] >= 0).all())
        key[torch.arange(R), twin[re].long()] = 0
    res = coalition_batch(bd, rg.to(DEV), torch.ones(R, dtype=torch.long, device=DEV), key.to(DEV),
                          rep_row=torch.arange(R, device=DEV), use=use, invert=True)
    want = occlude_batch(bd, rg.to(DEV), re.to(DEV), use=use, twin=None if twin is None else twin.to(DEV))
    _same(res, want)
    assert torch.equal(_feat(res), _feat(want)) and torch.equal(res.y, want.y) and res.no_self_loops == want.no_self_loops
    assert (res.x is None) == (want.x is None) and res.num_graphs == want.num_graphs


@pytest.mark.parametrize("name", ["spmotif_edges", "spmotif_nodes"])
def test_hip_equals_the_composition_of_splice_and_extract(name):
    b, rg, rrow, rth, key, use, _ = CASES[name]
    bd, rg, rrow, rth, key = _dev(b), rg.to(DEV), rrow.to(DEV), rth.to(DEV), key.to(DEV)
    rep = splice_batches(bd, bd, rg, torch.full_like(rg, -1))
    for invert in (False, True):
        res = coalition_batch(bd, rg, rth, key, rep_row=rrow, use=use, invert=invert)
        if use == "edges":
            rid = torch.repeat_interleave(torch.arange(rg.numel(), device=DEV), rep.edge_ptr[1:] - rep.edge_ptr[:-1])
            stay = key[rrow[rid], rep.edge_src].long() < rth[rid]
            comp = extract_subgraph(rep, edge_mask=stay != invert)
        else:
            stay = key[rrow[rep.batch], rep.node_src].long() < rth[rep.batch]
            comp = extract_subgraph(rep, node_mask=stay != invert, relabel=True)
        for k in ("edge_index", "ptr", "edge_ptr", "batch"):
            assert torch.equal(getattr(res, k), getattr(comp, k)), k
        assert torch.equal(_feat(res), _feat(comp))
        assert (res.max_nodes, res.max_edges) == (comp.max_nodes, comp.max_edges)


# ---- the models ---------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(layers=3, hidden=128, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _gpu_model(name, args=None, seed=None, deterministic=False):
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    args = args or _args()
    torch.manual_seed(SEEDS[name] if seed is None else seed)
    sd = O.init_state(name, 10, 4, hidden=args.hidden, layers=args.layers, heads=4, cat_or_add=args.cat_or_add)
    m = getattr(M, name)(10, 4, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")
    m = m.to(DEV)
    if deterministic:
        object.__setattr__(m, "_engine", StepEngine(m, deterministic=True))
    return m, sd


def _stage_names():
    h = _lib.lib()
    names, k = [], 1
    while True:
        nm = h.cal_engine_stage_name(k)
        nm = nm.decode() if isinstance(nm, bytes) else nm
        if not nm:
            return names
        names.append(nm)
        k += 1


_SMALL = {}


def _small():
    """The batch of six small SPMotif graphs the driver tests share (CPU), and its twin map."""
    if not _SMALL:
        b = Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=11))
        _SMALL["b"], _SMALL["twin"] = b, edge_twins(b)[0]
    return _SMALL["b"], _SMALL["twin"]


# ---- 4. the engine route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_replica_batch_takes_the_per_graph_route_and_matches_the_oracle(use):
    m, sd = _gpu_model("CausalGCN")
    b, _ = _small()
    off = b.edge_ptr if use == "edges" else b.ptr
    keys = random_orders(b, 2, use, None, seed=3)
    g = torch.Generator().manual_seed(9)
    rg = torch.randint(0, 6, (60,), generator=g)
    rrow = torch.randint(0, 2, (60,), generator=g)
    rth = 1 + torch.randint(0, 1 << 20, (60,), generator=g) % (off[rg + 1] - off[rg])      # at least one element stays
    rep = coalition_batch(_dev(b), rg.to(DEV), rth.to(DEV), keys.to(DEV), rep_row=rrow.to(DEV), use=use)
    assert rep.ptr.is_cuda and rep.edge_ptr.is_cuda and rep.max_nodes > 0 and rep.no_self_loops and rep.empty_graphs == 0
    m.eval()
    with torch.no_grad():
        lp = _log_probs(m, rep)
    names = _stage_names()
    assert "k_plan_graph" in names and "k_plan_count" not in names, names
    m.engine().check_status()
    r = coalition_oracle(b, rg, rrow, rth, keys, use, False)
    want = oracle_log_probs("CausalGCN", {k: v.double().cpu() for k, v in sd.items()}, r["x"], r["edge_index"], r["batch"], 60,
                            layers=3, heads=4)
    err = (lp.cpu().double() - want).abs().max().item()
    print("%s: max |log p - oracle| = %.3g" % (use, err))
    assert err < LOGIT_TOL, err


# ---- 5. Shapley against the fp64 oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use,undirected,subset", [("edges", None, False), ("edges", "mean", False), ("nodes", None, False),
                                                   ("edges", "max", True), ("nodes", None, True)])
@pytest.mark.parametrize("name,hidden", SHAPES)
def test_shapley_matches_the_oracle(name, hidden, use, undirected, subset):
    """The engine's log-probabilities are held to LOGIT_TOL of the oracle at these shapes; p <= 1, so each v is within 1.0001e-4
    of the oracle's.  A marginal is the difference of two and a mean of marginals keeps that bound: 2.1 LOGIT_TOL for every
    player.  The argmax is the engine's, handed to the oracle with the same orders; no player and no graph is left out."""
    m, sd = _gpu_model(name, _args(hidden=hidden))
    b, twin = _small()
    twin = twin if undirected else None
    off = b.edge_ptr if use == "edges" else b.ptr
    M = int(off[-1])
    el = (torch.rand(M, generator=torch.Generator().manual_seed(2)) < 0.5) if subset else None
    keys = random_orders(b, 3, use, twin, el, seed=7)
    sh = shapley(m, _dev(b), use=use, undirected=undirected, perms=keys.to(DEV), elements=None if el is None else el.to(DEV),
                 chunk=200)
    m.engine().check_status()
    want, p_full, p_empty, reps = shapley_oracle(name, sd, b, sh.yhat, keys, use, layers=3, heads=4)
    assert sh.replicas == reps and sh.forwards == 1 + -(-reps // 200) and torch.equal(sh.keys.cpu(), keys)
    assert (sh.twin is None) == (twin is None) and (twin is None or torch.equal(sh.twin.cpu(), twin))
    got = sh.score.cpu()
    assert got.dtype == torch.float64 and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.isnan(), keys[0] < 0)
    ok = ~want.isnan()
    err = (got - want)[ok].abs().max().item()
    perr = max((sh.p_full.cpu().double() - p_full).abs().max().item(), (sh.p_empty.cpu() - p_empty).abs().max().item())
    print("%s %s undirected=%s subset=%s: %d replicas, max |score - oracle| = %.3g, max |p - oracle| = %.3g (largest |score| %.3g)"
          % (name, use, undirected, subset, reps, err, perr, want[ok].abs().max().item()))
    assert err < 2.1 * LOGIT_TOL, err
    assert perr < 1.0001 * LOGIT_TOL, perr
    # the scores of a graph's players sum to p_full - p_empty: the telescoping sum of fp32 values taken in fp64
    rep = representatives(twin, M) & ok
    sums = torch.stack([got[lo:hi][rep[lo:hi]].sum() for lo, hi in zip(off[:-1].tolist(), off[1:].tolist())])
    n = torch.stack([rep[lo:hi].sum() for lo, hi in zip(off[:-1].tolist(), off[1:].tolist())])
    gap = (sums - (sh.p_full.cpu().double() - sh.p_empty.cpu())).abs()
    assert bool((gap <= (n + 1) * 2.0 ** -50).all()), gap
    if twin is not None:
        pair = twin >= 0
        assert torch.equal(got[pair].nan_to_num(7.0), got[twin[pair].long()].nan_to_num(7.0))


# ---- 6. exact properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hidden", SHAPES)
def test_exact_properties_on_a_deterministic_engine(name, hidden):
    m, _ = _gpu_model(name, _args(hidden=hidden), deterministic=True)
    b, twin = _small()
    bd = _dev(b)
    E = int(b.edge_index.size(1))
    m.eval()
    with torch.no_grad():
        full = _log_probs(m, _untiled(bd, _Layout(bd)))[1]
    p_full = full.max(-1).values.exp()
    # a control replica of every graph and the ratio = 1 insertion point reproduce p_full bit for bit
    B = b.num_graphs
    ctl = coalition_batch(bd, torch.arange(B, device=DEV), torch.zeros(B, dtype=torch.long, device=DEV),
                          torch.zeros(E, dtype=torch.int32, device=DEV), rep_row=torch.full((B,), -1, device=DEV))
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "y"):
        assert torch.equal(getattr(ctl, key), getattr(bd, key)), key
    assert torch.equal(_feat(ctl), _feat(bd)) and (ctl.max_nodes, ctl.max_edges) == (b.max_nodes, b.max_edges)
    with torch.no_grad():
        assert torch.equal(_log_probs(m, ctl)[1], full)
    cur = perturbation_curve(m, bd, ratios=(0.0, 0.5, 1.0))
    assert torch.equal(cur["p_full"], p_full) and torch.equal(cur["insertion"][:, 2], p_full)
    assert torch.equal(cur["deletion"][:, 0], p_full)
    # S identical orders, every order one chunk of its own: no spread, and the estimate of one order
    keys = random_orders(b, 1, "edges", twin, seed=5)
    per_order = int(representatives(twin, E).sum())
    one = shapley(m, bd, undirected="mean", perms=keys.to(DEV), chunk=per_order)
    same = shapley(m, bd, undirected="mean", perms=keys.repeat(3, 1).to(DEV), chunk=per_order)
    assert same.replicas == 3 * per_order and same.forwards == 4 and bool((same.stderr == 0).all())
    assert torch.equal(same.score, one.score) and bool(one.stderr.isnan().all()) and torch.equal(one.p_full, p_full)
    # a graph with one player: its score is p_full - p_empty exactly
    el = torch.zeros(E, dtype=torch.bool)
    el[b.edge_ptr[:-1]] = True                                            # the first column of every graph (and its twin)
    k1 = random_orders(b, 3, "edges", twin, el, seed=6)
    sh = shapley(m, bd, undirected="mean", perms=k1.to(DEV), elements=el.to(DEV), chunk=B)
    first = b.edge_ptr[:-1].to(DEV)
    assert sh.replicas == 3 * B and torch.equal(sh.score[first], sh.p_full.double() - sh.p_empty)
    assert int((~sh.score.isnan()).sum()) == 2 * B and bool((sh.stderr[first] == 0).all())
    # with a generator the global RNG states are unchanged, and equally seeded generators give equal bits
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    u = shapley(m, bd, use="nodes", perms=2, generator=torch.Generator().manual_seed(3))
    v = shapley(m, bd, use="nodes", perms=2, generator=torch.Generator().manual_seed(3))
    w = shapley(m, bd, use="nodes", perms=2)
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    assert torch.equal(u.keys, v.keys) and torch.equal(u.score, v.score) and torch.equal(u.stderr, v.stderr)
    assert not torch.equal(u.keys, w.keys) and bool((u.p_empty == 0.25).all())
    for lo, hi in zip(b.ptr[:-1].tolist(), b.ptr[1:].tolist()):
        assert sorted(u.keys[0, lo:hi].tolist()) == list(range(hi - lo))
    m.engine().check_status()


# ---- 7. curves ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use,undirected", [("edges", None), ("edges", "mean"), ("nodes", None)])
@pytest.mark.parametrize("name,hidden", SHAPES)
def test_perturbation_curve_matches_the_oracle_and_fidelity(name, hidden, use, undirected):
    """Every point is one p(ŷ): within 1.0001 LOGIT_TOL of the oracle's, so well within the 2.1 LOGIT_TOL of the Shapley test.
    The ranking handed to the oracle is the engine's own causal score, ranked in plain Python."""
    m, sd = _gpu_model(name, _args(hidden=hidden))
    b, twin = _small()
    bd = _dev(b)
    twin = twin if undirected else None
    ratios = (0.0, 0.1, 0.3, 0.5, 0.8, 1.0)
    res = perturbation_curve(m, bd, use=use, undirected=undirected, ratios=ratios, chunk=20)
    m.engine().check_status()
    ex = explain(m, bd, ratio=0.5, undirected=undirected)
    score = (ex.edge_score if use == "edges" else ex.node_score).cpu()
    ins, dele, p_full = curve_oracle(name, sd, b, res["yhat"], rank_keys(score, b, use, twin), ratios, use, layers=3, heads=4)
    B, T = b.num_graphs, len(ratios)
    skipped = 2 * B if use == "nodes" else 0
    assert res["replicas"] == 2 * T * B - skipped and res["forwards"] == 2 + 2 * -(-(T * B - skipped // 2) // 20)
    err = max((res["insertion"].cpu().double() - ins).abs().max().item(), (res["deletion"].cpu().double() - dele).abs().max().item(),
              (res["p_full"].cpu().double() - p_full).abs().max().item())
    print("%s %s undirected=%s: max |p - oracle| = %.3g" % (name, use, undirected, err))
    assert err < 2.1 * LOGIT_TOL, err
    if use == "nodes":
        assert bool((res["insertion"][:, 0] == 0.25).all()) and bool((res["deletion"][:, -1] == 0.25).all())
    x = torch.tensor(ratios, dtype=torch.float64, device=DEV)
    for key in ("insertion", "deletion"):
        y = res[key].double()
        want = sum((y[:, t + 1] + y[:, t]) / 2 * (x[t + 1] - x[t]) for t in range(T - 1))
        assert (res["auc_" + key] - want).abs().max().item() < 1e-15 and torch.equal(res[key + "_mean"], y.mean(0))
    if use == "edges":                                                    # both feed the engine the same graphs
        pf = res["p_full"].double().mean().item()
        for t, r in enumerate(ratios):
            fid = fidelity(m, bd, ratio=r, use="edges", undirected=undirected)
            assert abs(pf - res["insertion_mean"][t].item() - fid["fid_minus_o"]) < 2.1 * LOGIT_TOL
            assert abs(pf - res["deletion_mean"][t].item() - fid["fid_plus_o"]) < 2.1 * LOGIT_TOL


def test_eval_perturbation_curve_is_the_weighted_mean_of_the_batches():
    m, _ = _gpu_model("CausalGCN", deterministic=True)
    gs = spmotif.train_mix(7, node_num=7, seed=9)
    ratios = (0.0, 0.3, 1.0)
    res = eval_perturbation_curve(m, DataLoader(gs, batch_size=4, shuffle=False), DEV, undirected="mean", ratios=ratios)
    parts = [perturbation_curve(m, Batch.from_data_list(gs[i:i + 4]).to(DEV), undirected="mean", ratios=ratios) for i in (0, 4)]
    w = [4, 3]
    assert res["graphs"] == 7 and res["replicas"] == sum(p["replicas"] for p in parts) == 2 * 3 * 7
    assert res["forwards"] == sum(p["forwards"] for p in parts)
    for key in ("insertion_mean", "deletion_mean"):
        want = sum(p[key].cpu() * c for p, c in zip(parts, w)) / 7
        assert (torch.tensor(res[key], dtype=torch.float64) - want).abs().max().item() < 1e-12
    for key in ("auc_insertion_mean", "auc_deletion_mean"):
        assert abs(res[key] - sum(p[key].item() * c for p, c in zip(parts, w)) / 7) < 1e-12
    assert abs(res["p_full_mean"] - sum(p["p_full"].double().sum().item() for p in parts) / 7) < 1e-12


# ---- 8. state -----------------------------------------------------------------------------------------------------------------
def test_the_drivers_leave_the_engines_state_untouched():
    from cal_amd.engine import StepEngine
    args = _args(layers=2, hidden=64)
    m, _ = _gpu_model("CausalGCN", args, seed=0)
    m.train()
    eng = StepEngine(m, lr=1e-3, deterministic=True)
    object.__setattr__(m, "_engine", eng)
    gs = spmotif.train_mix(12, node_num=7, seed=9)
    tb = Batch.from_data_list(gs).to(DEV)
    perm = torch.randperm(12, device=DEV)
    for _ in range(2):
        eng.train_step(tb, perm, adam=True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    b = Batch.from_data_list(gs[:4]).to(DEV)
    for use, undirected in (("edges", "mean"), ("nodes", None)):
        sh = m.shapley(b, use=use, undirected=undirected, perms=2)
        cur = m.perturbation_curve(b, use=use, undirected=undirected, order=sh.score)
        ag = shapley_agreement(m, b, use=use, undirected=undirected, perms=sh.keys, ratio=0.3)
        assert ag["replicas"] == sh.replicas and ag["graphs"] == 4 and cur["insertion"].shape == (4, 11)
        assert ag["rho_undefined"] + ag["tau_undefined"] + ag["jaccard_undefined"] == 0 and -1.0 <= ag["rho"] <= 1.0
    eval_perturbation_curve(m, DataLoader(gs, batch_size=6, shuffle=False), DEV, ratios=(0.2, 0.6))
    eng.check_status()
    assert m.engine() is eng and m.training
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    eng.train_step(tb, perm, adam=True)                      # training goes on
    eng.check_status()
