"""Counterfactual explanations on the MI355X: the HIP subset builder (cal_subset_count / cal_subset_write) and the HIP beam step
(cal_beam_step) against the plain-int restatements and the host twins bit for bit on the whole case lists, ungrouped columns,
the replica batch on the engine's per-graph route against the fp64 oracle, the drivers' properties with GPU forwards (every found
set flips, beam=1 is the greedy loop, a wide beam finds the brute-force minimum), equal bits from two runs and the engine's state
left untouched."""
import argparse
import random

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.counterfactual import counterfactual, eval_counterfactual, ranking_flip, subset_batch
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import _log_probs, edge_twins, extract_subgraph
from oracle import cal_oracle as O
from tests.coalition_oracle import representatives
from tests.counterfactual_oracle import (balance_head, beam_cases, beam_oracle, binom_ok, brute_min_flip, check_subset, cut_graphs,
                                         greedy_occlude, run_beam, subset_cases, subset_oracle, subset_want)
from tests.subgraph_oracle import oracle_log_probs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: the engine's logits against the oracle at these shapes
CASES = subset_cases()
BEAMS = beam_cases()


def _dev(b):
    """A device copy of a CPU batch (the case list is shared between tests)."""
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _call(c, b=None, dev=DEV):
    t = lambda v: None if v is None else v.to(dev)
    return subset_batch(b if b is not None else (_dev(c["b"]) if dev == DEV else c["b"]), t(c["rg"]), t(c["bits"]),
                        rep_row=t(c["rrow"]), rep_flip=t(c["rflip"]), use=c["use"], twin=t(c["twin"]))


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src"):
        assert torch.equal(getattr(u, key).cpu(), getattr(v, key).cpu()), key
    assert (u.max_nodes, u.max_edges, u.empty_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs)


# ---- 1. the builder and the beam step, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_equals_restatement_and_host_twin(name):
    c = CASES[name]
    res = _call(c)
    assert res.edge_index.is_cuda and res.ptr.is_cuda and res.node_src.is_cuda
    check_subset(res, c, subset_want(name))
    _same(res, _call(c, dev="cpu"))
    if name.startswith("large"):
        assert res.max_nodes == 5000 and res.max_edges > 7000
    if name.startswith("scan"):
        assert res.num_graphs == 700 and res.empty_graphs > 200          # every thread of the scanning workgroup owns a run


@pytest.mark.parametrize("name", sorted(BEAMS))
def test_hip_beam_step_equals_restatement_and_host_twin(name):
    c = BEAMS[name]
    want, got, host = beam_oracle(c), run_beam(c, DEV), run_beam(c, "cpu")
    for k in want:
        assert got[k] == want[k], k
        assert got[k] == host[k], k


def test_hip_ungrouped_columns():
    c = CASES["spmotif_edges"]
    b = c["b"]
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.batch, f.num_graphs, f.y = None, (b.feat if b.x is None else b.x).to(DEV), b.batch.to(DEV), b.num_graphs, b.y.to(DEV)
    f.edge_index = b.edge_index[:, perm].to(DEV)
    order = torch.argsort(b.batch[b.edge_index[0, perm]], stable=True)
    g = Batch()
    g.__dict__.update(b.__dict__)
    g.edge_index = b.edge_index[:, perm][:, order]         # the same columns, grouped: what the operator sees
    res = _call(dict(c, twin=edge_twins(f)[0]), b=f)       # the twin map in the caller's numbering
    r = subset_oracle(dict(c, b=g, twin=edge_twins(g)[0]))
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src"):
        assert torch.equal(getattr(res, k).cpu(), r[k]), k
    assert torch.equal(res.feat.cpu(), r["x"]) and torch.equal(res.edge_src.cpu(), order[r["edge_src"]])


def test_two_runs_of_the_operators_give_equal_bits():
    c = CASES["scan_nodes"]
    u, v = _call(c), _call(c)
    _same(u, v)
    assert torch.equal(u.feat if u.x is None else u.x, v.feat if v.x is None else v.x)
    assert run_beam(BEAMS["two_words"], DEV) == run_beam(BEAMS["two_words"], DEV)


# ---- the models ---------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(layers=3, hidden=128, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _gpu_model(name="CausalGCN", args=None, seed=2, deterministic=False):
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    args = args or _args()
    torch.manual_seed(seed)
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


_SETUP = {}


def _setup(deterministic=False):
    """Eight SPMotif graphs cut to at most 8 (four of them: 5) undirected edges, on the device, and a model balanced on them."""
    if deterministic not in _SETUP:
        gs = cut_graphs(4, 8, 0) + cut_graphs(4, 5, 100)
        b = Batch.from_data_list(gs)
        m, _ = _gpu_model(deterministic=deterministic)
        _SETUP[deterministic] = (balance_head(m, _dev(b)), b, gs, edge_twins(b)[0])
    return _SETUP[deterministic]


# ---- 2. the engine route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_replica_batch_takes_the_per_graph_route_and_matches_the_oracle(use):
    m, sd = _gpu_model()
    b = CASES["spmotif_" + use]["b"]
    off = b.edge_ptr if use == "edges" else b.ptr
    g = torch.Generator().manual_seed(9)
    W = -(-int((off[1:] - off[:-1]).max()) // 32)
    bits = torch.randint(-2 ** 31, 2 ** 31, (5, W), generator=g, dtype=torch.long).to(torch.int32)
    bits[:, 0] |= 1                                                       # element 0 of every graph is present: no empty replica
    rg = torch.randint(0, 6, (60,), generator=g)
    rrow = torch.randint(0, 5, (60,), generator=g)
    rflip = 1 + torch.randint(0, 1 << 20, (60,), generator=g) % (off[rg + 1] - off[rg] - 1)      # never element 0
    c = dict(b=b, bits=bits, rg=rg, rrow=rrow, rflip=rflip, twin=None, use=use)
    rep = _call(c)
    assert rep.ptr.is_cuda and rep.edge_ptr.is_cuda and rep.max_nodes > 0 and rep.no_self_loops and rep.empty_graphs == 0
    m.eval()
    with torch.no_grad():
        lp = _log_probs(m, rep)
    names = _stage_names()
    assert "k_plan_graph" in names and "k_plan_count" not in names, names
    m.engine().check_status()
    r = subset_oracle(c)
    want = oracle_log_probs("CausalGCN", {k: v.double().cpu() for k, v in sd.items()}, r["x"], r["edge_index"], r["batch"], 60,
                            layers=3, heads=4)
    err = (lp.cpu().double() - want).abs().max().item()
    print("%s: max |log p - oracle| = %.3g" % (use, err))
    assert err < LOGIT_TOL, err


# ---- 3. the drivers' properties with GPU forwards -------------------------------------------------------------------------------
@pytest.mark.parametrize("use,undirected,beam", [("edges", "mean", 4), ("edges", None, 2), ("nodes", None, 4)])
def test_found_sets_flip_and_sizes_count_the_removed_players(use, undirected, beam):
    m, b, _, twin = _setup()
    bd = _dev(b)
    cf = m.counterfactual(bd, use=use, undirected=undirected, beam=beam, max_remove=4, chunk=97)
    m.engine().check_status()
    M = int(b.edge_index.size(1)) if use == "edges" else int(b.batch.numel())
    assert cf.removed.is_cuda and cf.removed.shape == (M,) and cf.size.shape == (8,)
    found, removed = cf.found.cpu(), cf.removed.cpu()
    print("%s undirected=%s beam=%d: sizes %s in %d rounds, %d replicas, %d forwards"
          % (use, undirected, beam, cf.size.tolist(), cf.rounds, cf.replicas, cf.forwards))
    assert int(found.sum()) >= 2 and torch.equal(found, cf.size.cpu() >= 0) and torch.equal(found, ~cf.p_cf.cpu().isnan())
    rep = representatives(twin if undirected else None, M)
    gid = b.batch[b.edge_index[0]] if use == "edges" else b.batch
    count = torch.zeros(8, dtype=torch.long).index_add_(0, gid, (removed & rep).long())
    assert torch.equal(torch.where(found, count, torch.full_like(count, -1)), cf.size.cpu())
    assert not bool(removed[~found[gid]].any()) and int(cf.size.max()) <= 4
    if undirected:
        pair = twin >= 0
        assert torch.equal(removed[pair], removed[twin[pair].long()])
    # every found set really flips: an independent forward of the extraction of ~removed.  The search's p(y^) of the set is
    # an engine forward of the same graph in another batch: both within LOGIT_TOL of the oracle's, as in test_gpu_coalition.py.
    sub = extract_subgraph(bd, edge_mask=~cf.removed) if use == "edges" else extract_subgraph(bd, node_mask=~cf.removed, relabel=True)
    m.eval()
    with torch.no_grad():
        lp = _log_probs(m, sub)[1]
    after = lp.argmax(-1)
    p_after = lp.gather(-1, cf.yhat.view(-1, 1)).view(-1).exp()
    margin = (lp.exp().topk(2, -1).values[:, 0] - lp.exp().topk(2, -1).values[:, 1])
    print("margins of the found sets", margin[cf.found].tolist())
    # a found set that this forward does not see flip must be too close to call (the search stops at the first flip, which sits
    # just beyond the decision boundary); at most 1 graph in 8
    left = cf.found & (after == cf.yhat)
    assert bool((margin[left] < LOGIT_TOL).all()) and int(left.sum()) <= 1
    assert torch.equal(after[cf.found & ~left], cf.y_cf[cf.found & ~left])
    assert float((p_after - cf.p_cf)[cf.found].abs().max()) < 2.1 * LOGIT_TOL


def test_beam_one_is_the_greedy_loop_over_occlude_batch():
    """A graph on which a round's best two p(ŷ) lie within LOGIT_TOL of each other may take another path through the greedy
    loop's own forwards; at most 1 graph in 8 may be left out for that."""
    m, b, _, twin = _setup()
    bd = _dev(b)
    cf = counterfactual(m, bd, undirected="mean", beam=1, max_remove=4)
    n = torch.zeros(8, dtype=torch.long).index_add_(0, b.batch[b.edge_index[0]], representatives(twin, twin.numel()).long())
    removed, size, gap = greedy_occlude(m, bd, twin.to(DEV), torch.clamp(n, max=4).tolist())
    print("sizes", size, "search", cf.size.tolist(), "gaps", ["%.2g" % v for v in gap])
    gid = b.batch[b.edge_index[0]]
    left = []
    for g in range(8):
        same = int(cf.size[g]) == size[g] and torch.equal(cf.removed.cpu()[gid == g], removed.cpu()[gid == g])
        if not same:
            assert gap[g] < LOGIT_TOL, (g, gap[g])
            left.append(g)
    assert len(left) <= 1 and int(cf.found.sum()) >= 2


def test_a_wide_beam_finds_the_brute_force_minimum():
    """As on the CPU (tests/test_counterfactual.py): where beam = 16 holds every subset below the brute-force size k the search
    returns exactly k, elsewhere nothing smaller.  A graph whose decisive brute-force margin is below LOGIT_TOL may be left
    out when it disagrees, at most 1 graph in 8."""
    m, b, gs, _ = _setup()
    cf = counterfactual(m, _dev(b), undirected="mean", beam=16, max_remove=8)
    left, exact = [], 0
    for g, d in enumerate(gs):
        k, margin, n = brute_min_flip(m, d, int(cf.yhat[g]), dev=DEV)
        size = int(cf.size[g])
        print("graph %d: %d undirected edges, brute-force minimum %d (margin %.3g), search %d" % (g, n, k, margin, size))
        must = k > 0 and binom_ok(n, k, 16)
        ok = size == k if (must or k < 0) else (size == -1 or size >= k)
        exact += must
        if not ok:
            assert margin < LOGIT_TOL, (g, k, size, margin)
            left.append(g)
    assert exact >= 3 and len(left) <= len(gs) // 8


# ---- 4. determinism and state ---------------------------------------------------------------------------------------------------
def test_two_runs_of_the_search_give_equal_bits():
    m, b, _, _ = _setup(deterministic=True)
    bd = _dev(b)
    u = counterfactual(m, bd, undirected="mean", beam=4, max_remove=4)
    v = counterfactual(m, bd, undirected="mean", beam=4, max_remove=4)
    for key in ("removed", "size", "found", "p_full", "yhat", "y_cf"):
        assert torch.equal(getattr(u, key), getattr(v, key)), key
    assert torch.equal(u.p_cf.view(torch.int32), v.p_cf.view(torch.int32))
    assert (u.rounds, u.replicas, u.forwards) == (v.rounds, v.replicas, v.forwards)
    r1, r2 = ranking_flip(m, bd, undirected="mean", max_remove=4), ranking_flip(m, bd, undirected="mean", max_remove=4)
    assert torch.equal(r1["size"], r2["size"])


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
        cf = m.counterfactual(b, use=use, undirected=undirected, beam=2, max_remove=2)
        rf = m.ranking_flip(b, use=use, undirected=undirected, max_remove=2)
        assert cf.size.shape == (4,) and rf["size"].shape == (4,) and cf.rounds <= 2
    res = eval_counterfactual(m, DataLoader(gs, batch_size=6, shuffle=False), DEV, undirected="mean", beam=2, max_remove=2,
                              edge_gt="spmotif")
    assert res["graphs"] == 12
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
