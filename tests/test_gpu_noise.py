"""Structural-noise replicas on the MI355X: the HIP builder (cal_noise_count / cal_noise_write) against the plain restatement and
the host twin bit for bit (the CPU case list, a ring above the LDS cap on the 256- and the 1024-thread workgroup, a scan beyond
one run per thread), against coalition_batch, the nesting and independence properties, cal_degree_onehot, the noisy batch on the
engine's per-graph route against the fp64 oracle, noise_curve() and stability() against the restatement fed the engine's own
argmaxes and scores, their exact values without noise on a deterministic engine, and the engine's state left untouched."""
import argparse
import random

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.coalition import coalition_batch
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import _Layout, _log_probs, _untiled, explain
from cal_amd.noise import degree_onehot, eval_noise_curve, eval_stability, noise_batch, noise_curve, stability
from oracle import cal_oracle as O
from tests.noise_oracle import (big_ring_case, check_noise, check_the_case_list_meets_duplicates, degree_oracle, many_tiny_case,
                                noise_cases, noise_oracle, replica_oracle, representatives, ring, twin_map, wide_lds_case)
from tests.occlude_oracle import agreement_counts_np, agreement_metrics_np, hand_batch
from tests.subgraph_oracle import oracle_log_probs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: the engine's logits against the oracle at these shapes
CASES = noise_cases()
SEEDS = {"CausalGCN": 2, "CausalGAT": 1, "CausalGIN": 1}                  # tests/test_gpu_occlude.py
SHAPES = [("CausalGCN", 128), ("CausalGAT", 64), ("CausalGIN", 64)]


def _dev(b):
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _to(v):
    return v.to(DEV) if torch.is_tensor(v) else v


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src"):
        assert torch.equal(getattr(u, key).cpu(), getattr(v, key).cpu()), key
    assert (u.max_nodes, u.max_edges, u.empty_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs)


def _feat(b):
    return b.feat if b.x is None else b.x


def _run(case):
    b, rg, add, dele, seed, und, tries = case
    res = noise_batch(_dev(b), _to(rg), add=_to(add), delete=_to(dele), seed=_to(seed), undirected=und, tries=tries)
    assert res.edge_index.is_cuda and res.ptr.is_cuda and res.added.is_cuda
    return res, check_noise(res, b, rg, add, dele, seed, und, tries)


# ---- 1. the builder, bit for bit ----------------------------------------------------------------------------------------------
def test_the_case_list_meets_duplicate_candidates():
    check_the_case_list_meets_duplicates(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_equals_restatement_and_host_twin(name):
    b, rg, add, dele, seed, und, tries = CASES[name]
    res, _ = _run(CASES[name])
    host = noise_batch(b, rg, add=add, delete=dele, seed=seed, undirected=und, tries=tries)
    _same(res, host)
    assert torch.equal(res.added.cpu(), host.added) and (res.n_added, res.short) == (host.n_added, host.short)


def test_hip_ring_above_the_lds_cap():
    """2200 columns: the adjacency test and the de-duplication walk the segment and the accepted pairs in global memory, next to
    3-node graphs that take the LDS path in the same launch."""
    res, r = _run(big_ring_case())
    assert r["added"].tolist()[1] == 1100 and r["added"].tolist()[3] == 275 and res.max_edges > 4000


def test_hip_wide_workgroups():
    """A batch whose average graph has more than 2048 columns: 1024-thread workgroups, chunks of 1024 candidates, for the large
    ring (the general path) and for the 6-ring beside it (the LDS path)."""
    b = hand_batch([(6, ring(6)), (2600, ring(2600))], F=4, seed=5)
    res, r = _run((b, torch.tensor([0, 1, 0, 1]), torch.tensor([2.0, 0.1, 0.5, 0.6]).double(), 0.1, 31, True, 8))
    assert r["added"].tolist()[1] == 260 and r["added"].tolist()[3] == 1560 and r["added"].tolist()[0] <= 9
    _run((b, torch.tensor([1, 0]), torch.tensor([0.3, 1.0]).double(), 0.0, 32, False, 8))


def test_hip_lds_path_beyond_one_chunk_of_wide_workgroups():
    """The 60-ring at a = 1080 in a batch that takes 1024-thread workgroups: its second chunk of candidates repeats pairs the first
    accepted, which only the set finds (the oracle asserts that on itself); the cases ring60_* do the same at 256 threads."""
    res, r = _run(wide_lds_case())
    assert r["walked"][0] > 1024 and r["cross"][0][1024] > 0 and r["added"].tolist() == [1080, 130, 1080]


def test_hip_scan_beyond_one_run_per_thread():
    res, r = _run(many_tiny_case())
    assert r["totals"][4] > 800 and r["totals"][6] > 100


# ---- 2. against coalition_batch -----------------------------------------------------------------------------------------------
def _sp():
    return Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=3))


def test_no_noise_is_the_control_replica():
    b = _sp()
    bd = _dev(b)
    rg = torch.tensor([0, 3, 3, 5, 1], device=DEV)
    E = int(b.edge_index.size(1))
    for und in (True, False):
        res = noise_batch(bd, rg, undirected=und)
        ctl = coalition_batch(bd, rg, torch.zeros(5, dtype=torch.long, device=DEV), torch.zeros(E, dtype=torch.int32, device=DEV),
                              rep_row=torch.full((5,), -1, device=DEV))
        _same(res, ctl)
        assert torch.equal(_feat(res), _feat(ctl)) and torch.equal(res.y, ctl.y) and (res.n_added, res.short) == (0, 0)


@pytest.mark.parametrize("und", [True, False])
def test_delete_only_is_a_coalition(und):
    """key[r, e] = 1 where column e stays in replica r (by the restatement), 0 where it goes; threshold 1, inverted."""
    b = _sp()
    bd = _dev(b)
    R, E = 12, int(b.edge_index.size(1))
    rg = torch.arange(R) % 6
    dele = torch.linspace(0.0, 1.0, R).double()
    res = noise_batch(bd, rg.to(DEV), delete=dele.to(DEV), seed=41, undirected=und)
    r = noise_oracle(b, rg, 0.0, dele, 41, und)
    key = torch.zeros(R, E, dtype=torch.int32)
    rid = torch.repeat_interleave(torch.arange(R), r["edge_ptr"][1:] - r["edge_ptr"][:-1])
    key[rid, r["edge_src"]] = 1
    want = coalition_batch(bd, rg.to(DEV), torch.ones(R, dtype=torch.long, device=DEV), key.to(DEV),
                           rep_row=torch.arange(R, device=DEV), invert=True)
    _same(res, want)
    assert torch.equal(_feat(res), _feat(want)) and torch.equal(res.y, want.y) and res.no_self_loops == want.no_self_loops
    assert res.num_graphs == want.num_graphs and int(res.edge_ptr[1]) == int(b.edge_ptr[1]) and int(res.edge_ptr[-1] - res.edge_ptr[-2]) == 0


# ---- 3. properties ------------------------------------------------------------------------------------------------------------
def _cols(res, q):
    lo, hi = int(res.edge_ptr[q]), int(res.edge_ptr[q + 1])
    n0 = int(res.ptr[q])
    return (res.edge_index[:, lo:hi] - n0).t().tolist(), res.edge_src[lo:hi].tolist()


@pytest.mark.parametrize("und", [True, False])
def test_nesting_and_independence(und):
    b = _sp()
    bd = _dev(b)
    B = b.num_graphs
    rg = torch.arange(B, device=DEV)
    seeds = torch.arange(B, device=DEV) * 13 + 5
    lo = noise_batch(bd, rg, add=0.2, delete=0.2, seed=seeds, undirected=und)
    hi = noise_batch(bd, rg, add=0.6, delete=0.5, seed=seeds, undirected=und)
    assert lo.short == 0 and hi.short == 0 and 0 < lo.n_added < hi.n_added
    for q in range(B):
        (cl, sl), (ch, sh) = _cols(lo, q), _cols(hi, q)
        new_lo, new_hi = [c for c, s in zip(cl, sl) if s < 0], [c for c, s in zip(ch, sh) if s < 0]
        assert new_hi[:len(new_lo)] == new_lo                                     # prefix nesting in add
        assert {s for s in sh if s >= 0} <= {s for s in sl if s >= 0}              # subset nesting in delete
        one = noise_batch(bd, rg[q:q + 1], add=0.6, delete=0.5, seed=seeds[q:q + 1], undirected=und)     # alone
        assert _cols(one, 0) == (ch, sh) and int(one.added[0]) == int(hi.added[q])


# ---- 4. cal_degree_onehot -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 10])
def test_degree_onehot(F):
    ei = torch.tensor([[0, 0, 0, 0, 1, 2, 2, 3, 5, 5, 0, 9, -1], [1, 2, 3, 5, 0, 0, 2, 3, 0, 5, 1, 0, 2]])     # self loops, a degree of 5,
    for N in (7, 0):                                                                                          # endpoints outside [0, N)
        got = degree_onehot(ei.to(DEV), N, F)
        assert torch.equal(got.cpu(), degree_oracle(ei, N, F)) and torch.equal(degree_onehot(ei, N, F), got.cpu())
    none = degree_onehot(torch.zeros(2, 0, dtype=torch.long, device=DEV), 4, F)
    assert torch.equal(none.cpu(), degree_oracle(torch.zeros(2, 0, dtype=torch.long), 4, F)) and bool((none[:, 0] == 1).all())


def test_degree_features_reproduce_make_graph():
    b = Batch.from_data_list(spmotif.train_mix(16, node_num=7, seed=11))
    bd = _dev(b)
    res = noise_batch(bd, features="degree")
    assert torch.equal(res.feat, bd.feat) and res.x is None
    noisy = noise_batch(bd, add=0.4, seed=2, features="degree")
    assert torch.equal(noisy.feat.cpu(), degree_oracle(noisy.edge_index.cpu(), int(noisy.batch.numel()), 10))
    assert not torch.equal(noisy.feat, noise_batch(bd, add=0.4, seed=2).feat)


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
    if not _SMALL:
        _SMALL["b"] = Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=11))
    return _SMALL["b"]


def _oracle_probs(name, sd, r, R, yhat_r, h=1):
    lp = oracle_log_probs(name, {k: v.double().cpu() for k, v in sd.items()}, r["x"], r["edge_index"], r["batch"], R, layers=3,
                          heads=4)
    return lp, lp[h].gather(-1, yhat_r.view(-1, 1)).view(-1).exp()


# ---- 5. the engine route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hidden", SHAPES)
def test_noisy_batch_takes_the_per_graph_route_and_matches_the_oracle(name, hidden):
    m, sd = _gpu_model(name, _args(hidden=hidden))
    b = _small()
    rg = torch.arange(6).repeat(4)
    rep = noise_batch(_dev(b), rg.to(DEV), add=0.3, delete=0.2, seed=5)
    assert rep.ptr.is_cuda and rep.edge_ptr.is_cuda and rep.max_nodes > 0 and rep.no_self_loops and rep.empty_graphs == 0
    assert rep.n_added > 0 and int((rep.edge_src >= 0).sum()) < 4 * int(b.edge_index.size(1))
    m.eval()
    with torch.no_grad():
        lp = _log_probs(m, rep)
    if name == "CausalGCN":
        names = _stage_names()
        assert "k_plan_graph" in names and "k_plan_count" not in names, names
    m.engine().check_status()
    r = noise_oracle(b, rg, 0.3, 0.2, 5)
    want, _ = _oracle_probs(name, sd, r, 24, torch.zeros(24, dtype=torch.long))
    err = (lp.cpu().double() - want).abs().max().item()
    print("%s: max |log p - oracle| = %.3g" % (name, err))
    assert err < LOGIT_TOL, err


# ---- 6. the drivers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hidden", SHAPES)
def test_noise_curve_counts_and_probabilities(name, hidden):
    """The counts (replicas, forwards, added, short) against the restatement; acc / agree from the engine's own argmaxes on the
    same replicas, bit for bit on a deterministic engine; p within 1.0001 LOGIT_TOL of the fp64 oracle's on the restated replicas
    (the engine's log-probabilities are held to LOGIT_TOL and p <= 1)."""
    m, sd = _gpu_model(name, _args(hidden=hidden), deterministic=True)
    b = _small()
    bd = _dev(b)
    B, T = b.num_graphs, 2
    adds, dels = (0.0, 0.2, 0.5), (0.0, 0.1, 0.3)
    res = noise_curve(m, bd, add=adds, delete=dels, trials=T, seed=3, chunk=5)
    m.engine().check_status()
    assert res["forwards"] == 1 + 3 * 3 and len(res["levels"]) == 3
    yhat = res["yhat"].cpu()
    m.eval()
    for lv, a, d in zip(res["levels"], adds, dels):
        rg, r = replica_oracle(b, T, a, d, 3, True)
        assert (lv["add"], lv["delete"]) == (a, d)
        assert (lv["replicas"], lv["forwards"], lv["added"], lv["short"]) == (T * B, 3, r["totals"][5], r["totals"][6])
        with torch.no_grad():
            lp = _log_probs(m, noise_batch(bd, rg.to(DEV), add=a, delete=d, seed=3))[1]
        pred = lp.argmax(-1).cpu()
        agree = (pred == yhat[rg]).double().view(T, B).sum(0) / T
        acc = (pred == b.y.view(-1)[rg]).double().view(T, B).sum(0) / T
        assert torch.equal(lv["agree_graph"].cpu(), agree) and torch.equal(lv["acc_graph"].cpu(), acc)
        assert lv["agree"] == agree.sum().item() / B and lv["acc"] == acc.sum().item() / B
        _, want = _oracle_probs(name, sd, r, T * B, yhat[rg])
        err = (lv["p_graph"].cpu() - want.view(T, B).mean(0)).abs().max().item()
        print("%s add=%.1f delete=%.1f: max |p - oracle| = %.3g" % (name, a, d, err))
        assert err < 1.0001 * LOGIT_TOL and abs(lv["p"] - want.mean().item()) < 1.0001 * LOGIT_TOL
    first = res["levels"][0]                                             # no noise: the clean batch again
    assert first["agree"] == 1.0 and first["added"] == 0 and torch.equal(first["p_graph"], res["p_full"].double())


def _stability_parts(m, bd, gt, T, add, dele, seed, ratio, und, chunk):
    """What a stability report is made of, from explain() on the clean batch and on the replicas noise_batch builds."""
    B = bd.num_graphs
    clean = explain(m, bd, ratio=ratio, undirected=und, edge_gt=gt)
    with torch.no_grad():
        full = _log_probs(m, _untiled(bd, _Layout(bd)))[1]
    yhat, p_full = full.argmax(-1), full.max(-1).values.exp()
    rg = torch.arange(B, device=DEV).repeat(T)
    seeds = seed + torch.arange(T * B, device=DEV)
    met, tail, prec = [], np.zeros(5), []
    for i in range(0, T * B, chunk):
        g = rg[i:i + chunk]
        nb = noise_batch(bd, g, add=add, delete=dele, seed=seeds[i:i + chunk], undirected=und is not None)
        surv = nb.edge_src >= 0
        ex = explain(m, nb, ratio=ratio, undirected=und, edge_gt=None if gt is None else gt[nb.edge_src.clamp(min=0)] & surv)
        E2 = int(nb.edge_index.size(1))
        rep = representatives(ex.edge_twin.cpu(), E2) if und is not None else torch.ones(E2, dtype=torch.bool)
        a = clean.edge_score[nb.edge_src.clamp(min=0)]
        counts = agreement_counts_np(a.cpu().numpy(), ex.edge_score.cpu().numpy(), nb.edge_ptr.cpu(), nb.max_edges,
                                     (surv.cpu() & rep).numpy(), ratio=ratio)
        met.append(agreement_metrics_np(counts))
        with torch.no_grad():
            lp = _log_probs(m, nb)[1]
        ins = ~surv.cpu() & rep
        tail += [int((lp.argmax(-1) != yhat[g]).sum()), (p_full[g] - lp.gather(-1, yhat[g].view(-1, 1)).view(-1).exp()).double().sum().item(),
                 int((ins & ex.edge_mask.cpu()).sum()), int(ins.sum()), int((surv.cpu() & rep).sum())]
        if gt is not None:
            prec.append(ex.metrics["edge"].cpu())
    return np.concatenate(met), tail, clean, (torch.cat(prec) if prec else None)


def _check_stability(res, met, tail, n):
    for j, key in enumerate(("rho", "tau", "jaccard")):
        ok = ~np.isnan(met[:, j])
        assert res[key + "_undefined"] == int((~ok).sum())
        assert abs(res[key] - met[ok, j].mean()) < 1e-12 if ok.any() else res[key] != res[key]
    assert res["flip"] == tail[0] / n and abs(res["dp"] - tail[1] / n) < 1e-12 and res["elements"] == int(tail[4])
    assert res["noise_in_top"] == (tail[2] / tail[3] if tail[3] else 0.0)


@pytest.mark.parametrize("und", ["mean", None])
def test_stability_from_the_engines_own_scores(und):
    m, sd = _gpu_model("CausalGCN", deterministic=True)
    b = _small()
    bd = _dev(b)
    B, T = b.num_graphs, 2
    gt = spmotif.ground_truth(bd)[1]
    res = stability(m, bd, add=0.3, delete=0.2, trials=T, seed=3, ratio=0.5, undirected=und, edge_gt=gt, chunk=5)
    m.engine().check_status()
    r = noise_oracle(b, torch.arange(B).repeat(T), 0.3, 0.2, 3, und is not None)
    assert (res["replicas"], res["forwards"], res["added"], res["short"]) == (T * B, 2 + 3, r["totals"][5], r["totals"][6])
    assert res["graphs"] == B and res["added"] > 0
    met, tail, clean, prec = _stability_parts(m, bd, gt, T, 0.3, 0.2, 3, 0.5, und, 5)
    _check_stability(res, met, tail, T * B)
    for key, mt in (("precision_clean", clean.metrics["edge"].cpu()), ("precision_noisy", prec)):
        ok = mt[:, 0] > 0
        assert abs(res[key] - (mt[ok, 1] / mt[ok, 0]).mean().item()) < 1e-12
    # the probabilities against the fp64 oracle on the restated replicas: dp is a difference of two, each within 1.0001 LOGIT_TOL
    rg = torch.arange(B).repeat(T)
    yhat = _log_probs(m, _untiled(bd, _Layout(bd)))[1].argmax(-1).cpu()
    src = dict(x=b.feat, edge_index=b.edge_index, batch=b.batch)
    _, p0 = _oracle_probs("CausalGCN", sd, src, B, yhat)
    _, p1 = _oracle_probs("CausalGCN", sd, r, T * B, yhat[rg])
    err = abs(res["dp"] - (p0[rg] - p1).mean().item())
    print("undirected=%s: |dp - oracle| = %.3g (dp %.3g)" % (und, err, res["dp"]))
    assert err < 2.1 * LOGIT_TOL


@pytest.mark.parametrize("name,hidden", SHAPES)
def test_no_noise_is_exact_on_a_deterministic_engine(name, hidden):
    m, _ = _gpu_model(name, _args(hidden=hidden), deterministic=True)
    bd = _dev(_small())
    for und in ("mean", None):
        res = stability(m, bd, add=0.0, delete=0.0, trials=2, ratio=0.5, undirected=und)
        assert res["rho"] == 1.0 and res["tau"] == 1.0 and res["jaccard"] == 1.0, res
        assert res["rho_undefined"] + res["tau_undefined"] + res["jaccard_undefined"] == 0
        assert res["flip"] == 0.0 and res["noise_in_top"] == 0.0 and res["dp"] == 0.0 and res["added"] == 0
    m.engine().check_status()


# ---- 7. state -----------------------------------------------------------------------------------------------------------------
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
    cur = m.noise_curve(b, add=(0.0, 0.3), delete=0.1, trials=2, features="degree")
    st = m.stability(b, add=0.2, delete=0.1, trials=2, ratio=0.3)
    assert len(cur["levels"]) == 2 and cur["levels"][1]["replicas"] == 8 and st["replicas"] == 8 and -1.0 <= st["rho"] <= 1.0
    loader = DataLoader(gs, batch_size=8, shuffle=False)
    ev = eval_noise_curve(m, loader, DEV, add=(0.0, 0.3), trials=2, seed=7)
    parts = [noise_curve(m, Batch.from_data_list(gs[i:i + 8]).to(DEV), add=(0.0, 0.3), trials=2, seed=7 + 2 * i) for i in (0, 8)]
    assert ev["graphs"] == 12 and ev["forwards"] == sum(p["forwards"] for p in parts)
    for lv, l0, l1 in zip(ev["levels"], parts[0]["levels"], parts[1]["levels"]):
        assert lv["added"] == l0["added"] + l1["added"] and lv["replicas"] == 24
        assert abs(lv["agree"] - (8 * l0["agree"] + 4 * l1["agree"]) / 12) < 1e-12
        assert abs(lv["acc"] - (8 * l0["acc"] + 4 * l1["acc"]) / 12) < 1e-12 and abs(lv["p"] - (8 * l0["p"] + 4 * l1["p"]) / 12) < 1e-12
    es = eval_stability(m, loader, DEV, add=0.2, trials=2, k=4)
    assert es["graphs"] == 12 and es["replicas"] == 24 and 0.0 <= es["precision_noisy"] <= 1.0 and 0.0 <= es["noise_in_top"] <= 1.0
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
