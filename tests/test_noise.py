"""Structural-noise replicas on the CPU: the host twin of cal_noise_count / cal_noise_write against the plain restatement (every
integer output, the copied rows and the totals bit for bit), the exported symbols, the properties of the contract (nesting,
independence, the deleted share), the cross-checks against coalition_batch, cal_degree_onehot, the Python layer's argument errors
and reordering, and noise_curve() / stability() of a CPU-resident model recomputed from the model's own outputs."""
import argparse
import math
import random
import subprocess

import numpy as np
import pytest
import torch

from cal_amd import _lib, noise, spmotif
from cal_amd.coalition import coalition_batch
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import _log_probs, edge_twins, explain
from cal_amd.noise import degree_onehot, eval_noise_curve, eval_stability, noise_batch, noise_curve, stability
from oracle import cal_oracle as O
from tests import noise_oracle as NO
from tests.noise_oracle import (big_ring_case, check_noise, check_the_case_list_meets_duplicates, degree_oracle, many_tiny_case,
                                noise_cases, noise_oracle, replica_oracle, representatives, ring, twin_map, wide_lds_case)
from tests.occlude_oracle import agreement_counts_np, agreement_metrics_np, hand_batch

CASES = noise_cases()
SYMBOLS = ("cal_noise_ws", "cal_noise_count", "cal_noise_write", "cal_degree_onehot")


# ---- the builder --------------------------------------------------------------------------------------------------------------
def test_the_case_list_meets_duplicate_candidates():
    check_the_case_list_meets_duplicates(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_restatement(name):
    b, rg, add, dele, seed, und, tries = CASES[name]
    check_noise(noise_batch(b, rg, add=add, delete=dele, seed=seed, undirected=und, tries=tries), b, rg, add, dele, seed, und, tries)


@pytest.mark.parametrize("case", [big_ring_case, many_tiny_case, wide_lds_case])
def test_host_twin_sizes(case):
    b, rg, add, dele, seed, und, tries = case()
    r = check_noise(noise_batch(b, rg, add=add, delete=dele, seed=seed, undirected=und, tries=tries), b, rg, add, dele, seed, und, tries)
    assert r["totals"][5] > 1000


def test_abi_symbols_and_constants():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_noise_count"][1]) == 20 and len(protos["cal_noise_write"][1]) == 28
    assert len(protos["cal_noise_ws"][1]) == 4 and len(protos["cal_degree_onehot"][1]) == 6
    text = open(_lib.HEADER).read()
    assert "#define CAL_NOISE_C_DEL 0x%016XULL" % NO.C_DEL in text and "#define CAL_NOISE_C_ADD 0x%016XULL" % NO.C_ADD in text
    assert (noise.C_DEL, noise.C_ADD) == (NO.C_DEL, NO.C_ADD) and NO.C_DEL != NO.C_ADD
    assert NO.splitmix64(0) == 0xE220A8397B1DCDAF                          # the published first output of splitmix64 from state 0


def test_the_twin_restatement_is_cal_edge_twin():
    for name in ("hand_F3_und", "ring40_und"):
        b = CASES[name][0]
        assert edge_twins(b)[0].tolist() == twin_map(b)


def _sp(n=6, seed=3):
    return Batch.from_data_list(spmotif.train_mix(n, node_num=7, seed=seed))


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src"):
        assert torch.equal(getattr(u, key), getattr(v, key)), key
    assert (u.max_nodes, u.max_edges, u.empty_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs)


def test_no_noise_is_the_control_replica_and_delete_only_is_a_coalition():
    b = _sp()
    E = int(b.edge_index.size(1))
    rg = torch.tensor([0, 3, 3, 5, 1])
    for und in (True, False):
        res = noise_batch(b, rg, undirected=und)
        ctl = coalition_batch(b, rg, torch.zeros(5, dtype=torch.long), torch.zeros(E, dtype=torch.int32), rep_row=torch.full((5,), -1))
        _same(res, ctl)
        assert torch.equal(res.feat, ctl.feat) and torch.equal(res.y, ctl.y) and (res.n_added, res.short) == (0, 0)
        R = 12
        rg2 = torch.arange(R) % 6
        dele = torch.linspace(0.0, 1.0, R).double()
        res = noise_batch(b, rg2, delete=dele, seed=41, undirected=und)
        r = noise_oracle(b, rg2, 0.0, dele, 41, und)
        key = torch.zeros(R, E, dtype=torch.int32)
        key[torch.repeat_interleave(torch.arange(R), r["edge_ptr"][1:] - r["edge_ptr"][:-1]), r["edge_src"]] = 1
        want = coalition_batch(b, rg2, torch.ones(R, dtype=torch.long), key, rep_row=torch.arange(R), invert=True)
        _same(res, want)
        assert torch.equal(res.feat, want.feat) and torch.equal(res.y, want.y) and res.no_self_loops == want.no_self_loops
        assert int(res.edge_ptr[1]) == int(b.edge_ptr[1]) and int(res.edge_ptr[-1] - res.edge_ptr[-2]) == 0


def _cols(res, q):
    lo, hi = int(res.edge_ptr[q]), int(res.edge_ptr[q + 1])
    return (res.edge_index[:, lo:hi] - int(res.ptr[q])).t().tolist(), res.edge_src[lo:hi].tolist()


@pytest.mark.parametrize("und", [True, False])
def test_nesting_and_independence(und):
    b = _sp()
    B = b.num_graphs
    rg, seeds = torch.arange(B), torch.arange(B) * 13 + 5
    lo = noise_batch(b, rg, add=0.2, delete=0.2, seed=seeds, undirected=und)
    hi = noise_batch(b, rg, add=0.6, delete=0.5, seed=seeds, undirected=und)
    assert lo.short == 0 and hi.short == 0 and 0 < lo.n_added < hi.n_added
    for q in range(B):
        (cl, sl), (ch, sh) = _cols(lo, q), _cols(hi, q)
        new_lo, new_hi = [c for c, s in zip(cl, sl) if s < 0], [c for c, s in zip(ch, sh) if s < 0]
        assert new_hi[:len(new_lo)] == new_lo and len(new_hi) > len(new_lo)       # prefix nesting in add
        assert {s for s in sh if s >= 0} <= {s for s in sl if s >= 0}              # subset nesting in delete
        one = noise_batch(b, rg[q:q + 1], add=0.6, delete=0.5, seed=seeds[q:q + 1], undirected=und)      # alone
        assert _cols(one, 0) == (ch, sh) and int(one.added[0]) == int(hi.added[q])
    # an int seed s is the seeds s + r
    assert torch.equal(noise_batch(b, rg, add=0.3, delete=0.3, seed=9, undirected=und).edge_index,
                       noise_batch(b, rg, add=0.3, delete=0.3, seed=9 + torch.arange(B), undirected=und).edge_index)


def test_the_deleted_share_is_binomial():
    """Over 20 400 players at delete = 0.3 the deleted share lies within 5 binomial standard deviations of 0.3 (on the
    restatement; the operators are bit-equal to it)."""
    b = hand_batch([(40, ring(40))] * 30, F=0)
    r = noise_oracle(b, torch.arange(30).repeat(17), 0.0, 0.3, 1234)
    n, gone = sum(r["players"]), sum(r["deleted"])
    assert n == 20400 and abs(gone / n - 0.3) < 5 * math.sqrt(0.3 * 0.7 / n), (gone, n)
    res = noise_batch(b, torch.arange(30).repeat(17), delete=0.3, seed=1234)
    assert int(res.edge_index.size(1)) == 2 * (n - gone)


# ---- cal_degree_onehot --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 10])
def test_degree_onehot(F):
    ei = torch.tensor([[0, 0, 0, 0, 1, 2, 2, 3, 5, 5, 0, 9, -1], [1, 2, 3, 5, 0, 0, 2, 3, 0, 5, 1, 0, 2]])
    for N in (7, 0):
        assert torch.equal(degree_onehot(ei, N, F), degree_oracle(ei, N, F))
    none = degree_onehot(torch.zeros(2, 0, dtype=torch.long), 4, F)
    assert bool((none[:, 0] == 1).all()) and float(none.sum()) == 4.0
    with pytest.raises(ValueError):
        degree_onehot(ei, 7, 0)


def test_degree_features_reproduce_make_graph():
    b = _sp(16, 11)
    res = noise_batch(b, features="degree")
    assert torch.equal(res.feat, b.feat) and res.x is None
    noisy = noise_batch(b, add=0.4, seed=2, features="degree")
    assert torch.equal(noisy.feat, degree_oracle(noisy.edge_index, int(noisy.batch.numel()), 10))
    assert not torch.equal(noisy.feat, noise_batch(b, add=0.4, seed=2).feat)
    with pytest.raises(ValueError):
        noise_batch(CASES["hand_F0_und"][0], features="degree")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_argument_errors():
    b = _sp()
    nan, inf, six = float("nan"), float("inf"), torch.full((6,), 0.5)
    for bad in (nan, inf, -0.5):                           # a level that is not finite or negative, as a float and as an entry
        worse = six.clone()
        worse[4] = bad
        for kw in (dict(add=bad), dict(delete=bad), dict(add=worse), dict(delete=worse), dict(add=six, delete=worse.double())):
            with pytest.raises(ValueError):
                noise_batch(b, **kw)
    assert noise_batch(b, add=six, delete=six.double()).num_graphs == 6
    for kw in (dict(add=-0.1), dict(delete=-1.0), dict(tries=0), dict(tries=2.0), dict(features="both"), dict(seed=1.5),
               dict(add=torch.ones(3)), dict(seed=torch.arange(3)), dict(delete=torch.ones(6, dtype=torch.long))):
        with pytest.raises((ValueError, TypeError)):
            noise_batch(b, **kw)
    with pytest.raises(TypeError):
        noise_batch(b, torch.tensor([0.5]))
    m = _cpu_model("CausalGCN", 10)[0]
    for kw in (dict(head="x"), dict(trials=0), dict(chunk=0), dict(add=(0.1, 0.2), delete=(0.1, 0.2, 0.3)), dict(add=(-0.1,)),
               dict(add=(0.1, inf)), dict(delete=nan)):
        with pytest.raises(ValueError):
            noise_curve(m, b, **kw)
    for kw in (dict(), dict(ratio=0.3, k=2), dict(k="gt"), dict(ratio=0.3, undirected="sum"), dict(ratio=0.3, add=-1.0),
               dict(ratio=0.3, add=inf), dict(ratio=0.3, delete=nan)):
        with pytest.raises(ValueError):
            stability(m, b, **kw)


def test_ungrouped_and_foreign_inputs():
    b = _sp()
    E = b.edge_index.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.batch, f.num_graphs, f.y = None, b.feat, b.batch, b.num_graphs, b.y
    f.edge_index = b.edge_index[:, perm]
    order = torch.argsort(b.batch[b.edge_index[0, perm]], stable=True)
    g = Batch()
    g.__dict__.update(b.__dict__)
    g.edge_index = b.edge_index[:, perm][:, order]         # the same columns, grouped: what the operator sees
    rg = torch.tensor([5, 0, 2, 2])
    res = noise_batch(f, rg, add=0.5, delete=0.3, seed=8)
    r = noise_oracle(g, rg, 0.5, 0.3, 8)
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src"):
        assert torch.equal(getattr(res, k), r[k]), k
    es = r["edge_src"]
    assert torch.equal(res.edge_src, torch.where(es >= 0, order[es.clamp(min=0)], es)) and torch.equal(res.feat, r["x"])
    assert torch.equal(f.edge_index[:, res.edge_src[res.edge_src >= 0]], res.node_src[res.edge_index[:, res.edge_src >= 0]])


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


def test_cpu_noise_curve_from_the_models_own_outputs():
    m, _ = _cpu_model("CausalGCN", 10)
    b = _sp(4, 6)
    B, T = 4, 3
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    py0, t0 = random.getstate(), torch.get_rng_state()
    m.train()
    adds, dels = (0.0, 0.25, 0.5), (0.0, 0.0, 0.4)
    res = m.noise_curve(b, add=adds, delete=dels, trials=T, seed=4, chunk=5)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    assert all(torch.equal(v, sd0[k]) for k, v in m.state_dict().items())
    assert res["forwards"] == 1 + 3 * 3
    m.eval()
    with torch.no_grad():
        full = _log_probs(m, b)[1]
        assert torch.equal(res["yhat"], full.argmax(-1)) and torch.equal(res["p_full"], full.max(-1).values.exp())
        for lv, a, d in zip(res["levels"], adds, dels):
            rg, r = replica_oracle(b, T, a, d, 4, True)
            assert (lv["replicas"], lv["forwards"], lv["added"], lv["short"]) == (T * B, 3, r["totals"][5], r["totals"][6])
            lp = _log_probs(m, noise_batch(b, rg, add=a, delete=d, seed=4))[1]
            pred = lp.argmax(-1)
            assert torch.equal(lv["agree_graph"], (pred == res["yhat"][rg]).double().view(T, B).sum(0) / T)
            assert torch.equal(lv["acc_graph"], (pred == b.y.view(-1)[rg]).double().view(T, B).sum(0) / T)
            p = lp.gather(-1, res["yhat"][rg].view(-1, 1)).view(-1).exp().double()
            assert (lv["p_graph"] - p.view(T, B).mean(0)).abs().max().item() < 1e-6 and abs(lv["p"] - p.mean().item()) < 1e-6
            assert lv["agree"] == lv["agree_graph"].sum().item() / B and lv["acc"] == lv["acc_graph"].sum().item() / B
    assert res["levels"][0]["agree"] == 1.0 and (res["levels"][0]["p_graph"] - res["p_full"].double()).abs().max().item() < 1e-6
    assert res["levels"][1]["added"] < res["levels"][2]["added"]
    # no labels: no accuracy
    b2 = Batch()
    b2.__dict__.update(b.__dict__)
    b2.y = None
    lv = noise_curve(m, b2, add=(0.2,), trials=1)["levels"][0]
    assert "acc" not in lv and "acc_graph" not in lv and 0.0 <= lv["agree"] <= 1.0
    ev = eval_noise_curve(m, DataLoader(spmotif.train_mix(5, node_num=7, seed=6), batch_size=3, shuffle=False), "cpu", add=(0.0, 0.3), trials=2)
    assert ev["graphs"] == 5 and ev["levels"][0]["agree"] == 1.0 and ev["levels"][1]["replicas"] == 10 and ev["forwards"] == 2 + 4


@pytest.mark.parametrize("und", ["mean", None])
def test_cpu_stability_from_the_models_own_scores(und):
    m, _ = _cpu_model("CausalGCN", 10)
    b = _sp(4, 6)
    B, T = 4, 2
    gt = spmotif.ground_truth(b)[1]
    res = m.stability(b, add=0.3, delete=0.2, trials=T, seed=3, ratio=0.5, undirected=und, edge_gt=gt, chunk=3)
    r = noise_oracle(b, torch.arange(B).repeat(T), 0.3, 0.2, 3, und is not None)
    assert (res["replicas"], res["forwards"], res["added"], res["short"]) == (T * B, 2 + 3, r["totals"][5], r["totals"][6])
    clean = explain(m, b, ratio=0.5, undirected=und, edge_gt=gt)
    m.eval()
    with torch.no_grad():
        full = _log_probs(m, b)[1]
    yhat, p_full = full.argmax(-1), full.max(-1).values.exp()
    rg, seeds = torch.arange(B).repeat(T), 3 + torch.arange(T * B)
    met, tail, prec = [], np.zeros(5), []
    for i in range(0, T * B, 3):
        g = rg[i:i + 3]
        nb = noise_batch(b, g, add=0.3, delete=0.2, seed=seeds[i:i + 3], undirected=und is not None)
        surv = nb.edge_src >= 0
        ex = explain(m, nb, ratio=0.5, undirected=und, edge_gt=gt[nb.edge_src.clamp(min=0)] & surv)
        E2 = int(nb.edge_index.size(1))
        rep = representatives(ex.edge_twin, E2) if und is not None else torch.ones(E2, dtype=torch.bool)
        counts = agreement_counts_np(clean.edge_score[nb.edge_src.clamp(min=0)].numpy(), ex.edge_score.numpy(), nb.edge_ptr,
                                     nb.max_edges, (surv & rep).numpy(), ratio=0.5)
        met.append(agreement_metrics_np(counts))
        with torch.no_grad():
            lp = _log_probs(m, nb)[1]
        ins = ~surv & rep
        tail += [int((lp.argmax(-1) != yhat[g]).sum()), (p_full[g] - lp.gather(-1, yhat[g].view(-1, 1)).view(-1).exp()).double().sum().item(),
                 int((ins & ex.edge_mask).sum()), int(ins.sum()), int((surv & rep).sum())]
        prec.append(ex.metrics["edge"])
    met, n = np.concatenate(met), T * B
    for j, key in enumerate(("rho", "tau", "jaccard")):
        ok = ~np.isnan(met[:, j])
        assert res[key + "_undefined"] == int((~ok).sum()) and abs(res[key] - met[ok, j].mean()) < 1e-9, key
    assert res["flip"] == tail[0] / n and abs(res["dp"] - tail[1] / n) < 1e-6 and res["elements"] == int(tail[4])
    assert res["noise_in_top"] == tail[2] / tail[3] and tail[3] == r["totals"][5] and res["graphs"] == B
    for key, mt in (("precision_clean", clean.metrics["edge"]), ("precision_noisy", torch.cat(prec))):
        ok = mt[:, 0] > 0
        assert abs(res[key] - (mt[ok, 1] / mt[ok, 0]).mean().item()) < 1e-12
    # no noise: the clean ranking again
    zero = stability(m, b, add=0.0, delete=0.0, trials=2, ratio=0.5, undirected=und)
    assert zero["rho"] == 1.0 and zero["tau"] == 1.0 and zero["jaccard"] == 1.0 and zero["flip"] == 0.0 and zero["noise_in_top"] == 0.0
    assert abs(zero["dp"]) < 1e-6 and "precision_clean" not in zero
    es = eval_stability(m, DataLoader(spmotif.train_mix(5, node_num=7, seed=6), batch_size=3, shuffle=False), "cpu", add=0.2, trials=2,
                        k=4, undirected=und)
    assert es["graphs"] == 5 and es["replicas"] == 10 and 0.0 <= es["precision_noisy"] <= 1.0
