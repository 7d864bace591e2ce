"""The parametric edge explainer on the CPU: the oracle's integer draw, the backward formulas against torch autograd, the host
twins of ``cal_edge_mlp_fwd`` / ``cal_edge_mlp_bwd`` against the fp64 formulas of tests/pgexplain_oracle.py on the shared kernel
cases, six seeded defects of those formulas against the same cases and bounds, and ``ExplainerTrainer`` / ``explain_edges`` of
CPU-resident models against the oracle's free-running loop, with the conditions under which that comparison means something
asserted on the oracle alone, the state a call leaves behind, the ``state_dict`` round trip and the argument errors.

Every comparison prints its figure before it asserts; the tolerances and how they were measured: tests/pgexplain_oracle.py.
"""
import random
import subprocess

import pytest
import torch

import cal_amd
from cal_amd import _lib
from cal_amd.coalition import perturbation_curve
from cal_amd.pgexplain import (EdgeExplainer, EdgePlayers, ExplainerTrainer, ParametricMask, eval_explainer, explain_edges,
                               explainer_agreement, fit_explainer)
from cal_amd.plan import _c, _q
from tests import noise_oracle
from tests import pgexplain_oracle as PO
from tests import softmask_oracle as SO

_IDS = lambda c: "Hd%d-tau%g-seed%d-step%d" % ((c[0],) + c[1])


def test_abi_symbols_are_exported_by_both_libraries():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert {"cal_edge_mlp_fwd", "cal_edge_mlp_bwd_ws", "cal_edge_mlp_bwd"} <= exported, path
    for name in ("cal_edge_mlp_fwd", "cal_edge_mlp_bwd_ws", "cal_edge_mlp_bwd"):
        assert name in protos and name in _lib.HOST_SYMBOLS
    assert protos["cal_edge_mlp_fwd"][2][:12] == ["pq", "w2", "b2", "row32", "col32", "pptr", "rep", "mate", "omega", "z", "mask", "terms"]
    assert cal_amd.explain_edges is explain_edges and cal_amd.ExplainerTrainer is ExplainerTrainer


# ---- 1. the draw -----------------------------------------------------------------------------------------------------------------
def test_the_hash_is_the_projects_and_the_uniform_is_exact_and_open():
    for x in (0, 1, 12345, (1 << 64) - 1, 0x9E3779B97F4A7C15):
        assert PO.splitmix64(x) == noise_oracle.splitmix64(x)
    lo, hi = 1.0, 0.0
    for seed, step in ((1, 0), (11, 5), ((1 << 63) + 7, (1 << 31) - 1)):
        for p in list(range(2000)) + [(1 << 31) - 1]:
            d = PO.draw(seed, step, p)
            u = PO.uniform(seed, step, p)
            assert 0 <= d < (1 << 23) and 0.0 < u < 1.0
            u32 = torch.tensor(u, dtype=torch.float32)
            assert u32.double().item() == u and (1.0 - u32).double().item() == 1.0 - u      # u and 1 - u are fp32 numbers
            lo, hi = min(lo, u), max(hi, u)
    assert lo < 0.01 and hi > 0.99
    # the extremes of the 23-bit draw stay inside (0, 1) in fp32
    for d in (0, (1 << 23) - 1):
        u32 = (torch.tensor(float(d), dtype=torch.float32) + 0.5) * (1.0 / (1 << 23))
        assert 0.0 < u32.item() < 1.0 and (1.0 - u32).item() > 0.0
    assert PO.draw(11, 0, 3) != PO.draw(11, 5, 3) and PO.draw(11, 0, 3) != PO.draw(12, 0, 3)


# ---- 2. the formulas against autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(16, (2.0, 11, 0)), (100, (1.0, 0, 0)), (4, (5.0, 11, 5))], ids=_IDS)
def test_backward_formula_is_the_gradient_of_the_composed_loss(case):
    Hd, (tau, seed, step) = case
    k = PO.kernel_inputs(Hd)
    pq, w2, b2 = (k[n].double().clone().requires_grad_(True) for n in ("pq", "w2", "b2"))
    loss = PO.composed_loss(k, pq, w2, b2, k["gmask"], tau, seed, step, *PO.KERNEL_COEFFS)
    want = torch.autograd.grad(loss, (pq, w2, b2))
    z = PO.forward_formula(k, tau, seed, step)[1]
    got = PO.backward_formula(k, z, k["gmask"], tau, *PO.KERNEL_COEFFS)
    for name, a, b in zip(("dpq", "dw2", "db2"), got, want):
        err = (a - b).abs().max().item()
        print("%s: max |formula - autograd| %.3g (scale %.3g)" % (name, err, b.abs().max().item()))
        assert err <= 1e-12 * max(1.0, b.abs().max().item())


# ---- 3. the host twins against the formulas --------------------------------------------------------------------------------------
def host_kernels(case, k=None, B=None, P=None):
    """Both host twins on one kernel case -> the seven outputs of ``KERNEL_OUTPUTS``."""
    Hd, (tau, seed, step) = case
    k = PO.kernel_inputs(Hd) if k is None else k
    B, P = k["B"] if B is None else B, k["P"] if P is None else P
    omega, z = torch.full((k["P"],), 7.0), torch.full((k["P"],), 7.0)
    mask, terms = k["mask"].clone(), torch.full((k["B"], 2), 7.0, dtype=torch.float64)
    _c("cal_edge_mlp_fwd", k["pq"], k["w2"], k["b2"], k["row"], k["col"], k["pptr"], k["rep"], k["mate"], omega, z, mask, terms,
       k["N"], k["E"], Hd, B, P, tau, seed, step)
    dpq, dw2, db2 = torch.full((k["N"], 2 * Hd), 7.0), torch.full((Hd,), 7.0), torch.full((1,), 7.0)
    ws = torch.empty(_q(dpq, "cal_edge_mlp_bwd_ws", k["N"], k["E"], Hd))
    _c("cal_edge_mlp_bwd", k["pq"], k["w2"], k["row"], k["col"], k["rowptr_src"], k["eid_src"], k["rowptr_dst"], k["eid_dst"],
       k["pptr"], k["rep"], k["mate"], PO.kernel_z(case), k["gmask"], dpq, dw2, db2, ws, k["N"], k["E"], Hd, B, P, tau,
       *PO.KERNEL_COEFFS)
    return omega, z, mask, terms, dpq, dw2, db2


def check_kernel_properties(k, got):
    """What holds for any implementation's outputs on a kernel case beyond the bounds."""
    omega, z, mask, terms, dpq, dw2, db2 = got
    E, Hd = k["E"], k["Hd"]
    rep, mate = k["rep"].long(), k["mate"].long()
    touched = torch.zeros(E, dtype=torch.bool)
    r_ok = rep < E
    t_ok = r_ok & (mate >= 0) & (mate < E)
    touched[rep[r_ok]] = True
    touched[mate[t_ok]] = True
    assert int((~touched).sum()) >= 100 and torch.equal(mask[~touched], k["mask"][~touched])      # non-players keep their bits
    assert bool((mask[touched] <= 1.0).all()) and bool((mask[touched] >= 0.0).all())
    assert int(t_ok.sum()) > 300 and torch.equal(mask[rep[t_ok]], mask[mate[t_ok]])              # a pair: the same bits
    assert terms[4].tolist() == [0.0, 0.0]                                                      # the graph without players
    assert omega[3].item() == 0.0 and z[3].item() == 0.0                                        # the player with rep out of range
    deg = torch.bincount(k["row"].long(), minlength=k["N"]) + torch.bincount(k["col"].long(), minlength=k["N"])
    assert int((deg == 0).sum()) >= 20 and bool((dpq[deg == 0] == 0).all())                      # nodes without a column: rows of 0
    assert bool((dpq[170:] == 0).all())                                                         # graph 4: columns, no players


@pytest.mark.parametrize("case", PO.KERNEL_CASES, ids=_IDS)
def test_host_twins_match_the_formulas(case):
    k = PO.kernel_inputs(case[0])
    got = host_kernels(case)
    err = PO.kernel_errors(got, PO.kernel_want(case))
    print("%s: max |host - fp64| %s" % (_IDS(case), " ".join("%s %.3g" % kv for kv in err.items())))
    assert PO.within(err), err
    check_kernel_properties(k, got)
    for u, v in zip(got, host_kernels(case)):
        assert torch.equal(u, v)                                          # a repeated call: the same bits


def test_the_kernel_cases_hold_what_they_are_sized_for():
    for Hd in PO.KERNEL_HD:
        k = PO.kernel_inputs(Hd)
        row, col = k["row"].long(), k["col"].long()
        assert k["N"] == 200 and k["B"] == 5 and 900 <= k["E"] <= 1100
        assert int(torch.bincount(row, minlength=200)[0]) > 64 and int(torch.bincount(col, minlength=200)[0]) > 64
        assert int((row == col).sum()) == 1 and int((k["mate"] < 0).sum()) >= 8
        assert int(k["pptr"][5] - k["pptr"][4]) == 0 and int((row >= 170).sum()) > 100
        assert int(k["rep"][3]) >= k["E"] and int(k["mate"][9]) >= k["E"]
        h = PO._hidden(k)
        assert int((h == 0).sum()) >= 30                                  # hidden units exactly at the kink
        om, z = PO.forward_formula(k, 5.0, 0, 0)[:2]
        assert z.abs().max().item() >= 79.9 and z.min().item() < -79 and z.max().item() > 79
        # players of one graph do not sit in one run of columns: non-players and other graphs' columns lie between them
        member = torch.zeros(k["E"], dtype=torch.bool)
        member[k["rep"].long()[k["rep"] < k["E"]]] = True
        assert int((member[1:] != member[:-1]).sum()) > 100


def test_without_graphs_or_players_nothing_is_written():
    case = (16, (2.0, 11, 0))
    k = PO.kernel_inputs(16)
    for B, P in ((0, k["P"]), (k["B"], 0), (0, 0)):
        got = host_kernels(case, B=B, P=P)
        assert torch.equal(got[2], k["mask"]) and all(bool((t == 7.0).all()) for t in got[:2] + got[3:])
    # a malformed pptr is clamped into [0, P]
    bad = dict(k, pptr=torch.tensor([-5, 1, 64, 64, 2 * 10 ** 9, 10 ** 9]))
    got = host_kernels(case, bad)
    want = PO.forward_formula(bad, 2.0, 11, 0) + PO.backward_formula(bad, PO.kernel_z(case), k["gmask"], 2.0, *PO.KERNEL_COEFFS)
    assert PO.within(PO.kernel_errors(got, want))
    with pytest.raises(_lib.CalError):
        _c("cal_edge_mlp_fwd", k["pq"], k["w2"], k["b2"], k["row"], k["col"], k["pptr"], k["rep"], k["mate"], got[0], got[1], got[2],
           got[3], k["N"], k["E"], 18, k["B"], k["P"], 1.0, 0, 0)          # Hd not a multiple of 4


# ---- 4. the cases and bounds notice seeded defects -------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", PO.DEFECTS)
def test_seeded_defects_of_the_formulas_exceed_the_bounds(defect):
    """The formulas with the defect, held to the formulas as the kernels are: some case of the table has to notice."""
    noticed = []
    for case in PO.KERNEL_CASES:
        err = PO.kernel_errors(PO.kernel_want(case, defect), PO.kernel_want(case))
        if not PO.within(err):
            noticed.append((_IDS(case), {n: "%.3g" % v for n, v in err.items() if v > PO.KERNEL_ATOL[n]}))
    print(defect, "noticed by", len(noticed), "cases, e.g.", noticed[:1])
    assert noticed, defect


# ---- 5. the free-running trainer against the oracle ------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        data = SO.model_batch()
        sd = SO.model_state(name, data.feat.size(1), seed=PO.TRAIN_SEED[name][0])
        _MODELS[name] = (SO.build_model(name, sd, data.feat.size(1)), data)
    return _MODELS[name]


def train_and_explain(m, data, name, case, dev="cpu"):
    """The trainer at the oracle's settings, then ``explain_edges`` -> ``(trainer, ParametricMask)``."""
    undirected, subset, head = case
    E = data.edge_index.size(1)
    el = SO.subset_of(E).to(dev) if subset else None
    ex = EdgeExplainer(32, PO.TRAIN_HD, seed=PO.TRAIN_SEED[name][1]).to(dev)
    tr = ExplainerTrainer(m, ex, head=head, undirected=undirected, total_steps=PO.TRAIN_STEPS, **PO.TRAIN_KW)
    for _ in range(PO.TRAIN_STEPS):
        tr.step(data, elements=el)
    return tr, explain_edges(m, ex, data, undirected=undirected, elements=el, head=head)


def train_errors(tr, res, want):
    """max |result - oracle| of the parameters, omega, mask, p_masked and the loss history; NaN patterns have to be the oracle's."""
    assert torch.equal(res.mask.cpu().isnan(), want["mask"].isnan()) and torch.equal(res.omega.cpu().isnan(), want["omega"].isnan())
    ok = ~want["mask"].isnan()
    d = lambda a, b: (a.detach().cpu().double() - b).abs().max().item() if b.numel() else 0.0
    params = max(d(p, w) for p, w in zip(tr.explainer.parameters(), want["params"]))
    return dict(params=params, omega=d(res.omega.cpu()[ok], want["omega"][ok]), mask=d(res.mask.cpu()[ok], want["mask"][ok]),
                p_masked=d(res.p_masked, want["p_masked"]), loss=d(tr.history, want["history"]))


def test_the_comparison_with_the_oracle_is_not_vacuous():
    """On the oracle alone, for every model and case: (A) no ReLU (model or explainer) within 1e-4 of its kink, (B) every
    parameter gradient of every step exactly 0 or at least ``GRAD_MARGIN``; and the parameters move."""
    for name in SO.MODELS:
        init = list(PO.init_state(32, PO.TRAIN_HD, PO.TRAIN_SEED[name][1]).values())
        for case in PO.TRAIN_CASES:
            w = PO.oracle_train(name, case)
            print("%s %s: smallest ReLU |pre| %.3g, smallest non-zero |dL/dparam| %.3g" % (name, case, w["min_pre"], w["min_grad"]))
            assert w["min_pre"] >= PO.RELU_MARGIN, (name, case, w["min_pre"])
            assert w["min_grad"] >= PO.GRAD_MARGIN, (name, case, w["min_grad"])
            moved = max((a.double() - b).abs().max().item() for a, b in zip(init, w["params"]))
            assert moved >= 1000 * PO.MODEL_ATOL[name]["params"], moved


@pytest.mark.parametrize("case", PO.TRAIN_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("name", SO.MODELS)
def test_trainer_matches_the_oracle(name, case):
    m, data = _model(name)
    want = PO.oracle_train(name, case)
    tr, res = train_and_explain(m, data, name, case)
    assert isinstance(res, ParametricMask) and res.forwards == 2 and res.mask.dtype == torch.float32
    assert tr.history.dtype == torch.float64 and tr.history.shape == (PO.TRAIN_STEPS, data.num_graphs, 3)
    assert torch.equal(res.yhat, want["yhat"]) and (res.p_full.double() - want["p_full"]).abs().max().item() < 1e-4
    err = train_errors(tr, res, want)
    print("%s %s: max |host path - oracle| %s" % (name, case, " ".join("%s %.3g" % kv for kv in err.items())))
    for key, v in err.items():
        assert v <= PO.MODEL_ATOL[name][key], (key, v)


# ---- 6. properties ----------------------------------------------------------------------------------------------------------------
def test_explain_edges_properties_and_downstream_tools():
    m, data = _model("CausalGCN")
    E = data.edge_index.size(1)
    ex = EdgeExplainer(32, 8, seed=3)
    res = m.explain_edges(ex, data)
    from cal_amd.explain import edge_twins
    twin = edge_twins(data)[0]
    t = twin.clamp(min=0).long()
    paired = (twin >= 0) & (t != torch.arange(E))
    assert torch.equal(res.twin, twin) and not bool(res.mask.isnan().any())
    assert int(paired.sum()) >= 20 and torch.equal(res.mask[paired], res.mask[t[paired]])
    assert torch.allclose(res.mask, torch.sigmoid(res.omega), atol=2e-7, rtol=0)
    # a graph alone gives the batch's mask for its columns (no noise at inference)
    from tests import maskopt_oracle as MO
    for g in range(data.num_graphs):
        one, _, cols = MO.graph_of(data, g)
        alone = explain_edges(m, ex, one)
        err = (alone.mask - res.mask[cols]).abs().max().item()
        print("graph %d alone: max |mask - batch's| %.3g" % (g, err))
        assert err <= PO.MODEL_ATOL["CausalGCN"]["mask"]
    el = SO.subset_of(E)
    part = explain_edges(m, ex, data, undirected=None, elements=el)
    assert part.twin is None and torch.equal(part.mask.isnan(), ~el) and torch.equal(part.omega.isnan(), ~el)
    cur = perturbation_curve(m, data, undirected="mean", ratios=(0.0, 0.5, 1.0), order=res.mask)
    assert bool(torch.isfinite(cur["auc_insertion"]).all())
    out = explainer_agreement(m, ex, data, ratio=0.3)
    assert set(out) == {"rho", "tau", "jaccard", "rho_undefined", "tau_undefined", "jaccard_undefined", "graphs", "elements", "forwards"}
    assert out["graphs"] == data.num_graphs and out["forwards"] == 3


def test_a_call_leaves_the_model_as_it_was_and_attention_scores_keep_their_bits():
    m, data = _model("CausalGAT")
    m.eval()
    with torch.no_grad():
        x = data.feat
        plan = cal_amd.plan.plan_of(data)
        from cal_amd import ops
        h = m._backbone(m.conv_feat(m.bn_feat(x), data.edge_index, relu=True), data.edge_index, plan)
        edge0 = ops.edge_attention(h, m.edge_att_mlp.weight, m.edge_att_mlp.bias, plan)[1]
        node0 = ops.node_attention_split(h, m.node_att_mlp.weight, m.node_att_mlp.bias)[2][:, 1]
        edge1, node1 = m._attention_scores(data)
        assert torch.equal(edge0, edge1) and torch.equal(node0, node1) and torch.equal(m._node_embeddings(data), h)
    m.train()
    emb = m._node_embeddings(data)
    assert m.training and not emb.requires_grad and torch.equal(emb, h)
    for p in m.parameters():
        p.grad = None
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    req0 = [p.requires_grad for p in m.parameters()]
    py0, t0 = random.getstate(), torch.get_rng_state()
    ex = EdgeExplainer(32, 8, seed=2)
    tr = ExplainerTrainer(m, ex, total_steps=2)
    tr.step(data)
    tr.step(data)
    explain_edges(m, ex, data)
    from tests.helpers import ref_batch
    ex2, hist = m.fit_explainer([ref_batch([0, 4])], "cpu", epochs=2, hidden=8)
    assert hist.shape == (2, 2, 3) and bool(torch.isfinite(hist).all()) and isinstance(ex2, EdgeExplainer)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    assert [p.requires_grad for p in m.parameters()] == req0 and all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    m.eval()


def test_state_dict_round_trips_and_the_seed_decides_the_parameters():
    a, b, c = EdgeExplainer(32, 8, seed=4), EdgeExplainer(32, 8, seed=4), EdgeExplainer(32, 8, seed=5)
    assert set(a.state_dict()) == {"lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"}
    assert a.lin1.weight.shape == (8, 64) and a.lin2.weight.shape == (1, 8) and a.lin2.bias.shape == (1,)
    assert all(torch.equal(u, v) for u, v in zip(a.parameters(), b.parameters()))
    assert not torch.equal(a.lin1.weight, c.lin1.weight)
    for k, v in PO.init_state(32, 8, 4).items():
        assert torch.equal(a.state_dict()[k], v), k
    c.load_state_dict(a.state_dict())
    m, data = _model("CausalGCN")
    assert torch.equal(explain_edges(m, a, data).mask, explain_edges(m, c, data).mask)
    assert a.lin1.weight.abs().max().item() <= 1 / 8.0


def test_argument_errors():
    m, data = _model("CausalGCN")
    E = data.edge_index.size(1)
    ex = EdgeExplainer(32, 8)
    for kw, exc in ((dict(hidden=6), ValueError), (dict(hidden=260), ValueError), (dict(hidden=0), ValueError), (dict(hidden=8.0), TypeError),
                    (dict(hidden_in=0), ValueError), (dict(seed=-1), ValueError), (dict(seed=1.5), TypeError)):
        with pytest.raises(exc):
            EdgeExplainer(**{"hidden_in": 32, **kw})
    for kw, exc in ((dict(lr=0.0), ValueError), (dict(lr="a"), TypeError), (dict(size_coeff=-0.1), ValueError),
                    (dict(ent_coeff=float("inf")), ValueError), (dict(temp=(5.0,)), ValueError), (dict(temp=(5.0, 0.0)), ValueError),
                    (dict(temp=5.0), ValueError), (dict(head="x"), ValueError), (dict(undirected="median"), ValueError),
                    (dict(total_steps=0), ValueError), (dict(total_steps=2.5), TypeError), (dict(seed=True), TypeError),
                    (dict(hidden=10), ValueError)):
        with pytest.raises(exc):
            ExplainerTrainer(m, **kw)
    with pytest.raises(TypeError):
        ExplainerTrainer(m, torch.nn.Linear(64, 1))
    with pytest.raises(ValueError):
        ExplainerTrainer(m, EdgeExplainer(16, 8))                          # another embedding width
    for kw, exc in ((dict(elements=torch.ones(E + 1, dtype=torch.bool)), ValueError), (dict(elements=torch.ones(E)), TypeError),
                    (dict(head="x"), ValueError), (dict(undirected="median"), ValueError)):
        with pytest.raises(exc):
            explain_edges(m, ex, data, **kw)
    with pytest.raises(ValueError):
        explainer_agreement(m, ex, data)                                   # neither ratio nor k
    with pytest.raises(ValueError):
        ExplainerTrainer(m, ex).fit([data], "cpu", epochs=0)
    pl = EdgePlayers.of(data, "mean")
    assert EdgePlayers.of(data, "mean") is pl and EdgePlayers.of(data, None) is not pl and pl.loops


def test_eval_explainer_counts_the_motif():
    from cal_amd.data import Batch
    from cal_amd.spmotif import ground_truth
    from tests.helpers import ref_graphs
    gs = ref_graphs([0, 4, 7, 9])
    loader = [Batch.from_data_list(gs[:2]), Batch.from_data_list(gs[2:])]
    m, _ = _model("CausalGCN")
    ex = EdgeExplainer(32, 8, seed=1)
    out = eval_explainer(m, ex, loader, "cpu", undirected=None)
    want = sum(int(ground_truth(b)[1].sum()) for b in loader)
    print(out)
    assert out["graphs"] == 4 and out["selected"] == want and want > 0
    assert all(0.0 <= out[k] <= 1.0 for k in ("precision", "recall", "auc")) and out["precision"] == out["recall"]
    und = eval_explainer(m, ex, loader, "cpu")
    assert und["graphs"] == 4 and 0 < und["selected"] <= want and all(und[k] == und[k] for k in ("precision", "recall", "auc"))
