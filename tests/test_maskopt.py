"""Learned mask explanations on the CPU: the host twin of ``cal_mask_step`` against the fp64 formula of tests/maskopt_oracle.py on
the shared kernel cases, six seeded defects of that formula against the same cases and bounds, and ``learn_mask`` /
``MaskOptimizer`` / ``mask_agreement`` of CPU-resident models against the oracle's free-running loop, with the conditions under
which that comparison means something asserted on the oracle alone, the properties of the result (batch independence, twin
pairs, subsets, a falling loss), the state a call leaves behind and the argument errors.

Every comparison prints its figure before it asserts; the tolerances and how they were measured: tests/maskopt_oracle.py.
"""
import random
import subprocess

import pytest
import torch

import cal_amd
from cal_amd import _lib
from cal_amd.coalition import perturbation_curve
from cal_amd.explain import edge_twins
from cal_amd.gradient import masked_log_probs
from cal_amd.maskopt import LearnedMask, MaskOptimizer, learn_mask, mask_agreement
from cal_amd.plan import _c
from tests import maskopt_oracle as MO
from tests import softmask_oracle as SO


def test_abi_symbol_is_exported_by_both_libraries():
    """The prototype of INTEGRATION.md section 11: nine pointers, B / P / M / step, six floats and the stream."""
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        assert "cal_mask_step" in {l.split()[-1] for l in out.splitlines() if " T " in l}, path
    assert "cal_mask_step" in protos and "cal_mask_step" in _lib.HOST_SYMBOLS
    assert len(protos["cal_mask_step"][1]) == 20
    assert protos["cal_mask_step"][2][:9] == ["pptr", "rep", "mate", "grad", "theta", "exp_avg", "exp_avg_sq", "mask", "terms"]
    assert cal_amd.learn_mask is learn_mask and cal_amd.MaskOptimizer is MaskOptimizer


# ---- 1. the host twin against the formula ---------------------------------------------------------------------------------------
def _host_step(case, k=None):
    step, (l_size, l_ent) = case
    k = MO.kernel_inputs() if k is None else k
    th, m1, m2, mask = (k[n].clone() for n in ("theta", "exp_avg", "exp_avg_sq", "mask"))
    terms = torch.full((k["B"], 2), 7.0, dtype=torch.float64)
    a = MO.ADAM
    _c("cal_mask_step", k["pptr"], k["rep"], k["mate"], k["grad"] if step else None, th, m1, m2, mask, terms, k["B"], k["P"], k["M"],
       step, a["lr"], a["beta1"], a["beta2"], a["eps"], l_size, l_ent)
    return th, m1, m2, mask, terms


@pytest.mark.parametrize("case", MO.KERNEL_CASES, ids=lambda c: "step%d-size%g-ent%g" % (c[0], c[1][0], c[1][1]))
def test_host_step_matches_the_formula(case):
    k = MO.kernel_inputs()
    got = _host_step(case)
    err = MO.kernel_errors(got, MO.kernel_want(case))
    print("step %d coeffs %s: max |host - fp64| %s" % (case[0], case[1], " ".join("%s %.3g" % kv for kv in err.items())))
    assert MO.within(err), err
    th, m1, m2, mask, terms = got
    # elements of no player (the out-of-range player's and the out-of-range mate's included) keep their prior bits
    touched = torch.zeros(k["M"], dtype=torch.bool)
    for idx in (k["rep"].long(), k["mate"].long()):
        touched[idx[(idx >= 0) & (idx < k["M"])]] = True
    assert int((~touched).sum()) >= 211 and torch.equal(mask[~touched], k["mask"][~touched])
    assert bool((mask[touched] <= 1.0).all()) and terms[0].tolist() == [0.0, 0.0]
    # a pair's two elements carry the same bits
    pr = (k["mate"] >= 0) & (k["mate"] < k["M"]) & (k["rep"] < k["M"])
    assert int(pr.sum()) > 500 and torch.equal(mask[k["rep"][pr].long()], mask[k["mate"][pr].long()])
    for u, v in zip(got, _host_step(case)):
        assert torch.equal(u, v)                                          # a repeated call: the same bits
    if case[0] == 0:
        assert all(torch.equal(u, k[n]) for u, n in zip(got[:3], ("theta", "exp_avg", "exp_avg_sq")))
    elif case[1] == (0.0, 0.0):
        assert int(k["zero"].sum()) > 100 and torch.equal(th[k["zero"]], k["theta"][k["zero"]])      # grad 0, no regulariser
        assert not torch.equal(th[~k["zero"]], k["theta"][~k["zero"]])
    grid = k["theta"].abs() == 80.0
    assert int(grid.sum()) == 200 and bool(torch.isfinite(th[grid]).all())


def test_host_step_without_graphs_or_players():
    k = MO.kernel_inputs()
    for B, P in ((0, k["P"]), (k["B"], 0), (0, 0)):
        th, mask, terms = k["theta"].clone(), k["mask"].clone(), torch.full((5, 2), 7.0, dtype=torch.float64)
        _c("cal_mask_step", k["pptr"], k["rep"], k["mate"], k["grad"], th, k["exp_avg"].clone(), k["exp_avg_sq"].clone(), mask, terms,
           B, P, k["M"], 1, 0.01, 0.9, 0.999, 1e-8, 0.005, 1.0)
        assert torch.equal(th, k["theta"]) and torch.equal(mask, k["mask"]) and bool((terms == 7.0).all())
    # a malformed pptr is clamped into [0, P]: nothing outside the arrays is read
    bad = dict(k, pptr=torch.tensor([-5, 1, 64, 64, 2 * 10 ** 9, 10 ** 9]))
    got = _host_step((1, (0.005, 1.0)), bad)
    want = MO.step_formula(bad["pptr"], k["rep"], k["mate"], k["grad"], k["theta"], k["exp_avg"], k["exp_avg_sq"], k["mask"], k["M"], 1,
                           l_size=0.005, l_ent=1.0, **MO.ADAM)
    assert MO.within(MO.kernel_errors(got, want))


# ---- 2. the cases and bounds notice seeded defects ------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", MO.DEFECTS)
def test_seeded_defects_of_the_formula_exceed_the_bounds(defect):
    """The formula with the defect, held to the formula as the kernel is: some case of the table has to notice."""
    noticed = []
    for case in MO.KERNEL_CASES:
        err = MO.kernel_errors(MO.kernel_want(case, defect), MO.kernel_want(case))
        if not MO.within(err):
            noticed.append((case, {n: "%.3g" % v for n, v in err.items() if v > MO.KERNEL_ATOL[n]}))
    print(defect, "noticed by", len(noticed), "cases, e.g.", noticed[:1])
    assert noticed, defect


# ---- 3. the free-running optimiser against the oracle ---------------------------------------------------------------------------
_MODELS = {}


def _model(name, case=None):
    seed = MO.LEARN_SEED.get((name, case))
    if (name, seed) not in _MODELS:
        data = SO.model_batch()
        _MODELS[name, seed] = (SO.build_model(name, SO.model_state(name, data.feat.size(1), seed=seed), data.feat.size(1)), data)
    return _MODELS[name, seed]


def _case_kw(case, data):
    use, undirected, subset, head = case
    M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
    return dict(use=use, undirected=undirected, head=head, elements=SO.subset_of(M) if subset else None)


def _errors(res, want):
    """max |result - oracle| of theta, mask, p_masked and the loss history; the NaN pattern of the mask has to be the oracle's."""
    assert torch.equal(res.mask.cpu().isnan(), want["mask"].isnan())
    ok = ~want["mask"].isnan()
    d = lambda a, b: (a.cpu().double() - b).abs().max().item() if b.numel() else 0.0
    return dict(theta=d(res.theta, want["theta"]), mask=d(res.mask.cpu()[ok], want["mask"][ok]), p_masked=d(res.p_masked, want["p_masked"]),
                loss=d(res.loss, want["loss"]))


def test_the_comparison_with_the_oracle_is_not_vacuous():
    """On the oracle alone, for every model and case: (A) no ReLU of a differentiated forward within 1e-4 of its kink, (B) every
    player's |dL/dtheta| at every step at least 1000 x the model's ``SCORE_ATOL``."""
    for name in SO.MODELS:
        for case in MO.LEARN_CASES:
            w = MO.oracle_learn(name, case)
            print("%s %s: smallest ReLU |pre| %.3g, smallest |dL/dtheta| %.3g" % (name, case, w["min_pre"], w["min_grad"]))
            assert w["min_pre"] >= MO.RELU_MARGIN, (name, case, w["min_pre"])
            assert w["min_grad"] >= 1000 * SO.SCORE_ATOL[name], (name, case, w["min_grad"])


@pytest.mark.parametrize("case", MO.LEARN_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("name", SO.MODELS)
def test_learn_mask_matches_the_oracle(name, case):
    m, data = _model(name, case)
    want = MO.oracle_learn(name, case)
    res = m.learn_mask(data, steps=MO.LEARN_STEPS, lr=0.01, init=1.0, **_case_kw(case, data))
    assert isinstance(res, LearnedMask) and res.steps == MO.LEARN_STEPS and res.forwards == MO.LEARN_STEPS + 2
    assert res.mask.dtype == torch.float32 and res.loss.dtype == torch.float64 and res.loss.shape == (MO.LEARN_STEPS + 1, data.num_graphs, 3)
    assert torch.equal(res.yhat, want["yhat"]) and (res.p_full.double() - want["p_full"]).abs().max().item() < 1e-4
    err = _errors(res, want)
    print("%s %s: max |host path - oracle| %s" % (name, case, " ".join("%s %.3g" % kv for kv in err.items())))
    for key, v in err.items():
        assert v <= MO.MODEL_ATOL[name][key], (key, v)
    moved = (want["theta"] - 1.0).abs().min().item()
    assert moved >= 100 * MO.MODEL_ATOL[name]["theta"], moved              # every logit moved by far more than the tolerance


# ---- 4. properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SO.MODELS)
def test_a_graph_learns_the_same_mask_alone(name):
    m, data = _model(name)
    case = MO.LEARN_CASES[1]
    res = learn_mask(m, data, steps=MO.LEARN_STEPS, undirected="mean")
    gid = MO.oracle_learn(name, case)["gid"]
    for g in range(data.num_graphs):
        one, _, _ = MO.graph_of(data, g)
        alone = learn_mask(m, one, steps=MO.LEARN_STEPS, undirected="mean")
        err = (alone.theta - res.theta[gid == g]).abs().max().item()
        print("%s graph %d alone: max |theta - batch's| %.3g" % (name, g, err))
        assert alone.theta.numel() == int((gid == g).sum()) and err <= MO.MODEL_ATOL[name]["theta"]


@pytest.mark.parametrize("name", SO.MODELS)
def test_twin_pairs_and_subsets(name):
    m, data = _model(name)
    E = data.edge_index.size(1)
    twin = edge_twins(data)[0]
    t = twin.clamp(min=0).long()
    paired = (twin >= 0) & (t != torch.arange(E))
    res = learn_mask(m, data, steps=3, undirected="mean")
    assert torch.equal(res.twin, twin) and not bool(res.mask.isnan().any())
    assert int(paired.sum()) >= 20 and torch.equal(res.mask[paired], res.mask[t[paired]])
    # the input self-loop column: only the regularisers move it, from sigmoid(1) towards 1 (the entropy term wins at theta = 1)
    alone = learn_mask(m, data, steps=3)
    assert alone.twin is None and float(torch.sigmoid(torch.tensor(1.0))) < alone.mask[0].item() < 1.0
    # a subset: the others are NaN in the result and were at 1 in the forward
    el = SO.subset_of(E)
    part = learn_mask(m, data, steps=3, elements=el)
    assert torch.equal(part.mask.isnan(), ~el)
    full = torch.where(el, part.mask, torch.ones(E))
    lp = masked_log_probs(m, data, edge_mask=full)[1]
    p = lp.gather(-1, part.yhat.view(-1, 1)).view(-1).exp()
    assert torch.equal(p.detach(), part.p_masked)
    assert (part.loss[-1, :, 0] + part.p_masked.double().log()).abs().max().item() < 1e-6
    # the same call twice: identical bits; more steps on the same optimiser go on where it stood
    again = learn_mask(m, data, steps=3, undirected="mean")
    assert torch.equal(again.theta, res.theta) and torch.equal(again.loss, res.loss)
    opt = MaskOptimizer(m, data, undirected="mean")
    for _ in range(3):
        opt.step()
    assert torch.equal(opt.result().theta, res.theta) and opt.result().steps == 3


@pytest.mark.parametrize("name", SO.MODELS)
def test_the_loss_falls(name):
    m, data = _model(name)
    res = learn_mask(m, data, steps=8, lr=0.01)
    total = res.loss.sum((1, 2))
    print("%s: total loss %.4f -> %.4f over 8 steps" % (name, total[0].item(), total[-1].item()))
    assert total[-1].item() < total[0].item()


def test_a_call_leaves_the_model_as_it_was():
    m, data = _model("CausalGAT")
    m.train()
    for p in m.parameters():
        p.grad = None
    m.convs[0].weight.grad = torch.full_like(m.convs[0].weight, 3.0)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    req0 = [p.requires_grad for p in m.parameters()]
    py0, t0 = random.getstate(), torch.get_rng_state()
    calls0 = m.convs[0]._calls
    learn_mask(m, data, steps=2, use="nodes")
    mask_agreement(m, data, steps=2, undirected="mean", ratio=0.3)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and m.convs[0]._calls == calls0
    assert [p.requires_grad for p in m.parameters()] == req0
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    for n, p in m.named_parameters():
        assert p.grad is None or (n == "convs.0.weight" and bool((p.grad == 3.0).all())), n
    m.eval()


def test_agreement_and_curves_take_the_mask():
    m, _ = _model("CausalGCN")
    from tests.helpers import ref_batch
    b = ref_batch([0, 4, 7])
    res = m.learn_mask(b, steps=2, undirected="mean")
    cur = perturbation_curve(m, b, undirected="mean", ratios=(0.0, 0.5, 1.0), order=res.mask)
    assert bool(torch.isfinite(cur["auc_insertion"]).all()) and bool(torch.isfinite(cur["auc_deletion"]).all())
    out = mask_agreement(m, b, steps=2, undirected="mean", ratio=0.3)
    assert set(out) == {"rho", "tau", "jaccard", "rho_undefined", "tau_undefined", "jaccard_undefined", "graphs", "elements", "forwards"}
    assert out["graphs"] == b.num_graphs and out["forwards"] == res.forwards + 1
    twin = edge_twins(b)[0]
    assert out["elements"] == int((~((twin >= 0) & (twin < torch.arange(twin.numel())))).sum())
    # an init tensor: one entry per element, the player reads its first element's
    E = b.edge_index.size(1)
    init = torch.linspace(-1.0, 1.0, E)
    opt = MaskOptimizer(m, b, undirected="mean", init=init)
    assert torch.equal(opt.theta, init[opt.rep.long()]) and torch.allclose(opt.mask[opt.rep.long()], torch.sigmoid(opt.theta), atol=2e-7, rtol=0)


def test_argument_errors():
    m, data = _model("CausalGCN")
    E = data.edge_index.size(1)
    for kw, exc in ((dict(use="graphs"), ValueError), (dict(head="x"), ValueError), (dict(use="nodes", undirected="mean"), ValueError),
                    (dict(undirected="median"), ValueError), (dict(elements=torch.ones(E + 1, dtype=torch.bool)), ValueError),
                    (dict(elements=torch.ones(E)), TypeError), (dict(steps=0), ValueError), (dict(steps=2.5), TypeError),
                    (dict(steps=True), TypeError), (dict(lr=0.0), ValueError), (dict(lr=-1.0), ValueError), (dict(lr="a"), TypeError),
                    (dict(size_coeff=-0.1), ValueError), (dict(ent_coeff=-1.0), ValueError), (dict(init=torch.ones(E - 1)), ValueError),
                    (dict(init=torch.ones(E, dtype=torch.float64)), TypeError), (dict(init="one"), TypeError),
                    (dict(betas=(0.9, 1.0)), ValueError)):
        with pytest.raises(exc):
            learn_mask(m, data, **{"steps": 1, **kw})
    with pytest.raises(ValueError):
        mask_agreement(m, data, steps=1)                                   # neither ratio nor k
    with pytest.raises(ValueError):
        mask_agreement(m, data, steps=1, k="gt")
