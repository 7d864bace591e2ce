"""Learned mask explanations on the MI355X: ``cal_mask_step`` (csrc/maskopt.hip) on the kernel cases of tests/maskopt_oracle.py --
canaries around every operand and output, every float operand once off 16-byte alignment, identical bits on a repeated call,
the fp64 formula within the bounds fixed on the CPU (``KERNEL_ATOL``) -- and ``learn_mask`` / ``MaskOptimizer`` /
``mask_agreement`` of GPU-resident models against the oracle's free-running loop with the tolerances fixed on the CPU
(``MODEL_ATOL``; tests/test_maskopt.py asserts on the oracle alone that the comparison means something), with the properties
of the result, an engine-backed model against a plain one, and the state a call leaves behind.
"""
import random

import pytest
import torch

from cal_amd import _lib
from cal_amd.coalition import perturbation_curve
from cal_amd.explain import edge_twins
from cal_amd.gradient import masked_log_probs
from cal_amd.maskopt import MaskOptimizer, learn_mask, mask_agreement
from cal_amd.plan import _stream
from tests import maskopt_oracle as MO
from tests import softmask_oracle as SO
from tests.helpers import Buf, pool_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
def _hip_step(pool, case, off, k=None, B=None, P=None):
    step, (l_size, l_ent) = case
    k = MO.kernel_inputs() if k is None else k
    pptr, rep, mate = Buf(pool, k["B"] + 1, torch.int64, data=k["pptr"]), Buf(pool, k["P"], torch.int32, data=k["rep"]), \
        Buf(pool, k["P"], torch.int32, data=k["mate"])
    grad = Buf(pool, k["M"], data=k["grad"], off=off)
    th, m1, m2 = (Buf(pool, k["P"], data=k[n], off=off) for n in ("theta", "exp_avg", "exp_avg_sq"))
    mask = Buf(pool, k["M"], data=k["mask"], off=off)
    terms = Buf(pool, 2 * k["B"], torch.float64, fill=7.0, off=off)
    a = MO.ADAM
    _lib.call("cal_mask_step", pptr.ptr(), rep.ptr(), mate.ptr(), grad.ptr() if step else None, th.ptr(), m1.ptr(), m2.ptr(), mask.ptr(),
              terms.ptr(), k["B"] if B is None else B, k["P"] if P is None else P, k["M"], step, a["lr"], a["beta1"], a["beta2"], a["eps"],
              l_size, l_ent, _stream())
    return th, m1, m2, mask, terms


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", MO.KERNEL_CASES, ids=lambda c: "step%d-size%g-ent%g" % (c[0], c[1][0], c[1][1]))
def test_hip_step_matches_the_formula(case, off):
    k = MO.kernel_inputs()
    pool = []
    runs = [_hip_step(pool, case, off) for _ in range(2)]
    torch.cuda.synchronize()
    assert pool_intact(pool)
    for u, v in zip(*runs):
        assert torch.equal(u.t, v.t)                                      # a repeated call: the same bits
    got = tuple(b.t.cpu() for b in runs[0])
    err = MO.kernel_errors(got, MO.kernel_want(case))
    print("step %d coeffs %s off %d: max |hip - fp64| %s" % (case[0], case[1], off, " ".join("%s %.3g" % kv for kv in err.items())))
    assert MO.within(err), err
    th, m1, m2, mask, terms = got
    touched = torch.zeros(k["M"], dtype=torch.bool)
    for idx in (k["rep"].long(), k["mate"].long()):
        touched[idx[(idx >= 0) & (idx < k["M"])]] = True
    assert torch.equal(mask[~touched], k["mask"][~touched])               # non-players keep their prior bits
    assert bool((mask[touched] <= 1.0).all()) and terms[:2].tolist() == [0.0, 0.0]
    pr = (k["mate"] >= 0) & (k["mate"] < k["M"]) & (k["rep"] < k["M"])
    assert torch.equal(mask[k["rep"][pr].long()], mask[k["mate"][pr].long()])
    if case[0] == 0:
        assert all(torch.equal(u, k[n]) for u, n in zip(got[:3], ("theta", "exp_avg", "exp_avg_sq")))
    elif case[1] == (0.0, 0.0):
        assert torch.equal(th[k["zero"]], k["theta"][k["zero"]])          # grad 0, no regulariser: theta bit for bit
    assert bool(torch.isfinite(th[k["theta"].abs() == 80.0]).all())


def test_hip_step_without_graphs_or_players():
    k = MO.kernel_inputs()
    pool = []
    before = _lib.lib().cal_launch_count()
    for B, P in ((0, k["P"]), (k["B"], 0), (0, 0)):
        th, m1, m2, mask, terms = _hip_step(pool, (1, (0.005, 1.0)), 0, B=B, P=P)
        torch.cuda.synchronize()
        assert torch.equal(th.t.cpu(), k["theta"]) and torch.equal(mask.t.cpu(), k["mask"]) and bool((terms.t == 7.0).all())
    assert _lib.lib().cal_launch_count() == before and pool_intact(pool)
    # a malformed pptr is clamped into [0, P]
    bad = dict(k, pptr=torch.tensor([-5, 1, 64, 64, 2 * 10 ** 9, 10 ** 9]))
    got = _hip_step(pool, (1, (0.005, 1.0)), 0, bad)
    torch.cuda.synchronize()
    want = MO.step_formula(bad["pptr"], k["rep"], k["mate"], k["grad"], k["theta"], k["exp_avg"], k["exp_avg_sq"], k["mask"], k["M"], 1,
                           l_size=0.005, l_ent=1.0, **MO.ADAM)
    assert pool_intact(pool) and MO.within(MO.kernel_errors(tuple(b.t.cpu() for b in got), want))


# ---- 2. the models ---------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, case=None):
    seed = MO.LEARN_SEED.get((name, case))
    if (name, seed) not in _MODELS:
        data = SO.model_batch()
        m = SO.build_model(name, SO.model_state(name, data.feat.size(1), seed=seed), data.feat.size(1)).to(DEV)
        _MODELS[name, seed] = (m, SO.to_device(data, DEV))
    return _MODELS[name, seed]


@pytest.mark.parametrize("case", MO.LEARN_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_learn_mask_matches_the_oracle(name, case):
    use, undirected, subset, head = case
    m, data = _model(name, case)
    M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
    want = MO.oracle_learn(name, case)
    res = m.learn_mask(data, steps=MO.LEARN_STEPS, lr=0.01, init=1.0, use=use, undirected=undirected, head=head,
                       elements=SO.subset_of(M).to(DEV) if subset else None)
    assert res.mask.is_cuda and res.loss.is_cuda and res.loss.shape == (MO.LEARN_STEPS + 1, data.num_graphs, 3)
    assert torch.equal(res.yhat.cpu(), want["yhat"]) and (res.p_full.cpu().double() - want["p_full"]).abs().max().item() < 1e-4
    assert torch.equal(res.mask.cpu().isnan(), want["mask"].isnan())
    ok = ~want["mask"].isnan()
    d = lambda a, b: (a.cpu().double() - b).abs().max().item()
    err = dict(theta=d(res.theta, want["theta"]), mask=d(res.mask.cpu()[ok], want["mask"][ok]), p_masked=d(res.p_masked, want["p_masked"]),
               loss=d(res.loss, want["loss"]))
    print("%s %s: max |gpu - oracle| %s (atol %s)" % (name, case, " ".join("%s %.3g" % kv for kv in err.items()),
                                                      " ".join("%.3g" % v for v in MO.MODEL_ATOL[name].values())))
    for key, v in err.items():
        assert v <= MO.MODEL_ATOL[name][key], (key, v)


@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_properties(name):
    m, data = _model(name)
    cpu = SO.model_batch()
    E = cpu.edge_index.size(1)
    res = learn_mask(m, data, steps=MO.LEARN_STEPS, undirected="mean")
    # a graph learned alone gives the batch's theta for its players
    gid = MO.oracle_learn(name, MO.LEARN_CASES[1])["gid"]
    for g in range(cpu.num_graphs):
        alone = learn_mask(m, SO.to_device(MO.graph_of(cpu, g)[0], DEV), steps=MO.LEARN_STEPS, undirected="mean")
        err = (alone.theta.cpu() - res.theta.cpu()[gid == g]).abs().max().item()
        print("%s graph %d alone: max |theta - batch's| %.3g" % (name, g, err))
        assert err <= MO.MODEL_ATOL[name]["theta"]
    # both columns of a twin pair carry the same bits
    twin = edge_twins(cpu)[0]
    t = twin.clamp(min=0).long()
    paired = (twin >= 0) & (t != torch.arange(E))
    mask = res.mask.cpu()
    assert torch.equal(res.twin.cpu(), twin) and torch.equal(mask[paired], mask[t[paired]]) and not bool(mask.isnan().any())
    # a subset: NaN outside, and those elements were at 1 in the forward
    el = SO.subset_of(E).to(DEV)
    part = learn_mask(m, data, steps=3, elements=el)
    assert torch.equal(part.mask.isnan(), ~el)
    lp = masked_log_probs(m, data, edge_mask=torch.where(el, part.mask, torch.ones(E, device=DEV)))[1]
    assert torch.equal(lp.gather(-1, part.yhat.view(-1, 1)).view(-1).exp().detach(), part.p_masked)
    # the same call twice: identical bits
    again = learn_mask(m, data, steps=MO.LEARN_STEPS, undirected="mean")
    assert torch.equal(again.theta, res.theta) and torch.equal(again.loss, res.loss) and torch.equal(again.mask, res.mask)
    # the loss falls
    total = learn_mask(m, data, steps=8, lr=0.01).loss.sum((1, 2))
    print("%s: total loss %.4f -> %.4f over 8 steps" % (name, total[0].item(), total[-1].item()))
    assert total[-1].item() < total[0].item()


@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_engine_backed_model_gives_the_plain_models_mask(name):
    m, data = _model(name)
    assert m.use_engine and m.engine() is not None
    with_engine = learn_mask(m, data, steps=3, undirected="mean")
    m.use_engine = False
    try:
        assert m.engine() is None
        plain = learn_mask(m, data, steps=3, undirected="mean")
    finally:
        del m.use_engine
    assert torch.equal(with_engine.theta, plain.theta) and torch.equal(with_engine.loss, plain.loss)
    assert torch.equal(with_engine.p_masked, plain.p_masked)


def test_gpu_call_leaves_the_model_as_it_was_and_feeds_the_downstream_tools():
    m, data = _model("CausalGAT")
    m.train()
    for p in m.parameters():
        p.grad = None
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    req0 = [p.requires_grad for p in m.parameters()]
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    eng = m.engine()
    assert eng is not None
    step0 = eng.step_count.clone()
    res = learn_mask(m, data, steps=2, use="nodes")
    out = mask_agreement(m, data, steps=2, undirected="mean", ratio=0.3)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    assert [p.requires_grad for p in m.parameters()] == req0 and all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    assert m.engine() is eng and torch.equal(eng.step_count, step0)
    m.eval()
    assert set(out) == {"rho", "tau", "jaccard", "rho_undefined", "tau_undefined", "jaccard_undefined", "graphs", "elements", "forwards"}
    assert out["graphs"] == data.num_graphs and out["forwards"] == 2 + 2 + 1 and res.forwards == 4
    from tests.helpers import ref_batch
    b = ref_batch([0, 4, 7]).to(DEV)
    g, _ = _model("CausalGCN")
    lm = g.learn_mask(b, steps=2, undirected="mean")
    cur = perturbation_curve(g, b, undirected="mean", ratios=(0.0, 0.5, 1.0), order=lm.mask)
    assert bool(torch.isfinite(cur["auc_insertion"]).all()) and bool(torch.isfinite(cur["auc_deletion"]).all())
    # argument errors on the device: an init or elements of the wrong size, a non-float init
    E = data.edge_index.size(1)
    with pytest.raises(ValueError):
        learn_mask(m, data, steps=1, init=torch.ones(E + 1, device=DEV))
    with pytest.raises(TypeError):
        learn_mask(m, data, steps=1, init=torch.ones(E, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        learn_mask(m, data, steps=0)
    with pytest.raises(ValueError):
        MaskOptimizer(m, data, lr=0.0)
