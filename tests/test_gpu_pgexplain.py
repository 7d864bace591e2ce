"""The parametric edge explainer on the MI355X: ``cal_edge_mlp_fwd`` / ``cal_edge_mlp_bwd`` (csrc/edgemlp.hip) on the kernel cases
of tests/pgexplain_oracle.py -- canaries around every operand and output, every float operand once off 16-byte alignment,
identical bits on a repeated call, the fp64 formulas within the bounds fixed on the CPU (``KERNEL_ATOL``) -- and
``ExplainerTrainer`` / ``explain_edges`` / ``eval_explainer`` of GPU-resident models against the oracle's free-running loop with
the tolerances fixed on the CPU (``MODEL_ATOL``; tests/test_pgexplain.py asserts on the oracle alone that the comparison means
something), with the properties of the result, an engine-backed model against a plain one, and the state a call leaves behind.
"""
import random

import pytest
import torch

from cal_amd import _lib
from cal_amd.explain import edge_twins
from cal_amd.pgexplain import EdgeExplainer, ExplainerTrainer, eval_explainer, explain_edges, explainer_agreement
from cal_amd.plan import _stream
from tests import maskopt_oracle as MO
from tests import pgexplain_oracle as PO
from tests import softmask_oracle as SO
from tests.helpers import Buf, pool_intact
from tests.test_pgexplain import _IDS, check_kernel_properties, train_and_explain, train_errors

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------
def _hip_kernels(pool, case, off, k=None, B=None, P=None):
    Hd, (tau, seed, step) = case
    k = PO.kernel_inputs(Hd) if k is None else k
    N, E, Pk, Bk = k["N"], k["E"], k["P"], k["B"]
    i32 = lambda name, n: Buf(pool, n, torch.int32, data=k[name])
    row, col, rep, mate = i32("row", E), i32("col", E), i32("rep", Pk), i32("mate", Pk)
    csr = [i32(n, N + 1 if n.startswith("rowptr") else E) for n in ("rowptr_src", "eid_src", "rowptr_dst", "eid_dst")]
    pptr = Buf(pool, Bk + 1, torch.int64, data=k["pptr"])
    pq, w2, b2 = (Buf(pool, k[n].numel(), data=k[n], off=off) for n in ("pq", "w2", "b2"))
    omega, z = Buf(pool, Pk, fill=7.0, off=off), Buf(pool, Pk, fill=7.0, off=off)
    mask = Buf(pool, E, data=k["mask"], off=off)
    terms = Buf(pool, 2 * Bk, torch.float64, fill=7.0, off=off)
    B, P = Bk if B is None else B, Pk if P is None else P
    _lib.call("cal_edge_mlp_fwd", pq.ptr(), w2.ptr(), b2.ptr(), row.ptr(), col.ptr(), pptr.ptr(), rep.ptr(), mate.ptr(), omega.ptr(),
              z.ptr(), mask.ptr(), terms.ptr(), N, E, Hd, B, P, tau, seed, step, _stream())
    zin, gmask = Buf(pool, Pk, data=PO.kernel_z(case), off=off), Buf(pool, E, data=k["gmask"], off=off)
    dpq, dw2, db2 = Buf(pool, N * 2 * Hd, fill=7.0, off=off), Buf(pool, Hd, fill=7.0, off=off), Buf(pool, 1, fill=7.0, off=off)
    ws = Buf(pool, _lib.query("cal_edge_mlp_bwd_ws", N, E, Hd), fill=7.0, off=off)
    _lib.call("cal_edge_mlp_bwd", pq.ptr(), w2.ptr(), row.ptr(), col.ptr(), csr[0].ptr(), csr[1].ptr(), csr[2].ptr(), csr[3].ptr(),
              pptr.ptr(), rep.ptr(), mate.ptr(), zin.ptr(), gmask.ptr(), dpq.ptr(), dw2.ptr(), db2.ptr(), ws.ptr(), N, E, Hd, B, P, tau,
              *PO.KERNEL_COEFFS, _stream())
    return omega, z, mask, terms, dpq, dw2, db2


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", PO.KERNEL_CASES, ids=_IDS)
def test_hip_kernels_match_the_formulas(case, off):
    k = PO.kernel_inputs(case[0])
    pool = []
    before = _lib.query("cal_launch_count")
    runs = [_hip_kernels(pool, case, off) for _ in range(2)]
    assert _lib.query("cal_launch_count") - before == 2 * (1 + 3)       # one launch forward, three backward
    torch.cuda.synchronize()
    assert pool_intact(pool)
    for u, v in zip(*runs):
        assert torch.equal(u.t, v.t)                                      # a repeated call: the same bits
    got = tuple(b.t.cpu() for b in runs[0])
    err = PO.kernel_errors(got, PO.kernel_want(case))
    print("%s off %d: max |hip - fp64| %s" % (_IDS(case), off, " ".join("%s %.3g" % kv for kv in err.items())))
    assert PO.within(err), err
    got = got[:3] + (got[3].view(-1, 2), got[4].view(k["N"], -1)) + got[5:]
    check_kernel_properties(k, got)


def test_hip_kernels_without_graphs_or_players_launch_nothing():
    case = (16, (2.0, 11, 0))
    k = PO.kernel_inputs(16)
    pool = []
    before = _lib.query("cal_launch_count")
    for B, P in ((0, k["P"]), (k["B"], 0), (0, 0)):
        got = _hip_kernels(pool, case, 0, B=B, P=P)
        torch.cuda.synchronize()
        assert torch.equal(got[2].t.cpu(), k["mask"]) and all(bool((b.t == 7.0).all()) for b in got[:2] + got[3:])
    assert _lib.query("cal_launch_count") == before and pool_intact(pool)
    # a malformed pptr is clamped into [0, P]
    bad = dict(k, pptr=torch.tensor([-5, 1, 64, 64, 2 * 10 ** 9, 10 ** 9]))
    got = _hip_kernels(pool, case, 0, bad)
    torch.cuda.synchronize()
    want = PO.forward_formula(bad, 2.0, 11, 0) + PO.backward_formula(bad, PO.kernel_z(case), k["gmask"], 2.0, *PO.KERNEL_COEFFS)
    assert pool_intact(pool) and PO.within(PO.kernel_errors(tuple(b.t.cpu() for b in got), want))


# ---- 2. the models ---------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        data = SO.model_batch()
        sd = SO.model_state(name, data.feat.size(1), seed=PO.TRAIN_SEED[name][0])
        _MODELS[name] = (SO.build_model(name, sd, data.feat.size(1)).to(DEV), SO.to_device(data, DEV))
    return _MODELS[name]


@pytest.mark.parametrize("case", PO.TRAIN_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_trainer_matches_the_oracle(name, case):
    m, data = _model(name)
    want = PO.oracle_train(name, case)
    tr, res = train_and_explain(m, data, name, case, DEV)
    assert res.mask.is_cuda and tr.history.is_cuda and tr.history.shape == (PO.TRAIN_STEPS, data.num_graphs, 3) and res.forwards == 2
    assert torch.equal(res.yhat.cpu(), want["yhat"]) and (res.p_full.cpu().double() - want["p_full"]).abs().max().item() < 1e-4
    err = train_errors(tr, res, want)
    print("%s %s: max |gpu - oracle| %s (atol %s)" % (name, case, " ".join("%s %.3g" % kv for kv in err.items()),
                                                      " ".join("%.3g" % v for v in PO.MODEL_ATOL[name].values())))
    for key, v in err.items():
        assert v <= PO.MODEL_ATOL[name][key], (key, v)


@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_properties(name):
    m, data = _model(name)
    cpu = SO.model_batch()
    E = cpu.edge_index.size(1)
    case = PO.TRAIN_CASES[1]
    tr, res = train_and_explain(m, data, name, case, DEV)
    # two fits with one seed: the same bits; another noise seed: other masks
    tr2, res2 = train_and_explain(m, data, name, case, DEV)
    assert torch.equal(res.mask, res2.mask) and torch.equal(tr.history, tr2.history)
    assert all(torch.equal(a, b) for a, b in zip(tr.explainer.parameters(), tr2.explainer.parameters()))
    ex3 = EdgeExplainer(32, PO.TRAIN_HD, seed=PO.TRAIN_SEED[name][1]).to(DEV)
    tr3 = ExplainerTrainer(m, ex3, total_steps=PO.TRAIN_STEPS, **dict(PO.TRAIN_KW, seed=2))
    for _ in range(PO.TRAIN_STEPS):
        tr3.step(data)
    assert not torch.equal(explain_edges(m, ex3, data).mask, res.mask)
    # NaN pattern, pair symmetry
    twin = edge_twins(cpu)[0]
    t = twin.clamp(min=0).long()
    paired = (twin >= 0) & (t != torch.arange(E))
    mask = res.mask.cpu()
    assert torch.equal(res.twin.cpu(), twin) and torch.equal(mask[paired], mask[t[paired]]) and not bool(mask.isnan().any())
    el = SO.subset_of(E).to(DEV)
    part = explain_edges(m, tr.explainer, data, undirected=None, elements=el)
    assert torch.equal(part.mask.isnan(), ~el) and part.forwards == 2
    # a graph alone gives the batch's mask for its columns (no noise at inference)
    for g in range(cpu.num_graphs):
        one, _, cols = MO.graph_of(cpu, g)
        alone = explain_edges(m, tr.explainer, SO.to_device(one, DEV))
        err = (alone.mask.cpu() - mask[cols]).abs().max().item()
        print("%s graph %d alone: max |mask - batch's| %.3g" % (name, g, err))
        assert err <= PO.MODEL_ATOL[name]["mask"]


@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_engine_backed_model_gives_the_plain_models_explainer(name):
    m, data = _model(name)
    assert m.use_engine and m.engine() is not None
    case = PO.TRAIN_CASES[1]
    tr, res = train_and_explain(m, data, name, case, DEV)
    m.use_engine = False
    try:
        assert m.engine() is None
        tr2, res2 = train_and_explain(m, data, name, case, DEV)
    finally:
        del m.use_engine
    assert torch.equal(res.mask, res2.mask) and torch.equal(tr.history, tr2.history) and torch.equal(res.p_masked, res2.p_masked)


def test_gpu_call_leaves_the_model_as_it_was_and_eval_counts_the_motif():
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
    ex = EdgeExplainer(32, 8, seed=2).to(DEV)
    tr = ExplainerTrainer(m, ex, total_steps=2)
    tr.step(data)
    tr.step(data)
    explain_edges(m, ex, data)
    out = explainer_agreement(m, ex, data, ratio=0.3)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    assert [p.requires_grad for p in m.parameters()] == req0 and all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    assert m.engine() is eng and torch.equal(eng.step_count, step0)
    m.eval()
    assert out["graphs"] == data.num_graphs and out["forwards"] == 3
    from cal_amd.data import Batch
    from cal_amd.spmotif import ground_truth
    from tests.helpers import ref_graphs
    gs = ref_graphs([0, 4, 7, 9])
    loader = [Batch.from_data_list(gs[:2]), Batch.from_data_list(gs[2:])]
    g, _ = _model("CausalGCN")
    gx = EdgeExplainer(32, 8, seed=1).to(DEV)
    res = eval_explainer(g, gx, loader, DEV, undirected=None)
    want = sum(int(ground_truth(b)[1].sum()) for b in loader)
    print(res)
    assert res["graphs"] == 4 and res["selected"] == want and want > 0
    assert all(0.0 <= res[k] <= 1.0 for k in ("precision", "recall", "auc"))
    ex2, hist = g.fit_explainer(loader, DEV, epochs=1, hidden=64)
    assert hist.shape == (2, 2, 3) and bool(torch.isfinite(hist).all()) and ex2.lin1.weight.is_cuda
