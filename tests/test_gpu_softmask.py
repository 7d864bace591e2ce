"""Soft edge masks and gradient attributions on the MI355X: ``cal_edge_dot`` and ``cal_gat_mask_fwd`` / ``_bwd`` (csrc/softmask.hip)
on the kernel cases of tests/test_softmask.py -- canaries around every operand and output, every float operand once off 16-byte
alignment, identical bits on a repeated call, the fp64 oracle and the host twin within the same tolerances -- and
``masked_log_probs`` / ``saliency`` / ``integrated_gradients`` of GPU-resident, engine-backed models against the fp64 oracle with
the tolerances fixed on the CPU (``softmask_oracle.SCORE_ATOL``), against the engine's own eval forward, against a
``coalition_batch`` replica run through the engine, and at the two shapes that take other kernel paths (a 4 x 64 GAT with a
200-column hub, a GIN at H 132: rows that are no multiple of 16 bytes).

The two wide cases (saliency over the edge columns): the fp32 host path against the fp64 oracle measured 2.14e-9 (CausalGAT, max
|score| 1.7e-3) and 5.25e-9 (CausalGIN, max |score| 3.4e-3); atol = 4 x that, rtol 1e-3.  Their seeds keep every ReLU of the one
differentiated forward 3e-5 away from its kink (asserted on the oracle); the hub's 200 columns come from ten neighbours, twenty
columns each, so that the graph stays small enough for such a seed to exist."""
import pytest
import torch

from cal_amd import _lib, ops
from cal_amd.coalition import coalition_batch
from cal_amd.data import Batch, Data
from cal_amd.explain import edge_twins
from cal_amd.gradient import integrated_gradients, masked_log_probs, saliency
from cal_amd.plan import GraphPlan, _stream
from tests import softmask_oracle as SO
from tests.helpers import Buf, pool_intact, ref_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_model.py: engine against operator path / oracle, on a logit


def _plan_bufs(pool, ei, n):
    """The plan of (ei, n) built on the GPU, its int32 arrays copied behind canaries."""
    plan = GraphPlan(ei.to(DEV), n, validate=True)
    nnz = int(plan.rowptr_dst[-1])
    arrs = {k: Buf(pool, getattr(plan, k).numel() if "rowptr" in k or "32" in k else nnz, torch.int32,
                   data=getattr(plan, k) if "rowptr" in k or "32" in k else getattr(plan, k)[:nnz])
            for k in ("rowptr_dst", "nbr_dst", "eid_dst", "rowptr_src", "nbr_src", "eid_src", "row32", "col32")}
    return plan, arrs


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [(0, 0, 0), (1, 0, 0), (0, 1, 1)], ids=["aligned", "a_off", "b_out_off"])
@pytest.mark.parametrize("H", SO.EDGE_DOT_H)
def test_hip_edge_dot(H, off):
    ei, n, facts, a, b, want = SO.edge_dot_case(H)
    pool = []
    plan, ar = _plan_bufs(pool, ei, n)
    E = plan.E
    A, Bm = Buf(pool, n * H, data=a, off=off[0]), Buf(pool, n * H, data=b, off=off[1])
    outs = [Buf(pool, E, fill=7.0, off=off[2]) for _ in range(2)]
    for o in outs:
        _lib.call("cal_edge_dot", ar["row32"].ptr(), ar["col32"].ptr(), A.ptr(), Bm.ptr(), o.ptr(), n, E, H, _stream())
    torch.cuda.synchronize()
    assert pool_intact(pool)
    got = outs[0].t.cpu()
    assert torch.equal(got, outs[1].t.cpu())                              # a repeated call: the same bits
    assert torch.allclose(got.double(), want, **SO.TOL_DW) and got[facts["loop"]].item() == 0.0
    host = torch.empty(E)
    cp = GraphPlan(ei, n)
    from cal_amd.plan import _c
    _c("cal_edge_dot", cp.row32, cp.col32, a, b, host, n, E, H)
    assert torch.allclose(got, host, **SO.TOL_DW)
    # E = 0 launches nothing and touches nothing
    before = _lib.lib().cal_launch_count()
    _lib.call("cal_edge_dot", None, None, A.ptr(), Bm.ptr(), outs[0].ptr(), n, 0, H, _stream())
    assert _lib.lib().cal_launch_count() == before and torch.equal(outs[0].t.cpu(), got)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("K,D", SO.GAT_SHAPES)
def test_hip_gat_mask(K, D, off):
    c = SO.gat_case(K, D)
    ei, n, facts = c["ei"], c["N"], c["facts"]
    H = K * D
    pool = []
    plan, ar = _plan_bufs(pool, ei, n)
    E = plan.E
    z, att, bias = Buf(pool, n * H, data=c["z"], off=off), Buf(pool, 2 * H, data=c["att"], off=off), Buf(pool, H, data=c["bias"], off=off)
    m, gout = Buf(pool, E, data=c["m"], off=off), Buf(pool, n * H, data=c["gout"], off=off)
    nws = _lib.query("cal_gat_mask_bwd_ws", n, E, K, D)
    assert nws >= (E + n) * K
    runs = []
    for _ in range(2):
        out, dz = Buf(pool, n * H, fill=7.0, off=off), Buf(pool, n * H, fill=7.0, off=off)
        adst, asrc, mx, den = (Buf(pool, n * K, fill=7.0, off=off) for _ in range(4))
        dm, ws, g = Buf(pool, E, fill=7.0, off=off), Buf(pool, nws, fill=7.0, off=off), Buf(pool, n * H, fill=7.0, off=off)
        _lib.call("cal_gat_mask_fwd", ar["rowptr_dst"].ptr(), ar["nbr_dst"].ptr(), ar["eid_dst"].ptr(), z.ptr(), att.ptr(), bias.ptr(),
                  1, 0.2, m.ptr(), out.ptr(), adst.ptr(), asrc.ptr(), mx.ptr(), den.ptr(), n, E, K, D, _stream())
        _lib.call("cal_relu_bwd_colsum", gout.ptr(), out.ptr(), g.ptr(), None, None, n, H, _stream())
        _lib.call("cal_gat_mask_bwd", ar["rowptr_dst"].ptr(), ar["nbr_dst"].ptr(), ar["eid_dst"].ptr(), ar["rowptr_src"].ptr(),
                  ar["nbr_src"].ptr(), ar["eid_src"].ptr(), z.ptr(), att.ptr(), adst.ptr(), asrc.ptr(), mx.ptr(), den.ptr(), g.ptr(), 0.2,
                  m.ptr(), dz.ptr(), dm.ptr(), ws.ptr(), n, E, K, D, _stream())
        runs.append((out, dz, dm, mx, den))
    torch.cuda.synchronize()
    assert pool_intact(pool)
    for u, v in zip(*runs):
        assert torch.equal(u.t, v.t)                                      # a repeated call: the same bits
    out, dz, dm = (t.t.cpu() for t in runs[0][:3])
    assert torch.allclose(out.view(n, H).double(), c["out"], **SO.TOL_OUT)
    assert torch.allclose(dz.view(n, H).double(), c["dz"], **SO.TOL_DZ)
    assert torch.allclose(dm.double(), c["dm"], **SO.TOL_DW) and dm[facts["loop"]].item() == 0.0
    # the host twin, through the operator on both sides
    zc, mc = c["z"].clone().requires_grad_(True), c["m"].clone().requires_grad_(True)
    ho = ops.gat_aggregate(zc, c["att"], c["bias"], GraphPlan(ei, n), K, relu=True, edge_mask=mc)
    ho.backward(c["gout"])
    zg, mg = c["z"].to(DEV).requires_grad_(True), c["m"].to(DEV).requires_grad_(True)
    go = ops.gat_aggregate(zg, c["att"].to(DEV), c["bias"].to(DEV), plan, K, relu=True, edge_mask=mg)
    go.backward(c["gout"].to(DEV))
    assert torch.allclose(go.detach().cpu(), ho.detach(), **SO.TOL_OUT) and torch.allclose(zg.grad.cpu(), zc.grad, **SO.TOL_DZ)
    assert torch.allclose(mg.grad.cpu(), mc.grad, **SO.TOL_DW)


def test_hip_gin_weighted_sum_and_node_mask_columns():
    ei, n, facts, a, b, _ = SO.edge_dot_case(132)
    plan, cp = GraphPlan(ei.to(DEV), n), GraphPlan(ei, n)
    g = torch.Generator().manual_seed(9)
    w = torch.rand(plan.E, generator=g)
    nm = torch.rand(n, generator=g)
    res = {}
    for dev, p in (("cpu", cp), (DEV, plan)):
        x, wd, nd = (t.clone().to(dev).requires_grad_(True) for t in (b, w, nm))
        out = ops.gin_aggregate(x, p, 0.25, edge_weight=wd * ops.node_mask_columns(nd, p))
        out.backward(a.to(dev))
        res[dev] = (out.detach().cpu(), x.grad.cpu(), wd.grad.cpu(), nd.grad.cpu())
    ro, rx, rw = SO.gin_weight_grad_oracle(b, ei, w * nm[ei[0]] * nm[ei[1]], a, 0.25)
    assert torch.allclose(res[DEV][0].double(), ro, **SO.TOL_OUT) and torch.allclose(res[DEV][1].double(), rx, **SO.TOL_DZ)
    for u, v, tol in zip(res[DEV], res["cpu"], (SO.TOL_OUT, SO.TOL_DZ, SO.TOL_DW, SO.TOL_DZ)):
        assert torch.allclose(u, v, **tol)
    assert res[DEV][2][facts["loop"]].item() == 0.0


# ---- 2. the models --------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        data = SO.model_batch()
        sd = SO.model_state(name, data.feat.size(1))
        _MODELS[name] = (SO.build_model(name, sd, data.feat.size(1)).to(DEV), SO.to_device(data, DEV))
    return _MODELS[name]


def _close(got, want, atol):
    got, want = got.cpu().double(), want.cpu().double()
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    err = (got - want)[ok].abs().max().item() if bool(ok.any()) else 0.0
    print("max |score - oracle| = %.3g (max |score| %.3g, atol %.3g)" % (err, want[ok].abs().max().item(), atol))
    return torch.allclose(got[ok], want[ok], atol=atol, rtol=SO.SCORE_RTOL)


@pytest.mark.parametrize("case", SO.SCORE_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_scores_match_the_oracle(name, case):
    use, undirected, subset, head = case
    m, data = _model(name)
    M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
    el = SO.subset_of(M).to(DEV) if subset else None
    for steps in (None, 4):
        want, _ = SO.oracle_scores(name, case, steps)
        if steps is None:
            got = m.saliency(data, use=use, undirected=undirected, head=head, elements=el)
        else:
            got = m.integrated_gradients(data, use=use, undirected=undirected, head=head, elements=el, steps=steps)
            assert (got.p_baseline.cpu().double() - want["p_baseline"]).abs().max().item() < LOGIT_TOL
            assert (got.gap.cpu() - want["gap"]).abs().max().item() < 4 * LOGIT_TOL
        assert got.score.is_cuda and got.score.dtype == torch.float64
        assert torch.equal(got.yhat.cpu(), want["yhat"]) and (got.p_full.cpu().double() - want["p_full"]).abs().max().item() < LOGIT_TOL
        assert _close(got.score, want["score"], SO.SCORE_ATOL[name])
        again = m.saliency(data, use=use, undirected=undirected, head=head, elements=el) if steps is None else \
            m.integrated_gradients(data, use=use, undirected=undirected, head=head, elements=el, steps=steps)
        assert torch.equal(again.score.nan_to_num(7.0), got.score.nan_to_num(7.0))       # the same call twice: identical bits


@pytest.mark.parametrize("name", SO.MODELS)
def test_gpu_masked_log_probs_and_engine_forward(name):
    m, data = _model(name)
    cpu = SO.model_batch()
    sd = {k: v.double() for k, v in SO.model_state(name, cpu.feat.size(1)).items()}
    E, N = cpu.edge_index.size(1), cpu.feat.size(0)
    g = torch.Generator().manual_seed(1)
    em, nm = torch.rand(E, generator=g), torch.rand(N, generator=g)
    em[::3], nm[::4] = 0.0, 0.0
    for kw in (dict(edge_mask=em), dict(node_mask=nm), dict(edge_mask=em, node_mask=nm)):
        got = masked_log_probs(m, data, **{k: v.to(DEV) for k, v in kw.items()})
        want = SO.masked_forward(name, sd, cpu.feat.double(), cpu.edge_index, cpu.batch, cpu.num_graphs,
                                 **{k: v.double() for k, v in kw.items()})
        assert max((a.cpu().double() - b).abs().max().item() for a, b in zip(got, want)) < LOGIT_TOL
    with pytest.raises(ValueError):
        masked_log_probs(m, data, edge_mask=em)                           # a mask on another device than the batch
    # p_full / yhat of saliency against the engine's own eval forward
    sal = saliency(m, data)
    was = m.training
    m.eval()
    with torch.no_grad():
        lp = m(data, eval_random=False)[1]
    m.train(was)
    assert torch.equal(sal.yhat, lp.argmax(-1))
    assert (sal.p_full.log() - lp.gather(-1, sal.yhat.view(-1, 1)).view(-1)).abs().max().item() < LOGIT_TOL


@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_gpu_binary_mask_is_a_coalition_replica_on_the_engine(use):
    b = ref_batch([0, 4, 7])
    feat = b.feat.size(1)
    m = SO.build_model("CausalGCN", SO.model_state("CausalGCN", feat), feat).to(DEV).eval()
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    M = b.edge_index.size(1) if use == "edges" else b.batch.numel()
    gid = (b.batch[b.edge_index[0]] if use == "edges" else b.batch).to(DEV)
    key = torch.randint(0, 10, (M,), generator=torch.Generator().manual_seed(6), dtype=torch.int32).to(DEV)
    rg, rth = torch.tensor([0, 1, 2, 1], device=DEV), torch.tensor([5, 3, 8, 10], device=DEV)
    reps = coalition_batch(d, rg, rth, key, use=use)
    assert reps.empty_graphs == 0 and m.engine() is not None
    with torch.no_grad():
        want = m(reps, eval_random=False)
    for r in range(rg.numel()):
        mask = torch.where((gid == rg[r]) & (key >= rth[r]), 0.0, 1.0)
        got = masked_log_probs(m, d, **{"edge_mask" if use == "edges" else "node_mask": mask})
        for h in range(3):
            assert (got[h][rg[r]].exp() - want[h][r].exp()).abs().max().item() < LOGIT_TOL, (r, h)


def _wide_case(name):
    """(model name) -> (cpu data, state, hidden, heads, atol): CausalGAT at K x D = 4 x 64 with a 200-column hub, CausalGIN at H 132."""
    g = torch.Generator().manual_seed(31)

    def small(n):
        a = torch.rand(n, n, generator=g) < 0.4
        a = a | a.t()
        a.fill_diagonal_(False)
        return Data(x=torch.randn(n, 10, generator=g), edge_index=a.nonzero().t().contiguous(), y=torch.zeros(1, dtype=torch.long))
    if name == "CausalGAT":
        src, dst = [], []
        for v in range(1, 11):                                            # node 0 receives 200 columns, 20 from each of ten
            src += [0, v] * 20; dst += [v, 0] * 20                        # neighbours, and sends as many back: few nodes, so
        star = Data(x=torch.randn(13, 10, generator=g),                   # that the ReLUs can be kept off their kinks
                    edge_index=torch.tensor([src + [11, 12], dst + [12, 11]]), y=torch.zeros(1, dtype=torch.long))
        return Batch.from_data_list([small(6), star, small(7)]), 256, 4, WIDE_ATOL[name], WIDE_SEED[name]
    return Batch.from_data_list([small(n) for n in (6, 9, 5, 8)]), 132, 4, WIDE_ATOL[name], WIDE_SEED[name]


#: 4 x the measured |fp32 host path - fp64 oracle| of the two wide cases (module docstring), and the seeds of their states
WIDE_ATOL = {"CausalGAT": 4 * 2.2e-9, "CausalGIN": 4 * 5.3e-9}
WIDE_SEED = {"CausalGAT": 1, "CausalGIN": 4}


@pytest.mark.parametrize("name", ["CausalGAT", "CausalGIN"])
def test_gpu_wide_shapes(name):
    b, hidden, heads, atol, seed = _wide_case(name)
    sd = SO.model_state(name, 10, hidden=hidden, heads=heads, seed=seed)
    m = SO.build_model(name, sd, 10, hidden=hidden, heads=heads).to(DEV)
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    if name == "CausalGAT":
        assert int(torch.bincount(b.edge_index[1]).max()) >= 200
    sd64 = {k: v.double() for k, v in sd.items()}
    track = SO.Track()
    E = b.edge_index.size(1)
    fwd = lambda mk: SO.masked_forward(name, sd64, b.x.double(), b.edge_index, b.batch, b.num_graphs, heads=heads, track=track, edge_mask=mk)
    want = SO.attribution(fwd, E, b.batch[b.edge_index[0]], b.num_graphs)
    assert track.min_pre >= 3e-5 and want["score"].abs().max().item() >= 100 * atol
    got = saliency(m, d)
    assert torch.equal(got.yhat.cpu(), want["yhat"]) and _close(got.score, want["score"], atol)
    em = torch.rand(E, generator=torch.Generator().manual_seed(2))
    em[::3] = 0.0
    lp = masked_log_probs(m, d, edge_mask=em.to(DEV))
    ref = SO.masked_forward(name, sd64, b.x.double(), b.edge_index, b.batch, b.num_graphs, heads=heads, edge_mask=em.double())
    assert max((u.cpu().double() - v).abs().max().item() for u, v in zip(lp, ref)) < LOGIT_TOL
    ig = integrated_gradients(m, d, steps=2, undirected="mean")
    assert bool(torch.isfinite(ig.gap).all()) and torch.equal(ig.twin.cpu(), edge_twins(b)[0])
