"""The per-graph attention forward as the tail of the last GCN layer's forward launch (k_gconv_fwd_att, gconv_fwd_att.hip:
engine_gconv.hpp compiled with CAL_GCF_ATT_UNIT + engine_attfwd_fold.hpp; Route::att_fwd_fold, switches CAL_AMD_ATT_FWD_FOLD and
StepEngine.set_att_fwd_fold): model.py:93-95 for layer L, then model.py:97-111 and gcn_conv.py:63-68, in ONE launch.

The folded launch adds a row's attention dots as 64 + 64 columns (the two slice workgroups of a graph exchange their partial
dots); k_att_fwd_graph's 32-lane tree ends with that very addition, and the halves are formed in its order, so anode, pq, att and
dis agree with the launch of its own bit for bit (asserted below) while the fp64 column statistics are added in another order.
Neither path is the reference, though: both are held to the SAME judge, a float64 restatement over the kernels' own operands,
tensor by tensor, with bounds that count the kernels' roundings (u = 2^-24; nothing is fitted to an output) --

  h_L      from the device's h_(L-1), dis and the layer's parameters: BatchNorm with fp64 batch statistics, x' W, A_hat z + b, ReLU.
           x' = x sc + sh carries 6 u M (M = |x sc| + |mean sc| + |beta|: the products, the add, sc and sh themselves), the
           statistics' error (the producer adds four values in fp32 before it goes to fp64: <= 4 u relative per sum and 5 u per sum of
           squares; 8 u taken) through mean and rstd = 1 / sqrtf(var + eps) (3 u); a dot of K = 128 products in any order is
           (K + 1) u sum |x' W|; a row of A_hat with n entries adds (n + 5) u (three roundings per coefficient, n for the sum, bias,
           spare).
  pq, logits   from the device's h_L: a dot of H = 128 products in any order, (H + 2) u sum |x w| (the fold's extra add of the two
           halves is inside "any order"; one spare).
  anode    the 2-way softmax of logits with error dl: a_k (a_other (dl_0 + dl_1 + u |l_0 - l_1| + x) + 4 u), x = 4 u the
           exponential's relative error (two ulp), 4 u for the sum, the reciprocal, the product and one spare.
  att      the same formula on the edge logits formed from the device's OWN pq (two adds: 2 u (|p| + |q| + |b|)).
  dis_c/o  from the device's OWN att: a sum of n + 1 positive fp32 terms (n u relative), halved by the power -1/2, and one rsqrt
           (sqrtf and the division, 1.5 u; 3 u taken): want (n / 2 + 3) u.
  bnc / bno sums   from the device's OWN anode and h_L: each term is one fp32 product (u) widened to fp64, its square 2 u, the
           fp64 sums N 2^-52: (u + N 2^-52) sum |a x| and (2 u + N 2^-52) sum (a x)^2.

test_the_fp32_restatement_is_inside_the_bounds (no GPU) shows that a plain fp32 evaluation of the same formulas passes the judge.
Cases: node counts 1, 31, 32, 33, 63, 64 with an edgeless graph, an empty graph in the middle and a hub; batches of 3 and 128
graphs (128 fills the launch); one graph alone trains on no route.  H = 64 and a batch with 2 T > CUs keep k_att_fwd_graph."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests.test_gpu_att_fold import NCLS, NFEAT, _model, _state
from tests.test_gpu_engine import LOGIT_TOL, _config2_batch, _stage_names

gpu = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
U = 2.0 ** -24
X_EXP = 4 * U
ST_U = 8 * U
LOOP_W = 1.0
EDGES = [(1, "rand"), (31, "rand"), (32, "none"), (0, "empty"), (33, "hub"), (63, "rand"), (64, "rand")]
THREE = [(20, "rand"), (64, "hub"), (5, "none")]


def _batch(spec, seed):
    """graphs without self loops, both directions of every edge (the per-graph kernels' batch layout)"""
    from cal_amd.data import Batch, Data
    g = torch.Generator().manual_seed(seed)
    ds = []
    for n, kind in spec:
        if n <= 1 or kind in ("none", "empty"):
            ei = torch.zeros(2, 0, dtype=torch.long)
        elif kind == "hub":
            leaves = torch.arange(1, n)
            ei = torch.cat([torch.stack([torch.zeros_like(leaves), leaves]), torch.stack([leaves, torch.zeros_like(leaves)])], 1)
        else:
            a = torch.rand(n, n, generator=g) < 0.08                   # (64 nodes: ~620 stored edges, under the 64-node kernels' 1024)
            a = a | a.t()
            a.fill_diagonal_(False)
            ei = a.nonzero().t().contiguous()
        ds.append(Data(x=torch.randn(n, NFEAT, generator=g), edge_index=ei, y=torch.randint(0, NCLS, (1,), generator=g)))
    return Batch.from_data_list(ds)


def _feat(b):
    return b.x if getattr(b, "x", None) is not None else b.feat


# ---- the judge -----------------------------------------------------------------------------------------------------------------
def _softmax2(l, dl):
    """(softmax over the two columns, its bound) for logits l with error bound dl"""
    a = torch.softmax(l, 1)
    delta = dl.sum(1, keepdim=True) + U * (l[:, :1] - l[:, 1:]).abs() + X_EXP
    return a, a * (a.flip(1) * delta + 4 * U)


def _judge(r, sd, ei, L, eps, fnode=1.0, fedge=1.0):
    """{name: (|got - want|, bound)} for the arrays r of one step (fp32 / fp64 CPU tensors), sd the parameters, ei edge_index"""
    H = r["h"].shape[2]
    N = r["h"].shape[1]
    src, dst = ei[0], ei[1]
    res = {}
    # h_L from h_(L-1)
    xin = r["h"][L - 1].to(F64)
    mean, ex2, mabs = xin.mean(0), (xin * xin).mean(0), xin.abs().mean(0)
    var = ex2 - mean * mean
    gamma, beta = sd["bns_conv.%d.weight" % (L - 1)].to(F64), sd["bns_conv.%d.bias" % (L - 1)].to(F64)
    W, bias = sd["convs.%d.weight" % (L - 1)].to(F64), sd["convs.%d.bias" % (L - 1)].to(F64)
    rstd = (var + eps) ** -0.5
    sc = gamma * rstd
    xp = xin * sc + (beta - mean * sc)
    dmean = ST_U * mabs
    drel = (ST_U * ex2 + 2 * mean.abs() * dmean) / (2 * (var + eps)) + 3 * U
    M = (xin * sc).abs() + (mean * sc).abs() + beta.abs()
    dxp = 6 * U * M + sc.abs() * dmean + ((xin - mean) * sc).abs() * drel
    z, zabs = xp @ W, xp.abs() @ W.abs()
    ez = dxp @ W.abs() + (H + 1) * U * zabs
    dis = r["dis_unit"].to(F64)
    coef, self_c = (dis[dst] * dis[src])[:, None], (dis * dis * LOOP_W)[:, None]
    agg = lambda v: torch.zeros(N, H, dtype=F64).index_add_(0, dst, coef * v[src]) + self_c * v
    nrow = (torch.bincount(dst, minlength=N) + 1).to(F64)[:, None]
    want = torch.relu(agg(z) + bias)
    res["h_L"] = ((r["h"][L].to(F64) - want).abs(), agg(ez) + (nrow + 5) * U * agg(zabs) + 2 * U * bias.abs())
    # the six dots from h_L
    x = r["h"][L].to(F64)
    Wn, bn = sd["node_att_mlp.weight"].to(F64), sd["node_att_mlp.bias"].to(F64)
    We, be = sd["edge_att_mlp.weight"].to(F64), sd["edge_att_mlp.bias"].to(F64)
    Wst = torch.cat([Wn, We[:, :H], We[:, H:]])                   # logits 0 / 1, p0, p1 (source half), q0, q1 (target half)
    D, ddot = x @ Wst.t(), (H + 2) * U * (x.abs() @ Wst.abs().t())
    res["pq"] = ((r["pq"].to(F64) - D[:, 2:]).abs(), ddot[:, 2:])
    l = D[:, :2] + bn
    a, ba = _softmax2(fnode * l, fnode * (ddot[:, :2] + U * l.abs()))
    res["anode"] = ((r["anode"].to(F64) - a).abs(), ba)
    # att from the device's own pq, dis from its own att
    pq = r["pq"].to(F64)
    le = torch.stack([pq[src, 0] + pq[dst, 2] + be[0], pq[src, 1] + pq[dst, 3] + be[1]], 1)
    dle = 2 * U * torch.stack([pq[src, 0].abs() + pq[dst, 2].abs() + be[0].abs(), pq[src, 1].abs() + pq[dst, 3].abs() + be[1].abs()], 1)
    ae, bae = _softmax2(fedge * le, fedge * dle)
    att = r["att"].to(F64)
    res["att"] = ((att.t() - ae).abs(), bae)
    nout = torch.bincount(src, minlength=N).to(F64)
    for k, name in enumerate(("dis_c", "dis_o")):
        deg = LOOP_W + torch.zeros(N, dtype=F64).index_add_(0, src, att[k])
        want = deg ** -0.5
        res[name] = ((r["dis_co"][k].to(F64) - want).abs(), want * (nout / 2 + 3) * U)
    # column sums of a_k x from the device's own anode
    an = r["anode"].to(F64)
    for k, name in enumerate(("bnc", "bno")):
        prod = an[:, k:k + 1] * x
        res[name + "_sum"] = ((r[name][0] - prod.sum(0)).abs(), (U + N * 2.0 ** -52) * prod.abs().sum(0))
        res[name + "_sq"] = ((r[name][1] - (prod * prod).sum(0)).abs(), (2 * U + N * 2.0 ** -52) * (prod * prod).sum(0))
    return res


def _worst(res):
    rat = {}
    for name, (err, bound) in res.items():
        assert bool(torch.isfinite(err).all()), name
        pos = bound > 0
        assert not bool((err[~pos] > 0).any()), name
        rat[name] = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return rat


def _report(tag, rat, check=True):
    """print the worst error / bound of every tensor; -> the tensors over their bound"""
    print("att_fwd_fold judge %-28s " % tag + " ".join("%s=%.3f" % kv for kv in sorted(rat.items())))
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not (check and bad), (tag, bad)
    return bad


# ---- no GPU: the reference alone is inside the bounds ----------------------------------------------------------------------------
def _fp32_restatement(sd, b, h_in, L, eps, fnode, fedge):
    """the formulas of _judge evaluated in fp32 (torch on the CPU), as a step's arrays"""
    f = torch.float32
    src, dst = b.edge_index
    N, H = h_in.shape
    mean, var = h_in.mean(0), h_in.var(0, unbiased=False)
    sc = sd["bns_conv.%d.weight" % (L - 1)] / torch.sqrt(var + eps)
    xp = h_in * sc + (sd["bns_conv.%d.bias" % (L - 1)] - mean * sc)
    z = xp @ sd["convs.%d.weight" % (L - 1)]
    deg = torch.bincount(dst, minlength=N).to(f) + LOOP_W
    dis = 1.0 / torch.sqrt(deg)
    out = torch.zeros(N, H).index_add_(0, dst, (dis[dst] * dis[src])[:, None] * z[src]) + (dis * dis * LOOP_W)[:, None] * z
    hL = torch.relu(out + sd["convs.%d.bias" % (L - 1)])
    Wn, We = sd["node_att_mlp.weight"], sd["edge_att_mlp.weight"]
    an = torch.softmax(fnode * (hL @ Wn.t() + sd["node_att_mlp.bias"]), 1)
    pq = torch.cat([hL @ We[:, :H].t(), hL @ We[:, H:].t()], 1)
    be = sd["edge_att_mlp.bias"]
    att = torch.softmax(fedge * torch.stack([pq[src, 0] + pq[dst, 2] + be[0], pq[src, 1] + pq[dst, 3] + be[1]], 1), 1).t().contiguous()
    dco = torch.stack([1.0 / torch.sqrt(LOOP_W + torch.zeros(N).index_add_(0, src, att[k])) for k in range(2)])
    rows = {}
    for k, name in enumerate(("bnc", "bno")):
        p = (an[:, k:k + 1] * hL).to(F64)
        rows[name] = torch.stack([p.sum(0), (p * p).sum(0)])
    return dict(h=torch.stack([h_in] * L + [hL]), dis_unit=dis, anode=an, pq=pq, att=att, dis_co=dco, **rows)


@pytest.mark.parametrize("fnode,fedge", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0)])
def test_the_fp32_restatement_is_inside_the_bounds(fnode, fedge):
    L, H = 2, 128
    sd = _state("CausalGCN", H, L)
    b = _batch([(n, k) for n, k in EDGES if n > 0] + THREE, 11)
    h_in = torch.relu(torch.randn(b.x.shape[0], H, generator=torch.Generator().manual_seed(4)) + 0.3)
    r = _fp32_restatement(sd, b, h_in, L, 1e-5, fnode, fedge)
    _report("fp32 restatement %g %g" % (fnode, fedge), _worst(_judge(r, sd, b.edge_index, L, 1e-5, fnode, fedge)))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _bn_rows(eng, k, H):
    """[2, H]: column sums and sums of squares of BatchNorm k as the step left them in the arena (the four planes added)"""
    from cal_amd import _lib
    out = (ctypes.c_int64 * 3)()
    _lib.call("cal_engine_bn_arena", eng._h, k, out)
    off, w, plane = int(out[0]), int(out[1]), int(out[2])
    arena = eng.buffer("arena", off + 2 * w + 3 * plane, torch.float64).cpu()
    return torch.stack([sum(arena[off + q * w + p * plane: off + q * w + p * plane + H] for p in range(4)) for q in range(2)])


def _run(fold, sd, bd, perm, hidden, layers, steps=0, **kw):
    """one train step (no Adam; steps > 0: that many Adam steps instead) of a fresh engine with the fold on / off"""
    from cal_amd.engine import StepEngine
    m = _model("CausalGCN", sd, hidden, layers, **kw)
    eng = StepEngine(m, lr=1e-3)
    eng.set_att_fwd_fold(fold)
    if steps:
        stats = torch.stack([eng.train_step(bd, perm.to(DEV), adam=True).clone() for _ in range(steps)]).cpu()
    else:
        stats = eng.train_step(bd, perm.to(DEV), adam=False).cpu().clone()
    eng.check_status()
    N, E, B, H, L = _feat(bd).shape[0], bd.edge_index.shape[1], int(perm.numel()), hidden, layers
    return dict(h=eng.buffer("h", (L + 1) * N * H).view(L + 1, N, H).cpu().clone(), dis_unit=eng.buffer("dis_unit", N).cpu().clone(),
                anode=eng.buffer("anode", 2 * N).view(N, 2).cpu().clone(), pq=eng.buffer("pq", 4 * N).view(N, 4).cpu().clone(),
                att=eng.buffer("att", 2 * E).view(2, E).cpu().clone(), dis_co=eng.buffer("dis_co", 2 * N).view(2, N).cpu().clone(),
                bnc=_bn_rows(eng, L + 1, H), bno=_bn_rows(eng, L + 2, H), stats=stats, names=_stage_names(),
                logp=eng.buffer("logp", 3 * B * NCLS).cpu().clone(), flat_p=eng.flat_p.detach().cpu().clone(),
                grads={k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None},
                eps=float(m.bns_conv[L - 1].eps))


def _folded(names):
    return "k_gconv_fwd_att" in names and "k_att_fwd_graph" not in names


def _judge_both(tag, b, bd, hidden, layers, **kw):
    """b / bd: the batch on the CPU and on the GPU.  Fold on and off on the same state, both through the judge."""
    B = int(b.y.numel())
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    sd = _state("CausalGCN", hidden, layers)
    ei = b.edge_index
    fn = 0.0 if kw.get("without_node_attention") else 1.0
    fe = 0.0 if kw.get("without_edge_attention") else 1.0
    runs, bad = {}, {}
    for fold in (True, False):
        r = runs[fold] = _run(fold, sd, bd, perm, hidden, layers, **kw)
        assert _folded(r["names"]) == fold, r["names"]
        bad[fold] = _report("%s fold=%d" % (tag, fold), _worst(_judge(r, sd, ei, layers, r["eps"], fn, fe)), check=False)
    assert not bad[True] and not bad[False], bad
    # layer L's own output does not depend on the tail: the same instructions wrote it
    assert torch.equal(runs[True]["h"], runs[False]["h"])
    for k in ("anode", "pq", "att", "dis_co"):                        # the dots are added in k_att_fwd_graph's order
        assert torch.equal(runs[True][k], runs[False][k]), k
    assert len(runs[True]["names"]) == len(runs[False]["names"]) - 2, (runs[True]["names"], runs[False]["names"])
    return runs


@gpu
@pytest.mark.parametrize("layers", [2, 3])
def test_folded_launch_on_the_tile_edges_passes_the_fp64_judge(layers):
    _judge_both("edges L=%d" % layers, _batch(EDGES, 5), _batch(EDGES, 5).to(DEV), 128, layers)


@gpu
def test_folded_launch_on_three_graphs_passes_the_fp64_judge():
    _judge_both("three", _batch(THREE, 6), _batch(THREE, 6).to(DEV), 128, 2)


@gpu
def test_folded_launch_that_fills_the_chip_passes_the_fp64_judge():
    b, bd = _config2_batch(128)
    assert 2 * 128 <= torch.cuda.get_device_properties(0).multi_processor_count
    _judge_both("128 graphs", b, bd, 128, 3)


@gpu
@pytest.mark.parametrize("kw", [dict(without_node_attention=True), dict(without_edge_attention=True),
                                dict(without_node_attention=True, without_edge_attention=True)], ids=["no-node", "no-edge", "neither"])
def test_folded_launch_with_attention_switched_off(kw):
    _judge_both("flags " + ",".join(sorted(kw)), _batch(EDGES, 7), _batch(EDGES, 7).to(DEV), 128, 2, **kw)


@gpu
def test_one_graph_alone_is_refused_with_the_fold_as_without():
    from cal_amd.engine import StepEngine
    bd1 = _batch([(33, "rand")], 5).to(DEV)
    sd = _state("CausalGCN", 128, 2)
    for fold in (True, False):
        eng = StepEngine(_model("CausalGCN", sd, 128, 2), lr=1e-3)
        eng.set_att_fwd_fold(fold)
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            eng.train_step(bd1, torch.zeros(1, dtype=torch.long, device=DEV), adam=False)


@gpu
def test_hidden_64_and_more_workgroups_than_cus_keep_the_attention_launch(monkeypatch):
    """H = 64 is one slice (nothing to exchange); 140 graphs x 2 slices are more workgroups than CUs (no co-residency);
    an evaluation forward and CAL_AMD_ATT_FWD_FOLD=0 keep k_att_fwd_graph as well"""
    from cal_amd.engine import StepEngine
    many = [(3 + i % 4, "rand") for i in range(140)]
    assert 2 * len(many) > torch.cuda.get_device_properties(0).multi_processor_count
    for spec, hidden in ((EDGES, 64), (many, 128)):
        bd = _batch(spec, 8).to(DEV)
        perm = torch.randperm(len(spec), generator=torch.Generator().manual_seed(1))
        sd = _state("CausalGCN", hidden, 2)
        on, off = _run(True, sd, bd, perm, hidden, 2), _run(False, sd, bd, perm, hidden, 2)
        assert "k_gconv_fwd_att" not in on["names"] and on["names"] == off["names"], on["names"]
        assert "k_att_fwd_graph" in on["names"] or "k_node_att_fwd" in on["names"], on["names"]
        assert torch.equal(on["logp"], off["logp"])
    bd = _batch(EDGES, 8).to(DEV)
    perm = torch.randperm(len(EDGES), generator=torch.Generator().manual_seed(1)).to(DEV)
    sd = _state("CausalGCN", 128, 2)
    eng = StepEngine(_model("CausalGCN", sd, 128, 2), lr=1e-3)
    eng.forward(bd, perm, training=False)
    assert "k_gconv_fwd_att" not in _stage_names() and "k_att_fwd_graph" in _stage_names()
    eng.train_step(bd, perm, adam=False)
    assert _folded(_stage_names())                                   # (on by default)
    monkeypatch.setenv("CAL_AMD_ATT_FWD_FOLD", "0")
    eng = StepEngine(_model("CausalGCN", sd, 128, 2), lr=1e-3)
    eng.train_step(bd, perm, adam=False)
    eng.check_status()
    assert "k_gconv_fwd_att" not in _stage_names() and "k_att_fwd_graph" in _stage_names()


@gpu
def test_folded_step_matches_the_oracle_also_after_three_adam_steps():
    """the whole step at the headline shape against the CPU oracle, tolerances of tests/test_gpu_engine.py"""
    b, bd = _config2_batch(128)
    hidden, layers, B = 128, 3, 128
    torch.manual_seed(5)
    sd = O.init_state("CausalGCN", NFEAT, NCLS, hidden=hidden, layers=layers)
    _model("CausalGCN", sd, hidden, layers)                            # (that test builds its model here: the generator moves as it does there)
    perm = torch.randperm(B)                                           # (state, batch and permutation of test_config2_scale_step_matches_oracle)
    on, off = _run(True, sd, bd, perm, hidden, layers), _run(False, sd, bd, perm, hidden, layers)
    assert _folded(on["names"]) and not _folded(off["names"]), on["names"]
    tr = O.CpuTrainer("CausalGCN", {k: v.clone() for k, v in sd.items()}, NCLS, lr=1e-3, layers=layers)
    loss, lc, lo, lco, logits = tr.step(_feat(b), b.edge_index, b.batch, b.y, perm=perm)
    for r, t in zip(logits, on["logp"].view(3, B, NCLS)):              # (that test's bounds)
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(on["stats"].numpy()[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    worst = {}
    for tag, run in (("fold=1", on), ("fold=0", off)):
        worst[tag] = max(((g - tr.sd[k].grad).abs() / (5e-5 + 2e-3 * tr.sd[k].grad.abs())).max().item()
                         for k, g in run["grads"].items() if tr.sd[k].grad is not None)
    print("att_fwd_fold whole step: worst gradient error / (5e-5 + 2e-3 |ref|): %s" % worst)
    for k, g in on["grads"].items():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(g, gref, atol=5e-5, rtol=2e-3), k
    # three Adam steps (test_three_steps_track_the_oracle's bound; the oracle has taken the first one above)
    three = _run(True, sd, bd, perm, hidden, layers, steps=3)
    assert abs(three["stats"][0][0].item() - loss.item()) < 2e-3
    for step in (1, 2):
        loss, *_ = tr.step(_feat(b), b.edge_index, b.batch, b.y, perm=perm)
        assert abs(three["stats"][step][0].item() - loss.item()) < 2e-3 * (step + 1), step


@gpu
def test_two_folded_runs_agree_to_the_order_of_the_atomics():
    bd = _batch(EDGES, 9).to(DEV)
    perm = torch.randperm(len(EDGES), generator=torch.Generator().manual_seed(3))
    sd = _state("CausalGCN", 128, 2)
    u, v = (_run(True, sd, bd, perm, 128, 2, steps=3) for _ in range(2))
    assert _folded(u["names"])
    for k in ("logp", "stats", "flat_p"):
        assert torch.allclose(u[k], v[k], atol=1e-5, rtol=1e-5), k    # (test_deterministic_engine_is_bit_reproducible's bound for the striped sums)
    for k in ("anode", "pq", "att", "dis_co"):
        assert torch.allclose(u[k], v[k], atol=1e-5, rtol=1e-5), k
