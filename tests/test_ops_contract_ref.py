"""tests/ops_contract_ref.py and tests/ops_contract_cases.py held to what the project already trusts, on the CPU:

  * the case table is complete: all 56 instantiations of the ten dispatched kernels, each (VEC, G) once filled and once with idle
    lanes, every sweep count, every part count of finish_colsum, every axis value per launcher, every aligned16 term isolated;
  * the reference is oracle.cal_oracle (gcn_conv, global_add_pool), torch autograd in float64 for every backward, and numpy's
    stable argsort for the plan;
  * libcalhost.so -- the same symbols in plain fp32 C++, every launcher of the table is exported there -- sits inside every
    bound on EVERY case of the table (no case exempted): the bounds are not too tight for an honest fp32 implementation;
  * fourteen seeded defects of the reference's outputs, on the table's own inputs, each exceed a bound or fail an exactness check.
"""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests import ops_contract_cases as C
from tests import ops_contract_ref as R
from tests import sparse_contract_ref as sref
from tests.test_sparse_contract_ref import _graph

F64 = torch.float64
TOL = dict(rtol=1e-12, atol=1e-13)


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_cases_reach_all_56_instantiations_with_every_axis_value():
    seen, sweeps, nparts = {}, {}, set()
    for c in C.CASES:
        ps, np_ = C.paths(c)
        for k, vec, G, sw in ps:
            seen.setdefault((k, vec, G), []).append(c)
            sweeps.setdefault((k, vec), set()).add(sw)
        if np_ is not None:
            nparts.add((c["launcher"], np_))
    gk = [k for L in C.LAUNCHERS.values() for k in L["g"]]
    ck = [k for L in C.LAUNCHERS.values() for k in L["col"]]
    assert len(gk) == 6 and len(ck) == 4
    want = {(k, v, G) for k in gk for v in (4, 1) for G in (8, 16, 32, 64)} | {(k, v, 0) for k in ck for v in (4, 1)}
    assert set(seen) == want and len(want) == 56
    for (k, vec, G), cs in seen.items():
        if G:                                                   # once filling the group, once leaving lanes idle
            assert any(c["H"] == G * vec for c in cs) and any(c["H"] < G * vec for c in cs), (k, vec, G)
    for k in gk:
        assert sweeps[(k, 4)] >= {1, 2} and sweeps[(k, 1)] >= {1, 2, 3}, k
    for k in ck:
        assert sweeps[(k, 4)] == {1, 2} and sweeps[(k, 1)] == {1, 2}, k
    for L in C.FINISH:
        assert {p for l, p in nparts if l == L} >= {0, 1, 2, 16, 17, 32, 33, 48, 49, 497}, L
    assert C.rows_per_block(C.BIG_N) == 34 and C.rows_per_block(16384) == 32
    for name, L in C.LAUNCHERS.items():
        cs = C.cases_of(name)
        for t in L["terms"]:                                    # the only false term, on a width that would vectorise
            assert any(c["off"] == {t: 1} and c["H"] % 4 == 0 for c in cs), (name, t)
        assert {c["H"] for c in cs if c["off"]} >= set(C.MIS_WIDTHS) or not L["terms"], name
        assert any(C.graph_of(c["graph"])["N"] == 0 for c in cs) or name == "add_pool_fwd", name
    ax = lambda name, key: {c[key] for c in C.cases_of(name)}
    assert ax("spmm", "relu") == {0, 1} and ax("spmm", "bias") == {0, 1} and ax("spmm", "loop_w") == set(C.LOOP_W) and ax("spmm", "key") == {0, 1}
    assert any(c["key"] == 0 and not c["bias"] for c in C.cases_of("spmm")) and any(c["unit"] for c in C.cases_of("spmm"))
    assert any(c["H"] == 1 and c["loop_w"] == 0 for c in C.cases_of("spmm"))
    assert ax("norm_fwd", "w") == {0, 1} and ax("norm_fwd", "loop_w") == set(C.LOOP_W)
    assert ax("norm_bwd", "w") == {0, 1} and ax("norm_bwd", "loop_w") == set(C.LOOP_W)
    assert ax("relu_bwd_colsum", "y") == {0, 1} and ax("relu_bwd_colsum", "dz") == {"buf", "null", "alias"} and ax("relu_bwd_colsum", "dbias") == {0, 1}
    assert ax("edge_att_bwd", "accumulate") == {0, 1} and ax("add_pool_fwd", "S") == set(C.SPLITS)
    for name in ("norm_fwd", "norm_bwd", "spmm", "edge_att_fwd", "edge_att_bwd"):
        assert any(C.graph_of(c["graph"])["E"] == 0 and C.graph_of(c["graph"])["N"] > 0 for c in C.cases_of(name)), name
    for S in C.SPLITS:                                          # graph lengths 0, 1, below S, no multiple of S
        assert 0 in C.POOL_SIZES and 1 in C.POOL_SIZES and (S == 1 or any(1 < n < S or n == 1 for n in C.POOL_SIZES))
        assert S == 1 or any(n > S and n % S for n in C.POOL_SIZES)
    # the plan's scans
    scans = {k: C.plan_scan(f()[1], f()[0].shape[1]) for k, f in C.PLAN_CASES.items()}
    assert scans["N8192"] == ("single", 1) and scans["N8193"] == ("single", 2) and scans["N32768"] == ("single", 4)
    assert scans["N32769-chunked"] == ("chunked", 5) and scans["N40000-E9"] == ("single", 5) and 32769 - 4 * 8192 == 1


def test_ladder_and_signed_graphs_hold_what_the_cases_need():
    for key in (0, 1):
        g = C.graph_of(("ladder", key))
        rows = np.diff(g["src" if key == 0 else "dst"][0])
        assert {int(r) % 4 for r in rows} == {0, 1, 2, 3} and rows.max() == 193 and rows.min() == 0
        assert g["N"] == 301 and all(301 % (256 // G) for G in (8, 16, 32, 64)) and int(g["loops"].sum()) == 5
    g = C.graph_of(("signed",))
    dis, ne, deg, _ = R.norm_fwd(g["src"][0], g["src"][2], g["ei"][0], g["ei"][1], g["w"], 0.0)
    assert deg[0] == 0 and dis[0] == 0 and deg[1] < 0 and bool(torch.isnan(dis[1])) and deg[2] == 0 and int(torch.isnan(dis).sum()) == 1
    assert bool((deg[4:] > 0).all()) and int(torch.isnan(ne).sum()) == 2 and int(g["loops"].sum()) >= 3


# ---- the reference is the oracle, autograd and numpy -------------------------------------------------------------------
@pytest.mark.parametrize("loop_w", [1.0, 2.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_norm_and_aggregation_are_the_oracle_gcn_conv(weighted, loop_w):
    ei, batch, N, g = _graph(3)
    H, E = 9, ei.shape[1]
    x, bias = torch.randn(N, H, generator=g, dtype=F64), torch.randn(H, generator=g, dtype=F64)
    w = (0.05 + 0.95 * torch.rand(E, generator=g, dtype=F64)) if weighted else None
    want = O.gcn_conv(x, torch.from_numpy(ei), torch.eye(H, dtype=F64), bias, w, loop_w == 2.0)
    src, dst = sref.csr_view(ei, N, 0), sref.csr_view(ei, N, 1)
    wn = None if w is None else torch.where(torch.from_numpy(ei[0] == ei[1]), torch.full_like(w, float("nan")), w)
    dis, ne, _, _ = R.norm_fwd(src[0], src[2], ei[0], ei[1], wn, loop_w)       # NaN on the self-loop columns changes nothing
    assert bool(torch.isfinite(ne).all()) and bool((ne[torch.from_numpy(ei[0] == ei[1])] == 0).all())
    for relu in (0, 1):
        out, T, n = R.spmm(*dst, ne, dis, loop_w, x, bias, relu)
        assert torch.allclose(out, torch.relu(want) if relu else want, **TOL) and bool((T >= out.abs() - 1e-12).all())
    pooled, _ = R.add_pool(x, R.graph_ptr(batch, 3))
    assert torch.allclose(pooled, O.global_add_pool(x, torch.from_numpy(batch), 3), **TOL)
    assert torch.equal(R.add_pool_bwd(pooled, batch), pooled[torch.from_numpy(batch)])


@pytest.mark.parametrize("loop_w", [0.5, 1.0, 1.25])          # 0 would leave the isolated nodes of this graph without a degree
def test_norm_bwd_is_autograd_through_the_normalisation(loop_w):
    ei, _, N, g = _graph(4)
    H, E = 7, ei.shape[1]
    r, c = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    keep = r != c
    h, dz = torch.randn(N, H, generator=g, dtype=F64), torch.randn(N, H, generator=g, dtype=F64)
    w = (0.05 + 0.95 * torch.rand(E, generator=g, dtype=F64)).requires_grad_(True)
    deg = torch.full((N,), loop_w, dtype=F64).index_add(0, r[keep], w[keep])
    dis = deg ** -0.5
    norm = dis[r] * w * dis[c]
    out = torch.zeros(N, H, dtype=F64).index_add(0, c[keep], norm[keep][:, None] * h[r[keep]]) + (dis * dis * loop_w)[:, None] * h
    (out * dz).sum().backward()
    src, dst = sref.csr_view(ei, N, 0), sref.csr_view(ei, N, 1)
    wn = torch.where(keep, w.detach(), torch.full_like(w.detach(), float("nan")))
    gn, gself, ddeg, dw = R.norm_bwd(src, dst, ei[0], ei[1], wn, dis.detach(), loop_w, h, dz)
    assert torch.allclose(dw, w.grad, rtol=1e-12, atol=1e-12 * float(w.grad.abs().max()))
    assert bool((dw[~keep] == 0).all()) and bool(torch.isnan(gn[~keep]).all()) and bool(torch.isfinite(gn[keep]).all())
    # the transposed aggregation is d/dh: cal_spmm_fwd on the by-source view, no bias
    hh = h.clone().requires_grad_(True)
    o2 = torch.zeros(N, H, dtype=F64).index_add(0, c[keep], norm.detach()[keep][:, None] * hh[r[keep]]) + (dis.detach() ** 2 * loop_w)[:, None] * hh
    (o2 * dz).sum().backward()
    assert torch.allclose(R.spmm(*src, norm.detach(), dis.detach(), loop_w, dz, None, 0)[0], hh.grad, **TOL)
    # and ReLU backward + bias gradient
    y = torch.relu(torch.randn(N, H, generator=g, dtype=F64)).requires_grad_(True)
    b = torch.zeros(H, dtype=F64, requires_grad=True)
    pre = y.detach() - 0.3
    pre.requires_grad_(True)
    (torch.relu(pre + b) * dz).sum().backward()
    dzr, db, _ = R.relu_bwd_colsum(dz, torch.relu(pre.detach()))
    assert torch.allclose(dzr, pre.grad, **TOL) and torch.allclose(db, b.grad, **TOL)


def test_attention_backwards_are_autograd():
    ei, _, N, g = _graph(5)
    H, E = 6, ei.shape[1]
    r, c = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    keep = r != c
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, W, b = rn(N, H).requires_grad_(True), rn(2, 2 * H).requires_grad_(True), rn(2).requires_grad_(True)
    datt = rn(2, E)
    att = torch.softmax(torch.cat([x[r], x[c]], 1) @ W.t() + b, -1).t()              # [2, E], model.py:97-104
    (att[:, keep] * datt[:, keep]).sum().backward()                                  # self-loop columns reach no conv
    pq = R.edge_proj(x.detach(), W.detach())[0]
    assert torch.allclose(R.edge_att_from_pq(pq, b.detach(), ei[0], ei[1])[0].t(), att.detach(), **TOL)
    src, dst = sref.csr_view(ei, N, 0), sref.csr_view(ei, N, 1)
    dn = datt.clone()
    dn[:, ~keep] = float("nan")
    base = rn(N, H)
    (dx, dW, db), bnd = R.edge_att_bwd(x.detach(), W.detach(), att.detach(), dn, (src[0], src[2]), (dst[0], dst[2]), base)
    rel = lambda a, b_: float((a - b_).abs().max()) <= 1e-12 * float(b_.abs().max())
    assert rel(dx - base, x.grad) and rel(dW, W.grad) and rel(db, b.grad)
    assert all(bool(torch.isfinite(t).all()) and bool((t >= 0).all()) for t in bnd)
    # node attention, model.py:106-111
    x2, Wn, bn = rn(N, H).requires_grad_(True), rn(2, H).requires_grad_(True), rn(2).requires_grad_(True)
    dxc, dxo = rn(N, H), rn(N, H)
    a = torch.softmax(x2 @ Wn.t() + bn, -1)
    ((a[:, 0:1] * x2) * dxc + (a[:, 1:2] * x2) * dxo).sum().backward()
    an = R.node_att(x2.detach(), Wn.detach(), bn.detach())[0]
    assert torch.allclose(an, a.detach(), **TOL)
    (dx, dWn, dbn), _ = R.node_att_bwd(x2.detach(), Wn.detach(), an, dxc, dxo)
    assert rel(dx, x2.grad) and rel(dWn, Wn.grad) and rel(dbn, bn.grad)


def test_plan_is_numpys_stable_argsort():
    for name in ("ladder-dst", "duplicates", "hub", "out-of-range"):
        ei, n = C.PLAN_CASES[name]()
        p = R.plan(ei, n)
        bad = ((ei < 0) | (ei >= n)).any(0)
        assert p["status"] == int(name == "out-of-range") == int(bad.any())
        for nm, key in (("dst", 1), ("src", 0)):
            ok = np.nonzero((ei[0] != ei[1]) & ~bad)[0]
            order = ok[np.argsort(ei[key][ok], kind="stable")]
            assert np.array_equal(p["eid_" + nm], order) and np.array_equal(p["nbr_" + nm], ei[1 - key][order])
            assert np.array_equal(p["rowptr_" + nm], np.concatenate([[0], np.cumsum(np.bincount(ei[key][ok], minlength=n))]))
            for v in (7, 8):
                s = p["eid_" + nm][p["rowptr_" + nm][v]:p["rowptr_" + nm][v + 1]]
                assert (np.diff(s) > 0).all()
    for name, (batch, B, valid) in C.GRAPH_PTR_CASES.items():
        assert R.graph_ptr_valid(batch, B) == valid, name
        if valid:
            gp = R.graph_ptr(batch, B)
            assert np.array_equal(np.diff(gp), np.bincount(batch, minlength=B)[:B]) and gp[0] == 0 and gp[-1] == len(batch)


# ---- the host twin: plain fp32 C++ inside every bound, on every case --------------------------------------------------------
def _host_exp_error():
    """largest relative error of the C library's expf on [-12, 0] against fp64 exp, at least one ulp (2 u): the `x` of the att bound"""
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.expf.restype, m.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    xs = np.linspace(-12.0, 0.0, 1 << 13, dtype=np.float32)
    got = np.array([m.expf(float(v)) for v in xs], np.float64)
    want = np.exp(xs.astype(np.float64))
    return max(float((np.abs(got - want) / want).max()), 2 * R.U)


@pytest.mark.parametrize("launcher", list(C.LAUNCHERS))
def test_host_twin_is_inside_every_bound_on_every_case(launcher):
    """Worst err / bound of libcalhost.so per launcher (bound 1): norm_fwd dis 0.15, norm_e 0.45; spmm 0.38; relu_bwd_colsum dz
    exact, dbias 0.011 (its column sums are float64); norm_bwd gn_e 0.54, gself 0.52, ddeg 0.32, dw 0.52; edge_att_fwd pq 0.53, att
    0.25; edge_att_bwd dx 0.38, dW 0.0096, db 0.0055; node_att_fwd att_n 0.15, xc / xo 0.998; node_att_bwd dx 0.44, dWn 0.0075, dbn
    0.0047; add_pool_fwd 0.998; add_pool_bwd exact.  Every launcher of the table is exported by the host library: none is judged
    through a numpy stand-in."""
    x = _host_exp_error()
    worst, bad = {}, []
    cs = C.cases_of(launcher)
    assert cs
    for c in cs:
        i = C.inputs_of(c)
        got, fails = C.run(c, i, C.HostBackend())
        rat, f2 = C.judge(c, i, got, x)
        bad += ["%s: %s" % (c["name"], f) for f in fails + f2]
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%-16s %3d cases, worst err/bound %s" % (launcher, len(cs), {k: "%.3g" % v for k, v in worst.items()}))
    assert not bad, "\n".join(bad)
    assert all(v <= 1.0 for v in worst.values())


def test_host_twin_plan_and_graph_ptr_are_exact():
    for name, f in C.PLAN_CASES.items():
        ei, n = f()
        be = C.HostBackend()
        got = {k: be.cpu(v).numpy() for k, v in C.launch_plan(ei, n, be).items()}
        assert be.intact() and not C.judge_plan(ei, n, got), (name, C.judge_plan(ei, n, got))
    for name, (batch, B, valid) in C.GRAPH_PTR_CASES.items():
        be = C.HostBackend()
        got = {k: be.cpu(v).numpy() for k, v in C.launch_graph_ptr(batch, B, be).items()}
        assert be.intact() and not C.judge_graph_ptr(batch, B, valid, got), name


# ---- sensitivity: seeded defects of the reference exceed the bounds -----------------------------------------------------
def _first(launcher, pred):
    return next(c for c in C.cases_of(launcher) if pred(c))


def _drop_last_of_rows_mod4_3(view):
    ptr, nbr, eid = view
    deg = np.diff(ptr)
    drop = np.zeros(len(nbr), bool)
    drop[(ptr[1:] - 1)[deg % 4 == 3]] = True
    return np.concatenate([[0], np.cumsum(deg - (deg % 4 == 3))]).astype(np.int32), nbr[~drop], eid[~drop]


def _d_spmm(c, i, good, what):
    G = i["G"]
    view = G["dst"] if c["key"] == 1 else G["src"]
    a = (i["norm_e"], i["dis"], c["loop_w"], i["h"], i["bias"], c["relu"])
    if what == "last slot":
        return dict(out=R.spmm(*_drop_last_of_rows_mod4_3(view), *a)[0])
    if what == "no loop":
        return dict(out=R.spmm(*view, a[0], a[1], 0.0, *a[3:])[0])
    if what == "loop_w once":
        return dict(out=sref.aggregate(*view, i["h"], torch.ones(i["N"], dtype=F64), i["norm_e"], c["loop_w"], i["bias"], c["relu"])[0])
    if what == "bias after relu":
        return dict(out=torch.relu(R.spmm(*view, a[0], a[1], a[2], a[3], None, 0)[0]) + i["bias"].double())
    if what == "second sweep":
        out = good["out"].clone()
        out[:, 256:] = float("nan")
        return dict(out=out)


def _d_norm_bwd(c, i, good, what):
    G = i["G"]
    if what == "upper half of G 16":
        h2 = i["h"].clone()
        h2[:, (torch.arange(c["H"]) // 4) % 16 >= 8] = 0
        gn, gs, _, _ = R.sddmm(*G["dst"], h2, i["dz"], i["E"])
        return dict(good, gn_e=gn, gself=gs)
    if what == "ddeg from col":
        r, cc = torch.from_numpy(G["ei"][0]), torch.from_numpy(G["ei"][1])
        p = good["gn_e"] * i["dis"].double()[r] * i["dis"].double()[cc]
        return dict(good, dw=torch.where(r != cc, p + good["ddeg"][cc], torch.zeros_like(p)))
    if what == "self-loop column not zeroed":
        r, cc = torch.from_numpy(G["ei"][0]), torch.from_numpy(G["ei"][1])
        return dict(good, dw=torch.where(r != cc, good["dw"], good["ddeg"][r]))


def _d_node_bwd(c, i, good, what):
    N = i["N"]
    keep = torch.ones(N, dtype=torch.bool)
    if what == "part lane p + 16":
        rpb = C.rows_per_block(N)
        part = torch.arange(N) // rpb
        keep = (part % 32) < 16
    sub = R.node_att_bwd(i["x"][keep], i["Wn"], i["att_n"][keep], i["dxc"][keep], i["dxo"][keep])[0]
    return dict(good, dWn=sub[1], dbn=sub[2])


def _d_relu(c, i, good, what):
    N = i["N"]
    extra = C.rows_per_block(N) * C.parts(N) - N                # rows of the last block past N: they hold the canary
    return dict(good, dbias=good["dbias"] + extra * C.CANARY)


def _d_edge_bwd(c, i, good, what):
    if what == "dW[1] sign":
        return dict(good, dW=torch.stack([good["dW"][0], good["dW"][0]]))
    if what == "accumulate ignored":
        return dict(good, dx=good["dx"] - i["base"].double())


def _d_pool(c, i, good, what):
    out, S, gp = good["out"].clone(), c["S"], i["gptr"]
    for b in range(i["B"]):
        n0, n1 = int(gp[b]), int(gp[b + 1])
        chunk = -(-(n1 - n0) // S)
        for sp in range(1, S):
            if chunk and n0 + sp * chunk < n1:
                out[b] += i["x"][n0 + sp * chunk].double()      # the slice before read one row too many
    return dict(out=out)


def _d_second_sweep_dot(c, i, good, what):
    a = R.node_att(i["x"][:, :64 * 4], i["Wn"][:, :64 * 4], i["bn"])[0]
    xc, xo = R.node_split_from(a, i["x"])
    return dict(att_n=a, xc=xc, xo=xo)


FLOAT_DEFECTS = [      # (what, case, the reference with the defect)
    ("last slot", lambda: C.case_by_name("spmm/H64"), _d_spmm),
    ("no loop", lambda: _first("spmm", lambda c: c["loop_w"] == 1.0 and c["graph"][0] == "ladder"), _d_spmm),
    ("loop_w once", lambda: _first("spmm", lambda c: c["loop_w"] == 2.0 and not c["unit"] and c["graph"][0] == "ladder"), _d_spmm),
    ("bias after relu", lambda: _first("spmm", lambda c: c["relu"] and c["bias"]), _d_spmm),
    ("second sweep", lambda: C.case_by_name("spmm/H260"), _d_spmm),
    ("second sweep of the dot", lambda: C.case_by_name("node_att_fwd/H260"), _d_second_sweep_dot),
    ("upper half of G 16", lambda: C.case_by_name("norm_bwd/H64"), _d_norm_bwd),
    ("ddeg from col", lambda: C.case_by_name("norm_bwd/H20"), _d_norm_bwd),
    ("self-loop column not zeroed", lambda: C.case_by_name("norm_bwd/H20"), _d_norm_bwd),
    ("part lane p + 16", lambda: C.case_by_name("node_att_bwd/N1025"), _d_node_bwd),
    ("rows past N", lambda: _first("relu_bwd_colsum", lambda c: c["dbias"] and c["graph"] in [("rand", n) for n in (33, 513, 1025, 1537)]), _d_relu),
    ("dW[1] sign", lambda: C.case_by_name("edge_att_bwd/H36"), _d_edge_bwd),
    ("accumulate ignored", lambda: _first("edge_att_bwd", lambda c: c["accumulate"] and C.graph_of(c["graph"])["N"] > 0), _d_edge_bwd),
    ("slices overlap", lambda: _first("add_pool_fwd", lambda c: c["S"] == 3), _d_pool),
]


@pytest.mark.parametrize("what", [d[0] for d in FLOAT_DEFECTS])
def test_seeded_defects_of_the_reference_exceed_the_bounds(what):
    _, pick, make = next(d for d in FLOAT_DEFECTS if d[0] == what)
    c = pick()
    i = C.inputs_of(c)
    good = C.reference(c, i)
    rat, fails = C.judge(c, i, good)
    assert not fails and max(rat.values()) == 0.0, (c["name"], rat, fails)           # the reference against itself
    rat, fails = C.judge(c, i, {k: v.float() for k, v in C.reference(c, i, stored=True).items()})
    assert not fails and max(rat.values()) <= 1.0, (c["name"], rat, fails)           # rounded to fp32: still inside every bound
    rat, fails = C.judge(c, i, make(c, i, good, what))
    print("%-32s %-28s worst err/bound %.3e" % (what, c["name"], max(rat.values())))
    assert fails and max(rat.values()) > 1.0, (what, c["name"], rat)


def test_seeded_defects_of_the_plan_fail_the_exact_comparison():
    ei, n = C.PLAN_CASES["hub"]()
    good = dict(R.plan(ei, n), status=np.array([0]))
    assert not C.judge_plan(ei, n, good)
    bad = {k: np.array(v, copy=True) for k, v in good.items()}
    s = bad["rowptr_dst"][7]
    for k in ("nbr_dst", "eid_dst"):                            # the rank unstable under equal keys: two slots of the hub swapped
        bad[k][[s, s + 1]] = bad[k][[s + 1, s]]
    assert C.judge_plan(ei, n, bad)
    ei, n = C.PLAN_CASES["N8193"]()
    good = dict(R.plan(ei, n), status=np.array([0]))
    bad = {k: np.array(v, copy=True) for k, v in good.items()}
    bad["rowptr_src"][8192:] -= bad["rowptr_src"][8192]          # the scan's carry lost between two passes
    assert not C.judge_plan(ei, n, good) and C.judge_plan(ei, n, bad)
    batch, B, _ = C.GRAPH_PTR_CASES["empty-first-middle-last"]
    gp = R.graph_ptr(batch, B)
    assert not C.judge_graph_ptr(batch, B, True, dict(gptr=gp, status=np.array([0])))
    gp2 = gp.copy()
    gp2[3] = gp[2]                                              # an empty graph in the middle left at its predecessor's start
    assert C.judge_graph_ptr(batch, B, True, dict(gptr=gp2, status=np.array([0])))
    assert C.judge_graph_ptr(*C.GRAPH_PTR_CASES["unsorted"], dict(gptr=gp, status=np.array([0])))
