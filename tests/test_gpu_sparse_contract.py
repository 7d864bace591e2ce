"""The node-level sparse kernels of csrc/engine_kernels.hpp one by one -- k_espmm in its six kinds at all four lane-group
widths (24 instantiations), k_edge_att_deg, k_pool2 / k_pool2_sum, k_pool_cnt -- through the test hooks cal_sparse_probe_*
(end of csrc/engine.hip), against the float64 restatement in tests/sparse_contract_ref.py (itself tied to the oracle and to
torch autograd by tests/test_sparse_contract_ref.py).

Every case: outputs NaN-filled before the launch, a canary block behind EVERY buffer (inputs included), operands from a seeded
generator, CSR arrays built here with numpy (stable sort by key, self loops dropped: the plan kernels are not judged).  The
per-edge weights of edges WITHOUT a slot (input self loops) are NaN: a kernel that reads them poisons its output.

Inputs.  The degree-ladder batch of tests/ladder.py (N = 301, three block-diagonal graphs, ~4.5 k edges): graph 0 has 256 nodes, node v has
exactly ladder[v] slots over distinct neighbours in the view under test -- every count 0..72, then 127..129 and 191..193, the
rest 1..6 -- so that for SPLIT = 64 / G = 1, 2, 4, 8 there is a full batch of 8 SPLIT, the batch below it, `case 8` of the
remainder switch, one and two slots over a batch, an empty row, and rows of two, three and four 64-slot rounds; graph 1 has 5
nodes and no edge; graph 2 is a 40-node random graph with one directed edge; five input self loops.  Two such batches: one
with the ladder on the by-destination view (forward kinds), one on the by-source view (SDDMM kinds, edge attention).  N = 301
is a multiple of neither 4 nor 32: 76 row blocks at rpb = 4 (72 remapped, 4 identity), 10 at rpb = 32 (8 + 2).

Bounds, u = 2^-24; none of them fitted to a kernel's output:

  out       an fp32 sum of n = deg + 1 terms in any order is off by at most (n - 1) u times the sum of absolute terms; every
            coefficient carries at most three more roundings (dis * w, the loop coefficient dis * loop_w, the final scale by
            dis) and the bias add is one more: deg + 4.  The bound allows deg + 6, which also covers a product that the
            compiler does not fuse into its add and the separate multiply of the loop term:
            |got - ref| <= (deg + 6) u T (1 + 1e-3), T = dis_i (sum |coef| |row| + dis_i loop_w |row_i|) + |bias| in fp64,
            the last factor for the second-order terms.  ReLU needs no exclusions: |relu(a) - relu(b)| <= |a - b|.
  gn, gself an fp32 dot of H products in any order: (H + 1) u sum_k |a_k b_k|.
  st        the column sums are compared with fp64 sums over the kernel's OWN stored out, so the aggregation's rounding does
            not enter: v and v^2 are exact in fp64, the only error is the order of n fp64 additions, n 2^-52 S (S = sum |v|
            or sum v^2, n = N rows; tests/test_gpu_gemm_contract.py has the derivation).  Atomic mode adds onto a non-zero
            starting value: n + 1 terms and S + |s0|.
  pooled    an fp32 sum of the n rows of a graph in any order (row slices included): (n - 1) u sum |x|.  One row: exact.
  counts    exact.
  att       a_k = e_k / (e_0 + e_1), e_k = expf(l_k - max l), l_k = fedge ((p_k + q_k) + b_k).  The logit carries three
            roundings (two adds, the scale): |dl_k| <= 3 u L_k, L_k = |p_k| + |q_k| + |b_k|; the subtraction one more, and one
            of the two arguments is exactly 0: the other is off by d = 3 u (L_0 + L_1) + u |l_0 - l_1|, which moves its
            exponential by the relative amount d; expf adds its own relative error x.  So e_k is off by h = d + x
            relatively, e_0 + e_1 by at most h + u, its reciprocal by h + 2 u, the product by 2 h + 3 u:
            |got - ref| <= ref (2 h + 3 u) (1 + 1e-3).  x: no ROCm device-library documentation of expf's error is installed
            with the toolchain, so x is MEASURED in the test's setup: the largest relative error of the device's fp32 exp
            against fp64 exp on 2^20 points of the range of the arguments, and not less than one ulp (2 u).  With
            fedge = 0 both logits are exactly 0 and both rows exactly 0.5.
  dis       against (loop_w + sum of the kernel's OWN stored att over the slots) ** -0.5 in fp64, so the softmax error does
            not enter twice: an fp32 sum of deg + 1 terms, the power halves it, eight roundings of slack and two for the
            square root and the reciprocal: relative (deg + 8) u + 2 u.  att itself is held to the reference above.

Worst printed ratios on MI355X (this commit) are recorded per test in the docstrings below.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import sparse_contract_ref as ref
from tests.helpers import Buf, pool_intact
from tests.ladder import LADDER, N, N0, N1, ladder_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24, U52 = 2.0 ** -24, 2.0 ** -52
NAN = float("nan")
F64 = torch.float64

KINDS = ["plain", "st", "wt", "wt_st", "wt_sd", "wt_sd_pb"]
WIDTHS = [4, 20, 32, 36, 64, 100, 128, 132, 200, 256]


def group_of(H):
    """lanes per row (with_g of csrc/engine.hip)"""
    g = 8
    while g * 4 < H and g < 64:
        g *= 2
    return g


@pytest.mark.parametrize("key", [1, 0])
def test_ladder_holds_in_the_view_under_test(key):
    b = ladder_batch(key)
    rows = np.diff(b["ptr"])
    assert np.array_equal(rows, b["deg"]) and np.array_equal(rows[:N0], b["deg0"])
    assert set(LADDER) <= set(rows[:N0].tolist()) and rows[:N0].max() == 193 and (rows[N0:N0 + N1] == 0).all()
    assert N == 301 and b["E"] < 10000 and int((~b["slotted"]).sum()) == 5 and b["ptr"][-1] == b["E"] - 5
    for v in range(N):                                          # distinct neighbours inside the row's own graph
        nb = b["nbr"][b["ptr"][v]:b["ptr"][v + 1]]
        assert len(set(nb.tolist())) == len(nb) and (b["batch"][nb] == b["batch"][v]).all()
    for G in (8, 16, 32, 64):                                   # what the ladder is for, per SPLIT = 64 / G
        sp = 64 // G
        for cnt in (8 * sp, 8 * sp - 1, 8 * sp + 1, 8 * sp + 2, 0, 128, 129, 192, 193):
            assert cnt in rows[:N0]
        if sp > 1:                                              # `case 8` of the remainder switch: 7 SPLIT < cnt - q < 8 SPLIT
            assert any(7 * sp < c % (8 * sp) < 8 * sp for c in rows[:N0] if c <= 64)


def _dev_csr(pool, b):
    return [Buf(pool, len(b[k]), torch.int32, data=torch.from_numpy(b[k])) for k in ("ptr", "nbr", "eid")]


# ---- k_espmm -------------------------------------------------------------------------------------------------------------
def espmm_axes(kind, H, j):
    """the launch parameters of variant j (0..2) of (kind, H): every value of every axis occurs within ONE (kind, width)"""
    ki, wi = KINDS.index(kind), WIDTHS.index(H)
    return {"nbranch": 1 + (j + ki) % 2, "relu": ((j + 1) // 2 + wi) % 2, "bias": (j + wi + ki) % 2,
            "loop_w": 1.0 + (j // 2 + wi) % 2, "rpb": (256 // group_of(H)) * (1, 2, 8)[(j + wi) % 3],
            "st": "atomic" if ((j + 1) // 2 + ki) % 2 == 0 else "parts"}


def test_cases_reach_all_24_instantiations_with_every_axis_value():
    pairs = {(k, group_of(H)) for k in KINDS for H in WIDTHS}
    assert pairs == {(k, G) for k in KINDS for G in (8, 16, 32, 64)} and len(pairs) == 24
    for k in KINDS:
        for G in (8, 16, 32, 64):
            ws = [H for H in WIDTHS if group_of(H) == G]
            assert any(H == 4 * G for H in ws) and any(H < 4 * G for H in ws)       # one fills the group, one leaves lanes idle
            ax = [espmm_axes(k, H, j) for H in ws for j in range(3)]
            base = 256 // G
            for name, vals in (("nbranch", {1, 2}), ("relu", {0, 1}), ("bias", {0, 1}), ("loop_w", {1.0, 2.0}),
                               ("rpb", {base, 2 * base, 8 * base}), ("st", {"atomic", "parts"})):
                assert {a[name] for a in ax} == vals, (k, G, name)


class Branch:
    """operands, outputs and float64 reference of one SpmmBranch"""

    def __init__(self, pool, g, b, kind, H, ax):
        E = b["E"]
        self.b, self.kind, self.H, self.ax = b, kind, H, ax
        wt, self.stt, self.sd, self.pb = kind != "plain" and kind != "st", kind in ("st", "wt_st"), "sd" in kind, "pb" in kind
        h = torch.randn(N, H, generator=g)
        if self.pb:                                             # an activation: half of it exactly 0.0, some of that -0.0
            h = torch.relu(h)
            h[(torch.rand(N, H, generator=g) < 0.1) & (h == 0)] = -0.0
        w = (0.05 + 0.95 * torch.rand(E, generator=g)) if wt else None
        wsl = (w.double() if wt else torch.ones(E, dtype=F64))[torch.from_numpy(b["eid"]).long()]
        deg = torch.full((N,), ax["loop_w"], dtype=F64).index_add_(0, ref.slot_rows(b["ptr"]), wsl)
        dis = (deg ** -0.5).float()                             # the true deg^-1/2 of the (weighted) view
        bias = torch.randn(H, generator=g) if ax["bias"] else None
        gp = torch.randn(3, H, generator=g) if self.pb else None
        z = torch.randn(N, H, generator=g) if self.sd else None
        d = lambda t: None if t is None else t.to(DEV)           # the float64 reference runs on the GPU: a few ms per launch
        rows = ref.feature_rows(d(h), d(gp), b["batch"] if self.pb else None)
        self.want, self.T, self.n = ref.aggregate(b["ptr"], b["nbr"], b["eid"], rows, d(dis), d(w), ax["loop_w"], d(bias), ax["relu"])
        pv, iv = [0] * 14, [0, 0]
        self.out = Buf(pool, N * H, fill=NAN)
        pv[0], pv[1], pv[4] = Buf(pool, N * H, data=h).ptr(), self.out.ptr(), Buf(pool, N, data=dis).ptr()
        if bias is not None:
            pv[2] = Buf(pool, H, data=bias).ptr()
        if wt:
            wd = w.clone()
            wd[torch.from_numpy(~b["slotted"])] = NAN           # never read: these edges have no slot
            pv[3] = Buf(pool, E, data=wd).ptr()
        if self.stt:
            gen = torch.Generator().manual_seed(99)
            self.s0 = [torch.randn(H, generator=gen).double() for _ in range(2)]
            self.acc = [Buf(pool, H, F64, data=s) for s in self.s0]
            pv[5], pv[7] = self.acc[0].ptr(), self.acc[1].ptr()
            if ax["st"] == "parts":
                self.P, self.stride = -(-N // ax["rpb"]), H + 4
                self.parts = [Buf(pool, self.P * self.stride, F64, fill=NAN) for _ in range(2)]
                pv[6], pv[8] = self.parts[0].ptr(), self.parts[1].ptr()
                iv = [self.stride, self.stride]
        if self.sd:
            self.gn, self.gself = Buf(pool, E, fill=NAN), Buf(pool, N, fill=NAN)
            pv[9], pv[10], pv[11] = Buf(pool, N * H, data=z).ptr(), self.gn.ptr(), self.gself.ptr()
            self.sd_want = ref.sddmm(b["ptr"], b["nbr"], b["eid"], rows, d(z), E)
        if self.pb:
            pv[12], pv[13] = Buf(pool, 3 * H, data=gp).ptr(), Buf(pool, N, torch.int64, data=torch.from_numpy(b["batch"])).ptr()
        self.pv, self.iv = pv, iv

    def untouched(self):
        ok = bool(torch.isnan(self.out.t).all())
        if self.sd:
            ok = ok and bool(torch.isnan(self.gn.t).all()) and bool(torch.isnan(self.gself.t).all())
        if self.stt:
            ok = ok and all(torch.equal(a.t.cpu(), s) for a, s in zip(self.acc, self.s0))
        return ok

    def check(self, fails, rat, tag):
        H = self.H
        got = self.out.t.view(N, H).double()
        if not bool(torch.isfinite(got).all()):
            fails.append("%s: %d entries of out were never written (or poisoned)" % (tag, int((~torch.isfinite(got)).sum())))
            return
        _ratio(got, self.want, (self.n + 5).double()[:, None] * U24 * self.T * (1 + 1e-3), "out", fails, rat, tag)
        if self.sd:
            gn, gself = self.gn.t.double(), self.gself.t.double()
            wn, ws, mn, ms = self.sd_want
            sl = torch.from_numpy(self.b["slotted"]).to(DEV)
            if not bool(torch.isnan(gn[~sl]).all()):
                fails.append(tag + ": gn of an edge without a slot was written")
            if not (bool(torch.isfinite(gn[sl]).all()) and bool(torch.isfinite(gself).all())):
                fails.append(tag + ": gn / gself hold entries the kernel never wrote")
            else:
                _ratio(gn[sl], wn[sl], (H + 1) * U24 * mn[sl], "gn", fails, rat, tag)
                _ratio(gself, ws, (H + 1) * U24 * ms, "gself", fails, rat, tag)
        if self.stt:
            s, q, a = ref.col_stats(got)
            acc = [x.t for x in self.acc]
            s0 = [x.to(DEV) for x in self.s0]
            if self.ax["st"] == "parts":
                parts = [p.t.view(self.P, self.stride) for p in self.parts]
                if not all(bool(torch.isfinite(p[:, :H]).all()) for p in parts):
                    fails.append(tag + ": partial rows were not all written")
                    return
                if not all(bool(torch.isnan(p[:, H:]).all()) for p in parts):
                    fails.append(tag + ": the padding of the partial rows was written")
                if not all(torch.equal(x, y) for x, y in zip(acc, s0)):
                    fails.append(tag + ": parts mode also added into the accumulators")
                gs, gq, start, terms = parts[0][:, :H].sum(0), parts[1][:, :H].sum(0), [0.0, 0.0], N
            else:
                gs, gq, start, terms = acc[0] - s0[0], acc[1] - s0[1], [x.abs() for x in s0], N + 1
            _ratio(gs, s, terms * U52 * (a + start[0]), "st_sum", fails, rat, tag)
            _ratio(gq, q, terms * U52 * (q + start[1]), "st_sq", fails, rat, tag)


def _ratio(got, want, bound, name, fails, rat, tag):
    err = (got - want).abs()
    bad = err > bound
    r = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    rat[name] = max(rat.get(name, 0.0), r)
    if bool(bad.any()):
        fails.append("%s: %s err/bound %.3e (%d entries over, largest error %.3e)" % (tag, name, r, int(bad.sum()), float(err.max())))


def _probe_espmm(csr, b, branches, nbranch, relu, loop_w, H, rpb, n_rows=N):
    from cal_amd import _lib
    from cal_amd.plan import _stream
    iv = [int(b["ptr"][-1]), nbranch, relu, n_rows, H, rpb]
    pv = [c.ptr() for c in csr]
    for br in branches:
        iv += br.iv
        pv += br.pv
    h = _lib.lib()
    rc = h.cal_sparse_probe_espmm((ctypes.c_int64 * len(iv))(*iv), (ctypes.c_void_p * len(pv))(*pv), (ctypes.c_double * 1)(loop_w), _stream())
    torch.cuda.synchronize()
    return rc, (h.cal_last_error().decode() if rc else "")


def _report(name, rat, fails):
    print("%s  %s" % (name, "  ".join("%s=%.3e" % kv for kv in sorted(rat.items()))))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_espmm(kind, H):
    """k_espmm<4, G, ...> of one kind at one width: three launches that cover one / two branches, relu, bias, loop_w, the three
    rows-per-block and both statistics modes (espmm_axes).
    Worst on MI355X over the 60 cases (err / bound, bound 1): out 0.40 (per kind: plain 0.36, st 0.36, wt 0.40, wt_st 0.39,
    wt_sd 0.38, wt_sd_pb 0.35), gn 0.45, gself 0.37, st_sum 0 (exact), st_sq 1.2e-2."""
    b = ladder_batch(0 if "sd" in kind else 1)
    fails, rat = [], {}
    for j in range(3):
        ax = espmm_axes(kind, H, j)
        pool = []
        csr = _dev_csr(pool, b)
        g = torch.Generator().manual_seed(7000 + 100 * KINDS.index(kind) + 10 * WIDTHS.index(H) + j)
        brs = [Branch(pool, g, b, kind, H, ax) for _ in range(ax["nbranch"])]
        tag = "%s H=%d G=%d %s" % (kind, H, group_of(H), " ".join("%s=%s" % kv for kv in ax.items()))
        rc, msg = _probe_espmm(csr, b, brs, ax["nbranch"], ax["relu"], ax["loop_w"], H, ax["rpb"])
        if rc:
            fails.append("%s: rc %d %s" % (tag, rc, msg))
            continue
        for k, br in enumerate(brs):
            br.check(fails, rat, "%s b%d" % (tag, k))
        if not pool_intact(pool):
            fails.append(tag + ": a canary behind a buffer was overwritten")
            break
    _report("k_espmm %s H=%d" % (kind, H), rat, fails)


def _refused(kind, H, rpb, name, second_kind=None, mutate=None):
    b = ladder_batch(0 if "sd" in kind else 1)
    pool = []
    csr = _dev_csr(pool, b)
    g = torch.Generator().manual_seed(7900)
    ax = {"nbranch": 2 if second_kind else 1, "relu": 0, "bias": 1, "loop_w": 1.0, "rpb": rpb, "st": "atomic"}
    Hd = H if H % 4 == 0 and H <= 256 else 8                    # the buffers of a width that is refused anyway
    brs = [Branch(pool, g, b, k, Hd, ax) for k in ([kind, second_kind] if second_kind else [kind])]
    if mutate:
        mutate(brs)
    rc, msg = _probe_espmm(csr, b, brs, ax["nbranch"], 0, 1.0, H, rpb)
    print("%s  rc=%d %s" % (name, rc, msg))
    assert rc == 2 and msg, (name, rc, msg)
    assert all(br.untouched() for br in brs), name + ": something was launched"
    assert pool_intact(pool)


def test_espmm_refusals():
    """no launch, return code 2 and a message: widths the engine does not accept, rows per block that are no multiple of
    the four waves, branches of different kind, the SDDMM without weights and with statistics"""
    _refused("wt", 260, 4, "H = 260")
    _refused("wt", 6, 32, "H = 6")
    _refused("wt", 64, 6, "rpb = 6")
    _refused("wt", 64, 16, "branches of different kind (weights)", second_kind="plain")
    _refused("wt_st", 64, 16, "branches of different kind (statistics)", second_kind="wt")
    _refused("wt_sd_pb", 64, 16, "branches of different kind (pool backward)", second_kind="wt_sd")

    def no_weights(brs):
        brs[0].pv[3] = 0
    _refused("wt_sd", 64, 16, "SD without weights", mutate=no_weights)

    def with_stats(brs):
        pool = []
        brs[0].keep = [Buf(pool, 64, F64, fill=0.0) for _ in range(2)]
        brs[0].pv[5], brs[0].pv[7] = brs[0].keep[0].ptr(), brs[0].keep[1].ptr()
    _refused("wt_sd", 64, 16, "SD with statistics", mutate=with_stats)


# ---- k_edge_att_deg ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_exp_error(lo):
    """largest relative error of the device's fp32 exp on [lo, 0] against fp64 (module docstring, `att`); at least one ulp"""
    x = torch.linspace(lo, 0.0, 1 << 20, device=DEV, dtype=torch.float32)
    want = torch.exp(x.double())
    return max(float(((torch.exp(x).double() - want).abs() / want).max()), 2 * U24)


@pytest.mark.parametrize("loop_w", [1.0, 2.0])
@pytest.mark.parametrize("fedge", [1.0, 0.0])
def test_edge_attention_and_degrees(fedge, loop_w):
    """k_edge_att_deg on the by-source ladder batch.  Worst on MI355X (err / bound, bound 1): att 0.21, dis 0.15; the measured
    relative error of the device's fp32 exp stayed under the one-ulp floor (x = 2 u = 1.19e-7)."""
    from cal_amd import _lib
    from cal_amd.plan import _stream
    b = ladder_batch(0)
    E = b["E"]
    pool, fails, rat = [], [], {}
    csr = _dev_csr(pool, b)
    g = torch.Generator().manual_seed(8000)
    pq, be = torch.randn(N, 4, generator=g) * 1.5, torch.randn(2, generator=g)
    att, dis_c, dis_o = Buf(pool, 2 * E, fill=NAN), Buf(pool, N, fill=NAN), Buf(pool, N, fill=NAN)
    dpq, dbe = Buf(pool, 4 * N, data=pq), Buf(pool, 2, data=be)
    _lib.call("cal_sparse_probe_edge_att", csr[0].ptr(), csr[1].ptr(), csr[2].ptr(), int(b["ptr"][-1]), dpq.ptr(), dbe.ptr(), att.ptr(),
              dis_c.ptr(), dis_o.ptr(), loop_w, N, E, fedge, _stream())
    torch.cuda.synchronize()
    pq, be = pq.to(DEV), be.to(DEV)
    want, _, _, logits = ref.edge_attention(b["ptr"], b["nbr"], b["eid"], pq, be, fedge, loop_w, E)
    got = att.t.view(2, E).double()
    sl = torch.from_numpy(b["slotted"]).to(DEV)
    assert bool(torch.isnan(got[:, ~sl]).all()), "att of an input self loop was written"
    assert bool(torch.isfinite(got[:, sl]).all()), "att of a slotted edge was never written"
    ed = torch.from_numpy(b["eid"]).long().to(DEV)
    if fedge == 0.0:
        assert bool((got[:, sl] == 0.5).all())
    else:
        ri, nb = ref.slot_rows(b["ptr"], DEV), torch.from_numpy(b["nbr"]).long().to(DEV)
        L = pq.double()[ri, 0:2].abs() + pq.double()[nb, 2:4].abs() + be.double().abs()
        gap = (logits[:, 0] - logits[:, 1]).abs()
        x = _device_exp_error(-float(gap.max()) - 1.0)
        h = 3 * U24 * L.sum(1) + U24 * gap + x
        bound = want[:, ed] * (2 * h + 3 * U24) * (1 + 1e-3)
        _ratio(got[:, ed], want[:, ed], bound, "att", fails, rat, "att")
        rat["expf_rel"] = x
    # degrees: fp64 over the kernel's own stored att
    ri = ref.slot_rows(b["ptr"], DEV)
    deg = torch.full((2, N), loop_w, dtype=F64, device=DEV).index_add_(1, ri, got[:, ed].contiguous())
    dwant = deg ** -0.5
    slots = torch.from_numpy(np.diff(b["ptr"]).astype(np.float64)).to(DEV)
    for k, d in enumerate((dis_c, dis_o)):
        _ratio(d.t.double(), dwant[k], dwant[k] * (slots + 10) * U24, "dis", fails, rat, "dis[%d]" % k)
    if not pool_intact(pool):
        fails.append("a canary behind a buffer was overwritten")
    _report("k_edge_att_deg fedge=%g loop_w=%g" % (fedge, loop_w), rat, fails)


# ---- k_pool2 / k_pool2_sum / k_pool_cnt ----------------------------------------------------------------------------------
def _activations(g, n, H):
    """two ReLU outputs: half of the entries exactly 0.0, some of them -0.0"""
    h = torch.relu(torch.randn(2, n, H, generator=g))
    h[(torch.rand(2, n, H, generator=g) < 0.1) & (h == 0)] = -0.0
    return h


def _probe_pool(sel, hc, ho, gptr, batch, pooled, cnt, slices, n, B, H, rpb_n=32):
    from cal_amd import _lib
    from cal_amd.plan import _stream
    S = (ctypes.c_int64 * 1)(-1)
    p = lambda x: x.ptr() if x is not None else None
    _lib.call("cal_sparse_probe_pool", sel, p(hc), p(ho), p(gptr), p(batch), p(pooled), p(cnt), p(slices), n, B, H, rpb_n, S, _stream())
    torch.cuda.synchronize()
    return int(S[0])


def _pool_case(sizes, H, want_S, seed, fails, rat):
    B, n = len(sizes), int(sum(sizes))
    gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    g = torch.Generator().manual_seed(seed)
    h = _activations(g, n, H)
    S = _probe_pool(3, None, None, None, None, None, None, None, n, B, H)
    assert S == want_S, ("slices", sizes, S, want_S)
    for sel in (0, 1):
        pool = []
        hc, ho = Buf(pool, n * H, data=h[0]), Buf(pool, n * H, data=h[1])
        dg = Buf(pool, B + 1, torch.int32, data=torch.from_numpy(gptr))
        pooled, cnt = Buf(pool, 2 * B * H, fill=NAN), Buf(pool, 2 * B * H, fill=NAN)
        slices = Buf(pool, S * 4 * B * H, fill=NAN) if S > 1 else None
        assert _probe_pool(sel, hc, ho, dg, None, pooled, cnt, slices, n, B, H) == S
        tag = "sizes=%s H=%d S=%d sel=%d" % (sizes, H, S, sel)
        gp, gc = pooled.t.view(2, B, H).double(), cnt.t.view(2, B, H).double()
        for k, hk in enumerate((hc, ho)):
            s, mag, c, rows = ref.pool(hk.t.view(n, H), gptr)
            if not bool(torch.isfinite(gp[k]).all()):
                fails.append(tag + ": pooled rows were never written")
                continue
            _ratio(gp[k], s, (rows - 1).clamp_min(0).double()[:, None] * U24 * mag, "pooled", fails, rat, tag)
            if sel == 0 and not torch.equal(gc[k], c):
                fails.append("%s: counts differ in %d places" % (tag, int((gc[k] != c).sum())))
        if sel == 1 and not bool(torch.isnan(gc).all()):
            fails.append(tag + ": counts were written without a count buffer")
        if not pool_intact(pool):
            fails.append(tag + ": a canary behind a buffer was overwritten")


@pytest.mark.parametrize("H", WIDTHS)
def test_pool_unsliced(H):
    """k_pool2<4>, one workgroup per (graph, branch): graph sizes around nrl = 256 / tc and 2 nrl rows, with and without counts.
    Worst on MI355X (err / bound, bound 1): pooled 0.88 (H = 200: graphs of 3 to 9 rows, where the bound is two to eight
    roundings), counts exact."""
    tc = min(256, 1 << max(0, (H // 4 - 1).bit_length()))
    nrl = 256 // tc
    sizes = [nrl - 1, 0, 1, 2 * nrl + 1, nrl, nrl + 1, 2 * nrl - 1, 2 * nrl]
    while sum(sizes) >= 2 * 128 * len(sizes):                   # keep S = N / (128 B) at 1
        sizes.append(1)
    assert (H, nrl) in {(4, 256), (20, 32), (32, 32), (36, 16), (64, 16), (100, 8), (128, 8), (132, 4), (200, 4), (256, 4)}
    assert H != 4 or max(sizes) == 513
    fails, rat = [], {}
    _pool_case(sizes, H, 1, 8100 + H, fails, rat)
    _report("k_pool2 H=%d" % H, rat, fails)


@pytest.mark.parametrize("H", [4, 36, 132, 256])
def test_pool_row_slices(H):
    """k_pool2<4> over S = 2 and 3 row slices + k_pool2_sum: a graph without rows, lengths that S does not divide.
    Worst on MI355X (err / bound, bound 1): pooled 1.8e-2, counts exact."""
    fails, rat = [], {}
    for sizes, S in (([0, 600], 2), ([299, 301], 2), ([400], 3), ([401, 0, 500], 2)):
        _pool_case(sizes, H, S, 8200 + H, fails, rat)
    _report("k_pool2 sliced H=%d" % H, rat, fails)


@pytest.mark.parametrize("H", WIDTHS)
def test_pool_counts_from_the_batch_vector(H):
    """k_pool_cnt<4, G>: empty graphs in the middle, graph boundaries inside a row block, a ragged last block.  Exact."""
    sizes = [5, 0, 0, 37, 1, 0, 64, 30, 3, 0]
    B, n = len(sizes), sum(sizes)
    batch = np.repeat(np.arange(B), sizes).astype(np.int64)
    g = torch.Generator().manual_seed(8300 + H)
    h = _activations(g, n, H)
    for rpb_n in (32, 40):
        pool = []
        hc, ho = Buf(pool, n * H, data=h[0]), Buf(pool, n * H, data=h[1])
        db = Buf(pool, n, torch.int64, data=torch.from_numpy(batch))
        cnt = Buf(pool, 2 * B * H, fill=NAN)
        _probe_pool(2, hc, ho, None, db, None, cnt, None, n, B, H, rpb_n)
        got = cnt.t.view(2, B, H).double()
        for k, hk in enumerate((hc, ho)):
            assert torch.equal(got[k], ref.pool_counts(hk.t.view(n, H), batch, B)), (H, rpb_n, k)
        assert pool_intact(pool)
