"""tests/gat_contract_ref.py tied to what the project already trusts -- oracle.cal_oracle.gat_conv in float64, torch autograd
through it, libcalhost's cal_gat_dropout_mask -- and the condition that keeps tests/test_gpu_gat_contract.py from being
vacuous: on the inputs and with the bounds that file uses (tests/gat_contract_cases.py, Judge), ten seeded defects of the
reference each exceed a bound.  The case table's path expectations are checked here against the restated dispatch rule.
CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests import gat_contract_cases as C
from tests import gat_contract_ref as ref
from tests import sparse_contract_ref as sref
from tests.ladder import N, ladder_batch
from tests.test_sparse_contract_ref import _graph

F64 = torch.float64
TOL = dict(rtol=1e-11, atol=1e-12)
SEED = 0x5EED0000BEEF0001


def _oracle_mask(ei, full, E):
    """[(E + N), K] by slot id -> the oracle's order: the edges that are no self loops in input order, then the N loops"""
    keep_e = np.nonzero(ei[0] != ei[1])[0]
    return torch.cat([torch.from_numpy(full[keep_e]), torch.from_numpy(full[E:])], 0)


@pytest.mark.parametrize("K,D,p,relu,slope", [(3, 4, 0.0, 0, 0.2), (2, 5, 0.4, 1, 0.2), (1, 8, 0.3, 0, 0.0), (4, 2, 0.5, 1, 0.1)])
def test_forward_and_backward_are_the_oracle_gat_conv_and_its_autograd(K, D, p, relu, slope):
    """explicit self loops (one twice), a directed edge, a pinned keep mask, ReLU; both CSR views give the same answer"""
    ei, _, n, g = _graph(11)
    E, H = ei.shape[1], K * D
    z = torch.randn(n, H, generator=g, dtype=F64, requires_grad=True)
    att = (torch.randn(1, K, 2 * D, generator=g, dtype=F64) * 0.8).requires_grad_(True)
    bias = torch.randn(H, generator=g, dtype=F64, requires_grad=True)
    gout = torch.randn(n, H, generator=g, dtype=F64)
    full = ref.keep_mask(SEED, E, n, K, p)
    assert p == 0 or 0.2 < float(1 - full.mean()) < 0.8
    want = O.gat_conv(z, torch.from_numpy(ei), torch.eye(H, dtype=F64), att, bias, K, slope, p, p > 0, _oracle_mask(ei, full, E))
    want = torch.relu(want) if relu else want
    ptr, nbr, eid = sref.csr_view(ei, n, 1)
    assert ptr[-1] == E - 3                                      # the three input self loops have no slot
    f = ref.forward(ptr, nbr, eid, z.detach(), att.detach()[0], bias.detach(), relu, slope, p, full, K, D, E)
    assert torch.allclose(f.out, want.detach(), **TOL)
    assert bool((f.T >= f.pre.abs() - 1e-12).all()) and bool((f.den >= 1).all())
    loops = ei[0] == ei[1]
    assert bool(torch.isnan(f.alpha[:E][loops]).all()) and bool(torch.isfinite(f.alpha[:E][~loops]).all())
    rowsum = f.alpha[E:] + torch.zeros(n, K, dtype=F64).index_add_(0, sref.slot_rows(ptr), f.alpha[torch.from_numpy(eid).long()])
    assert torch.allclose(rowsum, torch.ones_like(rowsum), **TOL)
    (want * gout).sum().backward()
    gm = gout * (want.detach() > 0) if relu else gout            # the kernels take the gradient already masked by the ReLU
    b = ref.backward(ptr, nbr, eid, z.detach(), att.detach()[0], f.adst, f.asrc, f.mx, f.den, gm, slope, p, full, K, D, E)
    assert torch.allclose(b.dz, z.grad, **TOL) and torch.allclose(b.datt, att.grad[0], **TOL) and torch.allclose(b.dbias, bias.grad, **TOL)
    assert bool(torch.isnan(b.draw[:E][loops]).all()) and bool(torch.isfinite(b.draw[:E][~loops]).all())


@pytest.mark.parametrize("seed", [0, 77, 0xDEADBEEF12345678, (1 << 64) - 1, ref.step_seed(77, 5), ref.step_seed((1 << 64) - 3, 1 << 40)])
def test_keep_mask_is_the_host_library_mask_bit_for_bit(seed):
    from cal_amd import _lib
    h = _lib.host_lib()
    assert ref.step_seed(1, 2) == (1 + 2 * 0x9E3779B97F4A7C15) % (1 << 64) and ref.step_seed(5, 0) == 5 and ref.step_seed((1 << 64) - 1, 1) == 0x9E3779B97F4A7C14
    for K, p, E, n in ((1, 0.3, 50, 7), (4, 0.3, 4467, 301), (7, 0.5, 13, 30), (4, 0.0, 20, 5), (40, 0.9, 100, 11), (3, 0.01, 1, 0)):
        got = np.full((E + n, K), -1.0, np.float32)
        rc = h.cal_gat_dropout_mask(ctypes.c_uint64(seed), E, n, K, ctypes.c_float(p), got.ctypes.data_as(ctypes.c_void_p), None)
        assert rc == 0
        mine = ref.keep_mask(seed, E, n, K, p)
        assert mine.dtype == np.float32 and np.array_equal(mine, got), (seed, K, p)
        if p > 0 and mine.size > 500:
            assert abs(float(1 - mine.mean()) - p) < 0.05


def test_case_table_reaches_every_path_with_every_axis_value():
    """the family every case is meant for is what the restated dispatch rule gives, and together the cases run every LH of the
    fused forward, every G of both layouts in the forward and both backwards, both d att partial kernels and the wave family"""
    fwd, bwd = {}, {}
    for c in C.CASES + C.WIDE:
        fam, v, G, LH = C.fwd_path(c["K"], c["D"], c["mis"], bool(c["bias"]))
        assert (fam, v) == C.FWD_FAMILY[c["fwd"]], c["name"]
        bf, bv, bG, datt = C.bwd_path(c["K"], c["D"], c["mis"])
        assert bf == C.BWD_FAMILY[c["bwd"]][0] and (bf == "refuse" or bv == C.BWD_FAMILY[c["bwd"]][1]), c["name"]
        assert "bias" not in c["mis"] or c["bias"]
        fwd.setdefault(c["fwd"], []).append((c, G, LH))
        bwd.setdefault(c["bwd"], []).append((c, bG, datt))
    assert {LH for _, _, LH in fwd["fused"]} == {1, 2, 4, 8, 16, 32, 64}
    fu = [(c["K"] * c["D"] // 4, G, LH) for c, G, LH in fwd["fused"]]
    assert any(G == LH for _, G, LH in fu) and any(G > LH for _, G, LH in fu)
    assert any(h < G and h & (h - 1) for h, G, _ in fu)                       # idle lanes in the row group
    assert any(h == 96 for h, G, _ in fu) and any(h == 128 for h, G, _ in fu)   # one and a half and two column passes of G = 64
    for name in ("fused", "twopass1"):
        assert {G for _, G, _ in fwd[name]} == {8, 16, 32, 64}, name
    assert {G for _, G, _ in fwd["twopass4"]} == {8, 16, 32, 64}
    for name in ("rows4", "rows1"):
        assert {G for _, G, _ in bwd[name]} == {8, 16, 32, 64}, name
    datts = {d for k in ("wave", "rows4", "rows1") for _, _, d in bwd[k]}
    assert "part_w" in datts and "part256" in datts and any(d in ("part64", "part128", "part192") for d in datts)
    assert any(c["mis"] == {"ws"} and d == "part256" for c, _, d in bwd["rows4"])   # K = 4, D = 64 on the generic partial kernel
    for fam, members in list(fwd.items()) + [(k, v) for k, v in bwd.items() if k != "refuse"]:
        cs = [c for c, _, _ in members]
        for axis, vals in (("p", {0.0, 0.3}), ("relu", {0, 1}), ("bias", {0, 1}), ("slope", {0.2, 0.0})):
            assert {c[axis] for c in cs} == vals, (fam, axis)
    assert all(any(c["asc"] for c, _, _ in fwd[k]) for k in ("wave", "fused", "twopass1"))
    assert len({c["name"] for c in C.CASES + C.WIDE}) == len(C.CASES + C.WIDE)


@pytest.mark.parametrize("key", [1, 0])
def test_ladder_holds_what_the_gat_kernels_need(key):
    """slot counts (edges + the node's own loop) at every boundary of the GAT kernels: the register cache of eight and its halves of
    four, the batches of four and eight, the 16-slot hash groups and (head, slot) layout, the 64-slot chunks and the two-sweep path"""
    rows = np.diff(ladder_batch(key)["ptr"])
    assert set(rows.tolist()) >= {c - 1 for c in (1, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129)}
    assert {int(c) % 8 for c in rows + 1} >= set(range(1, 8)) and {int(c) % 8 for c in rows} >= set(range(1, 8))
    assert N == 301 and -(-N // 4) == 76 and 8 * (76 // 8) == 72 and -(-N // 32) == 10 and N % 32 != 0
    b = C.sorted_rows(key)
    ptr, nbr, _ = b["dst"]
    assert all((np.diff(nbr[ptr[v]:ptr[v + 1]]) > 0).all() for v in range(N))


# ---- sensitivity: the bounds notice seeded defects ---------------------------------------------------------------------------
def _csr_keep_loops(ei, n, key):
    order = np.argsort(ei[key], kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, ei[key] + 1, 1)
    return np.cumsum(ptr).astype(np.int32), ei[1 - key][order].astype(np.int32), order.astype(np.int32)


class _Setup:
    def __init__(self, name):
        c = self.c = C.case_by_name(name)
        b = self.b = C.batch_of(c, 1)
        o = self.o = C.operands(c, 1)
        K, D, E = c["K"], c["D"], b["E"]
        self.keep = ref.keep_mask(SEED, E, N, K, c["p"])
        self.J = ref.Judge(*b["dst"], o["z"], o["att"], o["bias"], c["relu"], c["slope"], c["p"], self.keep, K, D, E, 2 * ref.U)
        f = self.J.f
        self.state = tuple(t.float() for t in (f.adst, f.asrc, f.mx, f.den))
        rb = self.rb = self.J.reference_backward(*self.state, o["gout"])
        self.good = dict(out=f.out, adst=f.adst, asrc=f.asrc, mx=f.mx, den=f.den, draw=rb.draw, dadst=rb.dadst, dasrc=rb.dasrc,
                         dz=rb.dz, datt=rb.datt)

    def fwd(self, csr=None, att=None, keep=None):
        c, o, b = self.c, self.o, self.b
        ptr, nbr, eid = csr or b["dst"]
        return ref.forward(ptr, nbr, eid, o["z"], o["att"] if att is None else att, o["bias"], c["relu"], c["slope"], c["p"],
                           self.keep if keep is None else keep, c["K"], c["D"], b["E"])

    def bwd(self, csr=None, att=None, keep=None):
        c, o, b = self.c, self.o, self.b
        ptr, nbr, eid = csr or b["dst"]
        return ref.backward(ptr, nbr, eid, o["z"], o["att"] if att is None else att, *self.state, o["gout"], c["slope"], c["p"],
                            self.keep if keep is None else keep, c["K"], c["D"], b["E"])

    def both(self, **kw):
        f, r = self.fwd(**kw), self.bwd(**kw)
        return dict(out=f.out, adst=f.adst, asrc=f.asrc, mx=f.mx, den=f.den, draw=r.draw, dadst=r.dadst, dasrc=r.dasrc, dz=r.dz, datt=r.datt)

    def ratio(self, got):
        J = self.J
        r = dict(J.state(got["adst"], got["asrc"], got["mx"], got["den"]))
        r.update(J.out(got["out"]))
        r.update(J.grads(self.state, self.o["gout"], got["draw"], got["dadst"], got["dasrc"], got["dz"], got["datt"])[0])
        rat = {}
        return ref.worst(r, rat), rat


def _defects(s):
    """name -> outputs of the reference with that defect (None: the defect does not exist for this case)"""
    c, b, o, f, rb, J = s.c, s.b, s.o, s.J.f, s.rb, s.J
    K, D, E, p = c["K"], c["D"], b["E"], c["p"]
    ptr, nbr, eid = b["dst"]
    ri, ed = J.ri, J.ed
    out = {}
    # the last slot of every row with more than eight slots left out
    deg = np.diff(ptr)
    drop = np.zeros(len(nbr), bool)
    drop[(ptr[1:] - 1)[deg > 8]] = True
    ptr2 = np.concatenate([[0], np.cumsum(deg - (deg > 8))]).astype(np.int32)
    out["last slot of rows over eight left out"] = s.both(csr=(ptr2, nbr[~drop], eid[~drop]))
    # the node's own loop left out of the max / of the sum
    neg = torch.full((N, K), -float("inf"), dtype=F64)
    out["loop left out of the max"] = dict(s.good, mx=ref._seg_max(neg, ri, f.le))
    out["loop left out of the sum"] = dict(s.good, den=f.den - torch.exp(f.ll - f.mx))
    if p > 0:
        keep = torch.from_numpy(s.keep)
        if K > 1:
            out["head (k + 1) % K's keep decision"] = s.both(keep=keep.roll(-1, 1))
        k2 = keep.clone()
        long_rows = np.nonzero(deg >= 17)[0]
        k2[torch.from_numpy(eid[ptr[long_rows] + 16]).long()] = keep[torch.from_numpy(eid[ptr[long_rows] + 15]).long()]
        assert not torch.equal(k2, keep)
        out["slot 16 takes slot 15's keep decision"] = s.both(keep=k2)
        out["1 / (1 - p) applied twice"] = s.both(keep=keep / (1 - p))
        out["1 / (1 - p) not applied"] = s.both(keep=keep * (1 - p))
    att = o["att"]
    out["halves of att swapped"] = s.both(att=torch.cat([att[:, D:], att[:, :D]], 1))
    out["an input self loop given a slot"] = s.both(csr=_csr_keep_loops(b["ei"], N, 1))
    if c["bias"]:
        bias = o["bias"].double().reshape(K, D)
        pre = (f.pre.reshape(N, K, D) - bias + bias / f.den[:, :, None]).reshape(N, K * D)
        out["bias added before the division"] = dict(s.good, out=torch.relu(pre) if c["relu"] else pre)
    if c["slope"] > 0:
        d2 = rb.draw.clone()
        d2[ed] = rb.draw[ed] / rb.lr_e
        d2[E:] = rb.draw[E:] / rb.lr_l
        out["slope dropped from the backward"] = dict(s.good, draw=d2)
    S2 = rb.S - rb.a_l * rb.dal_l
    d2 = rb.draw.clone()
    d2[ed] = rb.a_e * (rb.dal_e - S2[ri]) * rb.lr_e
    d2[E:] = rb.a_l * (rb.dal_l - S2) * rb.lr_l
    out["S without the loop"] = dict(s.good, draw=d2)
    return out


SENSITIVITY_CASES = ["wave-1", "wave-asc-drop", "fused-5x4", "fused-2x16-asc", "fused-6x16", "vec1-7x1", "mis-io-1x16", "twopass-3x12"]


@pytest.mark.parametrize("name", SENSITIVITY_CASES)
def test_seeded_defects_of_the_reference_exceed_the_bounds(name):
    s = _Setup(name)
    top, rat = s.ratio(s.good)
    assert top == 0.0, rat                                        # the reference against itself
    top, rat = s.ratio({k: v.float() for k, v in s.good.items()})
    assert top <= 1.0, rat                                        # rounded to fp32 it is still inside every bound
    if s.c["asc"]:                                                # the ascending set reaches the flush range of the bare v_exp_f32
        assert float((s.J.f.le - s.J.f.mx[s.J.ri]).min()) < -126 * np.log(2.0)
    seen = set()
    for what, got in _defects(s).items():
        top, rat = s.ratio(got)
        print("%-14s %-42s worst err/bound %.3e" % (name, what, top))
        assert top > 1.0, (name, what, rat)
        seen.add(what)
    assert len(seen) >= 7


def test_every_defect_is_seeded_somewhere():
    names = set()
    for n in SENSITIVITY_CASES:
        c = C.case_by_name(n)
        names |= {"keep"} if c["p"] > 0 else set()
        names |= {"heads"} if c["p"] > 0 and c["K"] > 1 else set()
        names |= {"bias"} if c["bias"] else set()
        names |= {"slope"} if c["slope"] > 0 else set()
    assert names == {"keep", "heads", "bias", "slope"}
