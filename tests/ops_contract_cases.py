"""The case table of the operator-level contract (csrc/gcn.hip, csrc/attn.hip, csrc/plan.hip), the inputs of every case, one
launch routine per exported launcher and the judge that holds its outputs to tests/ops_contract_ref.py.  Importable without a
GPU: tests/test_ops_contract_ref.py runs every case through libcalhost.so with the host backend below and seeds defects into the
reference's outputs; tests/test_gpu_ops_contract.py runs the same cases through libcalhip.so with tests.helpers.Buf.

Widths.  vec: 4, 20, 32 (G 8), 36, 64 (G 16), 100, 128 (G 32), 132, 256 (G 64), 260 (a second, partly filled sweep); scalar by
width: 1, 7 (G 8), 13 (G 16), 22 (G 32), 33, 70, 130 (G 64, one to three sweeps); scalar by misalignment: 8, 16, 32, 64 with ONE
operand one float past a 16-byte boundary, rotated so that every aligned16 term of every launcher's vec_ok is once the only
false one (8 is there so that the scalar G 8 instantiation is once filled: 1 and 7 leave lanes idle); column kernels also 258
(scalar) and 1028 (vec): two column sweeps.  Rows: the degree ladder of tests/ladder.py (N = 301) in the view the kernel walks;
N in PART_N at width 20 for the part-count edges of finish_colsum (0, 1, 1, 2, 16, 17, 32, 33, 48, 49 parts); N = 16897 at
width 4 (34 rows per block).  The mirror of the dispatch (`group_for`, `vec_ok`, `rows_per_block`, `col_threads`, `paths`) maps
every case to the (kernel, VEC, G, sweeps, parts) it runs; tests/test_ops_contract_ref.py asserts that the table is complete.
"""
import functools
import zlib

import numpy as np
import torch

from tests import ops_contract_ref as R
from tests import sparse_contract_ref as sref
from tests.ladder import N as LADDER_N
from tests.ladder import ladder_batch

NAN = float("nan")
F32, F64 = torch.float32, torch.float64
CANARY, NCAN = 12345.0, 256                       # tests.helpers.Buf's
VEC_WIDTHS = [4, 20, 32, 36, 64, 100, 128, 132, 256, 260]
SCALAR_WIDTHS = [1, 7, 13, 22, 33, 70, 130]
MIS_WIDTHS = [8, 16, 32, 64]
COL_WIDTHS = [258, 1028]
PART_N = [0, 1, 32, 33, 512, 513, 1024, 1025, 1536, 1537]
BIG_N = 16897
LOOP_W = [0.0, 1.0, 2.0, 1.25]
SPLITS = [1, 2, 3, 64]
POOL_SIZES = (0, 1, 2, 37, 0, 63, 130, 5, 0)

#: launcher -> its lane-group kernels, its column kernels, the operands behind the aligned16 terms of its vec_ok, the view
#: whose rows carry the ladder
LAUNCHERS = {
    "norm_fwd": dict(g=[], col=[], terms=[], key=0),
    "spmm": dict(g=["k_spmm"], col=[], terms=["h", "out", "bias"], key=1),
    "relu_bwd_colsum": dict(g=[], col=["k_relu_bwd_colsum"], terms=["dout", "y", "dz", "part"], key=1),
    "norm_bwd": dict(g=["k_sddmm"], col=[], terms=["h", "dz"], key=1),
    "edge_att_fwd": dict(g=["k_edge_proj"], col=[], terms=["x", "W"], key=0),
    "edge_att_bwd": dict(g=[], col=["k_edge_att_bwd_x"], terms=["x", "W", "dx", "ws"], key=0),
    "node_att_fwd": dict(g=["k_node_att_split"], col=[], terms=["x", "Wn", "xc", "xo"], key=1),
    "node_att_bwd": dict(g=["k_node_att_split_bwd"], col=["k_wcolsum1"], terms=["x", "Wn", "dxc", "dxo", "dx", "ws"], key=1),
    "add_pool_fwd": dict(g=[], col=["k_add_pool"], terms=["x", "dst"], key=1),
    "add_pool_bwd": dict(g=["k_add_pool_bwd"], col=[], terms=["dout", "dx"], key=1),
}
FINISH = ("relu_bwd_colsum", "edge_att_bwd", "node_att_bwd")          # launchers that end in finish_colsum


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def group_for(H, vec):
    need, g = cdiv(H, vec), 1
    while g < need and g < 64:
        g <<= 1
    return g


def dispatch(H, vec_ok):
    """CAL_DISPATCH_VG -> (VEC, G)"""
    vec = 4 if vec_ok else 1
    return vec, max(8, group_for(H, vec))


def rows_per_block(N):
    return max(32, (N + 511) // 512)


def parts(N):
    return 0 if N == 0 else cdiv(N, rows_per_block(N))


def col_threads(H, vec):
    t = H // 4 if vec else H
    return 256 if t > 256 else cdiv(t, 64) * 64


def vec_ok(c):
    return c["H"] % 4 == 0 and not c["off"]


def rows_of(c):
    return len(POOL_SIZES) if c["launcher"] == "add_pool_fwd" else graph_of(c["graph"])["N"]


def paths(c):
    """[(kernel, VEC, G or 0, sweeps)] that the case launches, and the part count its finish pass sums"""
    L, H, n = LAUNCHERS[c["launcher"]], c["H"], rows_of(c)
    out = []
    if n > 0:
        vec = 4 if vec_ok(c) else 1
        for k in L["g"]:
            _, G = dispatch(H, vec_ok(c))
            out.append((k, vec, G, cdiv(H, G * vec)))
        for k in L["col"]:
            out.append((k, vec, 0, cdiv(H, col_threads(H, vec == 4) * vec)))
    return out, (parts(n) if c["launcher"] in FINISH and c.get("dbias", 1) else None)


# ---- graphs -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph_of(spec):
    """("ladder", key) | ("rand", N) | ("noedge", N) | ("signed",) -> ei, N, E, batch, B, src / dst views, loops"""
    kind = spec[0]
    extra = {}
    if kind == "ladder":
        b = ladder_batch(spec[1])
        ei, n, batch, B = b["ei"], LADDER_N, b["batch"], 3
    elif kind == "rand":
        n = spec[1]
        rng = np.random.default_rng(7000 + n)
        ei = rng.integers(0, max(n, 1), (2, 3 * n)).astype(np.int64)
        if n > 0:
            lp = rng.integers(0, n, min(n, 3))
            pos = rng.choice(ei.shape[1], len(lp), replace=False)
            ei[:, pos] = lp                                       # input self loops (random pairs add a few more)
        B = n // 40 + 3
        batch = np.sort(rng.integers(1, B - 1, n)).astype(np.int64)    # graphs 0 and B - 1 are empty
    elif kind == "noedge":
        n, B = spec[1], 2
        ei, batch = np.zeros((2, 0), np.int64), np.repeat([0, 1], [n - n // 2, n // 2]).astype(np.int64)
    else:
        # signed weights: node 0 has out-weights +0.5 and -0.5 (degree exactly 0 at loop_w 0), node 1 -0.75 and -0.5 (negative),
        # nodes 2 and 3 have no edge, 4..39 a ring and random edges with positive weights, self loops on 9, 10, 10
        n, B = 40, 2
        rng = np.random.default_rng(4242)
        ring = np.stack([np.arange(4, 40), np.r_[np.arange(5, 40), 4]])
        rnd = rng.integers(4, 40, (2, 60))
        sp = np.array([[0, 0, 1, 1, 9, 10, 10], [5, 6, 7, 8, 9, 10, 10]])
        ei = np.concatenate([sp, ring, rnd], 1).astype(np.int64)
        w = 0.05 + 0.95 * rng.random(ei.shape[1])
        w[:4] = [0.5, -0.5, -0.75, -0.5]
        perm = rng.permutation(ei.shape[1])
        ei, extra["w"] = ei[:, perm], torch.from_numpy(w[perm]).float()
        batch = np.repeat([0, 1], [20, 20]).astype(np.int64)
    g = {"ei": ei, "N": n, "E": ei.shape[1], "batch": batch, "B": B, "loops": ei[0] == ei[1],
         "dst": sref.csr_view(ei, n, 1), "src": sref.csr_view(ei, n, 0)}
    g.update(extra)
    return g


# ---- the table ----------------------------------------------------------------------------------------------------------
def _axes(launcher, j, off):
    """the axis values of the j-th case of a launcher (every value of every axis occurs; an operand that is off is present)"""
    if launcher == "spmm":
        bias = 1 if "bias" in off else (j // 2) % 2
        return dict(relu=j % 2, bias=bias, loop_w=LOOP_W[(j + j // 4) % 4], key=1 if bias else (j // 4) % 2, unit=0)
    if launcher == "relu_bwd_colsum":
        dz = "buf" if "dz" in off else ["buf", "null", "alias"][j % 3]
        if off and dz == "alias":
            dz = "buf"                                             # dz == dout would put two terms off at once
        return dict(y=1 if "y" in off else j % 2, dz=dz, dbias=1 if "part" in off or dz == "null" else (j // 2) % 2)
    if launcher == "norm_bwd":
        return dict(w=(j // 2) % 2, loop_w=LOOP_W[j % 4])
    if launcher == "edge_att_bwd":
        return dict(accumulate=j % 2)
    if launcher == "add_pool_fwd":
        return dict(S=SPLITS[j % 4])
    return {}


def _float_cases():
    out = []
    for launcher, L in LAUNCHERS.items():
        if launcher == "norm_fwd":
            continue
        rows = []                                                  # (name, H, graph, off)
        lad = ("ladder", L["key"])
        widths = VEC_WIDTHS + SCALAR_WIDTHS + (COL_WIDTHS if L["col"] else [])
        rows += [("H%d" % H, H, lad, {}) for H in widths]
        nmis = max(len(L["terms"]), len(MIS_WIDTHS))
        rows += [("H%d-%s-off" % (MIS_WIDTHS[i % 4], L["terms"][i % len(L["terms"])]), MIS_WIDTHS[i % 4], lad,
                  {L["terms"][i % len(L["terms"])]: 1}) for i in range(nmis)]
        if launcher != "add_pool_fwd":                             # its rows are the graphs of POOL_SIZES
            rows += [("N%d" % n, 20, ("rand", n), {}) for n in PART_N] + [("N%d" % BIG_N, 4, ("rand", BIG_N), {})]
            if launcher not in ("add_pool_bwd", "node_att_fwd", "node_att_bwd", "relu_bwd_colsum"):
                rows += [("E0", 20, ("noedge", 37), {})]
        for j, (name, H, graph, off) in enumerate(rows):
            c = dict(launcher=launcher, name="%s/%s" % (launcher, name), H=H, graph=graph, off=off)
            c.update(_axes(launcher, j, off))
            if launcher == "spmm" and graph[0] == "ladder":
                c["graph"] = ("ladder", c["key"])
            if launcher == "relu_bwd_colsum" and graph[0] == "rand":
                c["dbias"] = 1                                     # the part-count sweep is about k_colsum_finish
            out.append(c)
    sp = dict(launcher="spmm", off={}, relu=0, unit=0)
    # cal_spmm_fwd as cal_amd/ops.py and cal_amd/gradient.py call it
    out += [dict(sp, name="spmm/by-source-null-bias", H=64, graph=("ladder", 0), key=0, bias=0, loop_w=1.0),
            dict(sp, name="spmm/width1-loop0", H=1, graph=("ladder", 1), key=1, bias=0, loop_w=0.0),
            dict(sp, name="spmm/unit-dis", H=20, graph=("ladder", 1), key=1, bias=0, loop_w=1.25, unit=1),
            dict(sp, name="spmm/width1-by-source", H=1, graph=("ladder", 0), key=0, bias=0, loop_w=1.25)]
    for wi in (0, 1):
        for lw in LOOP_W:
            out.append(dict(launcher="norm_fwd", name="norm_fwd/ladder-w%d-loop%g" % (wi, lw), H=0, graph=("ladder", 0), off={}, w=wi, loop_w=lw))
    for j, n in enumerate(PART_N + [BIG_N]):
        out.append(dict(launcher="norm_fwd", name="norm_fwd/N%d" % n, H=0, graph=("rand", n), off={}, w=j % 2, loop_w=LOOP_W[j % 4]))
    out.append(dict(launcher="norm_fwd", name="norm_fwd/E0", H=0, graph=("noedge", 37), off={}, w=1, loop_w=1.0))
    # exact semantics: a weighted degree of exactly 0, a negative one (NaN where pow(-0.5) has NaN)
    out.append(dict(launcher="norm_fwd", name="norm_fwd/signed", H=0, graph=("signed",), off={}, w=1, loop_w=0.0))
    out.append(dict(launcher="norm_bwd", name="norm_bwd/signed", H=20, graph=("signed",), off={}, w=1, loop_w=0.0))
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _float_cases()


def cases_of(launcher):
    return [c for c in CASES if c["launcher"] == launcher]


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def _hub():
    """node 7 has 3000 in-edges whose edge ids alternate with 3000 in-edges of node 8"""
    rng = np.random.default_rng(77)
    src = rng.integers(9, 50, 6000)
    dst = np.tile([7, 8], 3000)
    return np.stack([src, dst]).astype(np.int64), 50


def _rand_ei(n, e, seed):
    return np.random.default_rng(seed).integers(0, n, (2, e)).astype(np.int64)


def _dups():
    ei = _rand_ei(20, 30, 5)
    return np.tile(ei, (1, 3))[:, np.random.default_rng(6).permutation(90)], 20


def _oor():
    ei = ladder_batch(1)["ei"].copy()
    ei[0, 1234] = LADDER_N                                         # one index one past the last node
    return ei, LADDER_N


PLAN_CASES = {
    "ladder-dst": lambda: (ladder_batch(1)["ei"], LADDER_N), "ladder-src": lambda: (ladder_batch(0)["ei"], LADDER_N),
    "N8192": lambda: (_rand_ei(8192, 3 * 8192, 1), 8192), "N8193": lambda: (_rand_ei(8193, 3 * 8193, 2), 8193),
    "N32768": lambda: (_rand_ei(32768, 3 * 32768, 3), 32768), "N32769-chunked": lambda: (_rand_ei(32769, 2 * 32769, 4), 32769),
    "N40000-E9": lambda: (_rand_ei(40000, 9, 5), 40000), "hub": _hub, "duplicates": _dups, "out-of-range": _oor,
    "E0": lambda: (np.zeros((2, 0), np.int64), 5), "N0": lambda: (np.zeros((2, 0), np.int64), 0),
}


def plan_scan(n, e):
    """-> ("single", passes) | ("chunked", chunks): which scan cal_plan_build takes"""
    if n > 4 * 8192 and e >= 2 * cdiv(n, 8192):
        return "chunked", cdiv(n, 8192)
    return "single", cdiv(n, 8192)


GRAPH_PTR_CASES = {                                                # name -> (batch, B, valid)
    "ladder": (ladder_batch(1)["batch"], 3, True),
    "empty-first-middle-last": (np.repeat([1, 2, 5, 6], [3, 1, 300, 2]).astype(np.int64), 9, True),
    "B0-N0": (np.zeros(0, np.int64), 0, True),
    "N0": (np.zeros(0, np.int64), 4, True),
    "unsorted": (np.array([0, 0, 2, 1, 3, 3], np.int64), 4, False),
    "id-past-B": (np.array([0, 1, 1, 6, 3, 3], np.int64), 4, False),
    "id-past-B-last": (np.array([0, 1, 1, 2, 3, 5], np.int64), 4, False),
    "negative-id": (np.array([0, -3, 1, 1, 2], np.int64), 4, False),        # the canary in FRONT of gptr: no store below gptr[0]
}


# ---- inputs -------------------------------------------------------------------------------------------------------------
def inputs_of(c):
    """every operand of the case as CPU tensors (float32 / int), from a generator seeded by the case's name"""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    L, H = c["launcher"], c["H"]
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    if L == "add_pool_fwd":
        gptr = np.concatenate([[0], np.cumsum(POOL_SIZES)]).astype(np.int32)
        return dict(x=rn(int(gptr[-1]), H), gptr=gptr, B=len(POOL_SIZES), N=int(gptr[-1]))
    G = graph_of(c["graph"])
    N, E = G["N"], G["E"]
    loops = torch.from_numpy(G["loops"])
    i = dict(G=G, N=N, E=E)
    if L in ("norm_fwd", "norm_bwd"):
        w = G.get("w", 0.05 + 0.95 * ru(E)).clone() if c["w"] else None
        if w is not None:
            w[loops] = NAN                                         # never read: a self-loop column reaches no output
        i["w"] = w
    if L == "spmm":
        ne = 0.5 * rn(E)
        ne[loops] = NAN
        i.update(norm_e=ne, dis=torch.ones(N) if c["unit"] else 0.1 + 0.9 * ru(N), h=rn(N, H), bias=rn(H) if c["bias"] else None)
    elif L == "relu_bwd_colsum":
        y = torch.relu(rn(N, H))
        y[(ru(N, H) < 0.1) & (y == 0)] = -0.0
        i.update(dout=rn(N, H), y=y if c["y"] else None)
    elif L == "norm_bwd":
        if c["graph"] == ("signed",):                              # the dis that cal_gcn_norm_fwd hands on: 0, NaN and all
            dis = R.norm_fwd(G["src"][0], G["src"][2], G["ei"][0], G["ei"][1], G["w"], c["loop_w"])[0].float()
        else:
            dis = 0.1 + 0.9 * ru(N)
        i.update(dis=dis, h=rn(N, H), dz=rn(N, H))
    elif L == "edge_att_fwd":
        i.update(x=rn(N, H), W=1.5 * rn(2, 2 * H) / max(H, 1) ** 0.5, b=rn(2))
    elif L == "edge_att_bwd":
        datt = rn(2, E)
        datt[:, loops] = NAN
        i.update(x=rn(N, H), W=rn(2, 2 * H), att=torch.softmax(1.5 * rn(E, 2).double(), -1).t().contiguous().float(), datt=datt,
                 base=rn(N, H) if c["accumulate"] else None)
    elif L == "node_att_fwd":
        i.update(x=rn(N, H), Wn=1.5 * rn(2, H) / max(H, 1) ** 0.5, bn=rn(2))
    elif L == "node_att_bwd":
        i.update(x=rn(N, H), Wn=rn(2, H), att_n=torch.softmax(1.5 * rn(N, 2).double(), -1).float(), dxc=rn(N, H), dxo=rn(N, H))
    elif L == "add_pool_bwd":
        i.update(dout=rn(G["B"], H))
    return i


# ---- backends -----------------------------------------------------------------------------------------------------------
class HostBuf:
    """tests.helpers.Buf in host memory"""

    def __init__(self, n, dtype=F32, fill=None, data=None, off=0):
        self.n, self.off = int(n), int(off)
        self.full = torch.full((self.off + self.n + NCAN,), CANARY, dtype=dtype)
        self.t = self.full[self.off:self.off + self.n]
        if data is not None:
            self.t.copy_(data.reshape(-1).to(dtype))
        elif fill is not None:
            self.t.fill_(fill)

    def ptr(self):
        return self.full.data_ptr() + self.off * self.full.element_size()

    def intact(self):
        return bool((self.full[self.off + self.n:] == CANARY).all() and (self.full[:self.off] == CANARY).all())


class HostBackend:
    """libcalhost.so on host pointers"""

    def __init__(self):
        self.pool = []

    def buf(self, n, dtype=F32, fill=None, data=None, off=0):
        b = HostBuf(n, dtype, fill, data, off)
        self.pool.append(b)
        return b

    def call(self, name, *args):
        from cal_amd import _lib
        _lib.call(name, *args, None, host=True)

    def query(self, name, *args):
        from cal_amd import _lib
        return _lib.query(name, *args, host=True)

    def intact(self):
        return all(b.intact() for b in self.pool)

    def cpu(self, b):
        return b.t.clone()


def _np(be, a, dtype=torch.int32):
    return be.buf(len(a), dtype, data=torch.from_numpy(np.ascontiguousarray(a)))


def _p(b):
    return None if b is None else b.ptr()


# ---- one launch per launcher: fresh outputs, NaN-filled ---------------------------------------------------------------------
def _launch(c, i, be):
    """-> {name: output buffer}"""
    L, H, off = c["launcher"], c["H"], c["off"]
    o = lambda k: off.get(k, 0)
    fl = lambda k: be.buf(i[k].numel(), data=i[k], off=o(k)) if i.get(k) is not None else None
    nanb = lambda n, k=None: be.buf(n, fill=NAN, off=o(k) if k else 0)
    if L == "add_pool_fwd":
        B, S = i["B"], c["S"]
        out = nanb(B * H, "dst" if S == 1 else None)
        part = nanb(S * B * H, "dst") if S > 1 else None
        be.call("cal_add_pool_fwd", fl("x").ptr(), _np(be, i["gptr"]).ptr(), out.ptr(), _p(part), B, H, S)
        return dict(out=out)
    G, N, E = i["G"], i["N"], i["E"]
    src, dst = [_np(be, a) for a in G["src"]], [_np(be, a) for a in G["dst"]]
    row, col = _np(be, G["ei"][0].astype(np.int32)), _np(be, G["ei"][1].astype(np.int32))
    if L == "norm_fwd":
        dis, ne = nanb(N), nanb(E)
        be.call("cal_gcn_norm_fwd", src[0].ptr(), src[2].ptr(), row.ptr(), col.ptr(), _p(fl("w")), c["loop_w"], N, E, dis.ptr(), ne.ptr())
        return dict(dis=dis, norm_e=ne)
    if L == "spmm":
        v = dst if c["key"] == 1 else src
        out = nanb(N * H, "out")
        be.call("cal_spmm_fwd", v[0].ptr(), v[1].ptr(), v[2].ptr(), fl("norm_e").ptr(), fl("dis").ptr(), c["loop_w"], fl("h").ptr(),
                _p(fl("bias")), c["relu"], out.ptr(), N, H)
        return dict(out=out)
    if L == "relu_bwd_colsum":
        dout = fl("dout")
        dz = nanb(N * H, "dz") if c["dz"] == "buf" else dout if c["dz"] == "alias" else None      # alias: in place, as cal_amd/ops.py
        dbias = nanb(H) if c["dbias"] else None
        part = nanb(be.query("cal_colsum_parts", N) * H, "part") if c["dbias"] else None
        be.call("cal_relu_bwd_colsum", dout.ptr(), _p(fl("y")), _p(dz), _p(dbias), _p(part), N, H)
        return {k: b for k, b in (("dz", dz), ("dbias", dbias)) if b is not None}
    if L == "norm_bwd":
        gn, gs, dd, dw = nanb(E), nanb(N), nanb(N), nanb(E)
        be.call("cal_gcn_norm_bwd", dst[0].ptr(), dst[1].ptr(), dst[2].ptr(), src[0].ptr(), src[1].ptr(), src[2].ptr(), row.ptr(), col.ptr(),
                _p(fl("w")), fl("dis").ptr(), c["loop_w"], fl("h").ptr(), fl("dz").ptr(), gn.ptr(), gs.ptr(), dd.ptr(), dw.ptr(), N, E, H)
        return dict(gn_e=gn, gself=gs, ddeg=dd, dw=dw)
    if L == "edge_att_fwd":
        pq, att = nanb(4 * N), nanb(2 * E)
        be.call("cal_edge_att_fwd", fl("x").ptr(), fl("W").ptr(), fl("b").ptr(), row.ptr(), col.ptr(), pq.ptr(), att.ptr(), N, E, H)
        return dict(pq=pq, att=att)
    if L == "edge_att_bwd":
        dx = be.buf(N * H, data=i["base"], off=o("dx")) if c["accumulate"] else nanb(N * H, "dx")
        dW, db, ws = nanb(4 * H), nanb(2), nanb(be.query("cal_edge_att_bwd_ws", N, E, H), "ws")
        be.call("cal_edge_att_bwd", fl("x").ptr(), fl("W").ptr(), fl("att").ptr(), fl("datt").ptr(), src[0].ptr(), src[2].ptr(), dst[0].ptr(),
                dst[2].ptr(), dx.ptr(), c["accumulate"], dW.ptr(), db.ptr(), ws.ptr(), N, E, H)
        return dict(dx=dx, dW=dW, db=db)
    if L == "node_att_fwd":
        a, xc, xo = nanb(2 * N), nanb(N * H, "xc"), nanb(N * H, "xo")
        be.call("cal_node_att_split_fwd", fl("x").ptr(), fl("Wn").ptr(), fl("bn").ptr(), a.ptr(), xc.ptr(), xo.ptr(), N, H)
        return dict(att_n=a, xc=xc, xo=xo)
    if L == "node_att_bwd":
        dx, dWn, dbn, ws = nanb(N * H, "dx"), nanb(2 * H), nanb(2), nanb(be.query("cal_node_att_bwd_ws", N, H), "ws")
        be.call("cal_node_att_split_bwd", fl("x").ptr(), fl("Wn").ptr(), fl("att_n").ptr(), fl("dxc").ptr(), fl("dxo").ptr(), dx.ptr(),
                dWn.ptr(), dbn.ptr(), ws.ptr(), N, H)
        return dict(dx=dx, dWn=dWn, dbn=dbn)
    if L == "add_pool_bwd":
        dx = nanb(N * H, "dx")
        be.call("cal_add_pool_bwd", fl("dout").ptr(), _np(be, G["batch"], torch.int64).ptr(), dx.ptr(), N, H)
        return dict(dx=dx)
    raise KeyError(L)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)


def run(c, i, be, launch=_launch):
    """the launcher twice on fresh outputs -> the first run's outputs as CPU tensors, [what went wrong around them]"""
    a = launch(c, i, be)
    fails = [] if be.intact() else ["a canary around a buffer was overwritten by the first launch"]
    b = launch(c, i, be)
    fails += [] if be.intact() else ["a canary around a buffer was overwritten by the second launch"]
    got = {k: be.cpu(v) for k, v in a.items()}
    again = {k: be.cpu(v) for k, v in b.items()}
    fails += ["%s differs between two launches" % k for k in got if not _same_bits(got[k], again[k])]
    return got, fails


# ---- the reference's outputs, and the judge ---------------------------------------------------------------------------------
def _views(c, i):
    G = i["G"]
    return G["src"], G["dst"], G["ei"][0], G["ei"][1]


def reference(c, i, stored=False):
    """the launcher's outputs in float64, in the layout of the buffers.  stored: every intermediate that the launcher hands
    back is rounded to fp32 before the next stage reads it (what a perfect fp32 kernel would store)"""
    L = c["launcher"]
    rd = (lambda t: t.float().double()) if stored else (lambda t: t)
    if L == "add_pool_fwd":
        return dict(out=R.add_pool(i["x"], i["gptr"])[0])
    src, dst, row, col = _views(c, i)
    if L == "norm_fwd":
        dis = rd(R.norm_fwd(src[0], src[2], row, col, i["w"], c["loop_w"])[0])
        return dict(dis=dis, norm_e=R.norm_e_from(dis, row, col, i["w"]))
    if L == "spmm":
        return dict(out=R.spmm(*(dst if c["key"] == 1 else src), i["norm_e"], i["dis"], c["loop_w"], i["h"], i["bias"], c["relu"])[0])
    if L == "relu_bwd_colsum":
        dz, db, _ = R.relu_bwd_colsum(i["dout"], i["y"])
        return {k: v for k, v in (("dz", dz), ("dbias", db)) if (k == "dz" and c["dz"] != "null") or (k == "dbias" and c["dbias"])}
    if L == "norm_bwd":
        gn, gs, _, _ = R.sddmm(*dst, i["h"], i["dz"], i["E"])
        gn, gs = rd(gn), rd(gs)
        ddeg = rd(R.norm_bwd_node(src, dst, i["w"], i["dis"], c["loop_w"], gn, gs)[0])
        return dict(gn_e=gn, gself=gs, ddeg=ddeg, dw=R.norm_bwd_edge(row, col, i["dis"], gn, ddeg)[0])
    if L == "edge_att_fwd":
        pq = rd(R.edge_proj(i["x"], i["W"])[0])
        return dict(pq=pq, att=R.edge_att_from_pq(pq, i["b"], row, col)[0].t().contiguous())
    if L == "edge_att_bwd":
        dx, dW, db = R.edge_att_bwd(i["x"], i["W"], i["att"], i["datt"], (src[0], src[2]), (dst[0], dst[2]), i["base"])[0]
        return dict(dx=dx, dW=dW, db=db)
    if L == "node_att_fwd":
        a = rd(R.node_att(i["x"], i["Wn"], i["bn"])[0])
        xc, xo = R.node_split_from(a, i["x"])
        return dict(att_n=a, xc=xc, xo=xo)
    if L == "node_att_bwd":
        dx, dWn, dbn = R.node_att_bwd(i["x"], i["Wn"], i["att_n"], i["dxc"], i["dxo"])[0]
        return dict(dx=dx, dWn=dWn, dbn=dbn)
    if L == "add_pool_bwd":
        return dict(dx=R.add_pool_bwd(i["dout"].to(F64), i["G"]["batch"]))
    raise KeyError(L)


def _xe(x_exp, logits):
    if not callable(x_exp):
        return x_exp
    return x_exp(float((logits[:, 0] - logits[:, 1]).abs().max()) if logits.numel() else 0.0)


def judge(c, i, got, x_exp=2 * R.U):
    """-> {output: worst err / bound}, [failures].  x_exp: the relative error of the implementation's fp32 exp, or a function
    of the largest |l_0 - l_1| of the case that measures it on that range"""
    L, H, tag = c["launcher"], c["H"], c["name"]
    rat, fails = {}, []
    cmp = lambda k, want, bound, g=None: R.compare(k, (got[k] if g is None else g).reshape(want.shape), want, bound, rat, fails, tag)
    if L == "add_pool_fwd":
        cmp("out", *R.add_pool(i["x"], i["gptr"]))
        return rat, fails
    N, E = i["N"], i["E"]
    src, dst, row, col = _views(c, i)
    if L == "norm_fwd":
        dis, _, deg, M = R.norm_fwd(src[0], src[2], row, col, i["w"], c["loop_w"])
        cmp("dis", dis, R.dis_bound(dis, deg, M, R.slots(src[0])))
        ne = R.norm_e_from(got["dis"], row, col, i["w"])           # on the stored dis
        cmp("norm_e", ne, 4 * R.U * ne.abs() * R.SLACK)
    elif L == "spmm":
        want, T, n = R.spmm(*(dst if c["key"] == 1 else src), i["norm_e"], i["dis"], c["loop_w"], i["h"], i["bias"], c["relu"])
        cmp("out", want, R.spmm_bound(T, n))
    elif L == "relu_bwd_colsum":
        dz, db, mag = R.relu_bwd_colsum(i["dout"], i["y"])
        if c["dz"] != "null":
            R.exact("dz", got["dz"].reshape(dz.shape), dz, rat, fails, tag)
        if c["dbias"]:
            cmp("dbias", db, R.colsum_bound(mag, N))
    elif L == "norm_bwd":
        gn, gs, mn, ms = R.sddmm(*dst, i["h"], i["dz"], E)
        cmp("gn_e", gn, R.dot_bound(mn, H))                        # NaN (never written) exactly on the edges without a slot
        cmp("gself", gs, R.dot_bound(ms, H))
        cmp("ddeg", *R.norm_bwd_node(src, dst, i["w"], i["dis"], c["loop_w"], got["gn_e"], got["gself"]))
        cmp("dw", *R.norm_bwd_edge(row, col, i["dis"], got["gn_e"], got["ddeg"]))
    elif L == "edge_att_fwd":
        pq, mag = R.edge_proj(i["x"], i["W"])
        cmp("pq", pq, R.dot_bound(mag, H))
        a, lg, Lm = R.edge_att_from_pq(got["pq"].reshape(N, 4), i["b"], row, col)
        cmp("att", a, R.softmax2_bound(a, lg, Lm, 3, _xe(x_exp, lg)), got["att"].reshape(2, E).t())
    elif L == "edge_att_bwd":
        want, bnd = R.edge_att_bwd(i["x"], i["W"], i["att"], i["datt"], (src[0], src[2]), (dst[0], dst[2]), i["base"])
        for k, w_, b_ in zip(("dx", "dW", "db"), want, bnd):
            cmp(k, w_, b_)
    elif L == "node_att_fwd":
        a, lg, Lm = R.node_att(i["x"], i["Wn"], i["bn"])
        cmp("att_n", a, R.softmax2_bound(a, lg, Lm, H + 2, _xe(x_exp, lg)))
        for k, w_ in zip(("xc", "xo"), R.node_split_from(got["att_n"].reshape(N, 2), i["x"])):
            cmp(k, w_, R.U * w_.abs() * R.SLACK)
    elif L == "node_att_bwd":
        want, bnd = R.node_att_bwd(i["x"], i["Wn"], i["att_n"], i["dxc"], i["dxo"])
        for k, w_, b_ in zip(("dx", "dWn", "dbn"), want, bnd):
            cmp(k, w_, b_)
    elif L == "add_pool_bwd":
        R.exact("dx", got["dx"].reshape(N, H), R.add_pool_bwd(i["dout"], i["G"]["batch"]), rat, fails, tag)
    return rat, fails


# ---- the plan and graph_ptr, in integers --------------------------------------------------------------------------------
FILL = -7


def launch_plan(ei, n, be):
    E = ei.shape[1]
    ib = lambda m: be.buf(m, torch.int32, fill=FILL)
    o = dict(rowptr_dst=ib(n + 1), nbr_dst=ib(E), eid_dst=ib(E), rowptr_src=ib(n + 1), nbr_src=ib(E), eid_src=ib(E), row32=ib(E),
             col32=ib(E))
    work, o["status"] = ib(4 * (n + 1) + 4 * E), ib(1)
    be.call("cal_plan_build", _np(be, ei.reshape(-1), torch.int64).ptr(), E, n, *(o[k].ptr() for k in R.PLAN_KEYS), work.ptr(), o["status"].ptr())
    return o


def judge_plan(ei, n, got):
    """every output exactly the reference; the slots behind nnz untouched"""
    want, fails = R.plan(ei, n), []
    nnz = int(want["rowptr_dst"][-1])
    for k in R.PLAN_KEYS:
        g = np.asarray(got[k])
        m = nnz if k[:3] in ("nbr", "eid") else len(g)
        if not np.array_equal(g[:m], want[k]):
            fails.append("%s differs from the stable counting sort in %d places" % (k, int((g[:m] != want[k]).sum())))
        if not (g[m:] == FILL).all():
            fails.append("%s was written behind its %d entries" % (k, m))
    if int(got["status"][0]) != want["status"]:
        fails.append("status %d, expected %d" % (int(got["status"][0]), want["status"]))
    return fails


def launch_graph_ptr(batch, B, be):
    gptr, status = be.buf(B + 1, torch.int32, fill=FILL, off=4), be.buf(1, torch.int32, fill=0)
    be.call("cal_graph_ptr", _np(be, batch, torch.int64).ptr(), len(batch), B, gptr.ptr(), status.ptr())
    return dict(gptr=gptr, status=status)


def judge_graph_ptr(batch, B, valid, got):
    fails = []
    if valid:
        if int(got["status"][0]) != 0:
            fails.append("status %d on a valid batch" % int(got["status"][0]))
        if not np.array_equal(np.asarray(got["gptr"]), R.graph_ptr(batch, B)):
            fails.append("gptr differs")
    elif int(got["status"][0]) & 2 == 0:
        fails.append("status bit 1 not set")
    return fails
