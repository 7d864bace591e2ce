"""The cases of tests/test_gpu_gat_contract.py and their operands, in one place so that the CPU test
(tests/test_gat_contract_ref.py) can show that the very inputs and bounds the GPU test uses notice seeded defects: the shape
table, the dispatch rule of gat_forward / gat_backward (csrc/gat.hip) restated in Python, and the seeded operand generator.
No GPU needed."""
import functools

import numpy as np
import torch

from tests import sparse_contract_ref as sref
from tests.ladder import N, N0, ladder_batch

F64 = torch.float64
MIS_IO = frozenset({"z", "out", "gout", "dz"})


def pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def group_for(H, vec):
    """lanes per row: group_for of csrc/common.hpp, with CAL_DISPATCH_VG's smallest group of 8"""
    need, g = -(-H // vec), 8
    while g < need and g < 64:
        g *= 2
    return g


def fwd_path(K, D, mis=frozenset(), bias=True):
    """gat_forward's choice for a shape and a set of operands that are not 16 B aligned -> (family, VEC, G, LH)"""
    al = lambda *names: all(n not in mis for n in names)
    vec_ok = D % 4 == 0 and al("z", "out") and (not bias or al("bias"))
    if vec_ok and K == 4 and D == 64 and al("att", "adst", "asrc", "mx", "den"):
        return ("wave", 4, 64, 16)
    if vec_ok and pow2(D // 4) and al("att") and D // 4 <= 64:
        return ("fused", 4, group_for(K * D, 4), D // 4)
    v = 4 if vec_ok else 1
    return ("twopass", v, group_for(K * D, v), None)


def bwd_path(K, D, mis=frozenset(), part_out_aligned=None):
    """gat_backward's choice -> (family, VEC, G, d att partial kernel), family "refuse" where it must return an error"""
    al = lambda *names: all(n not in mis for n in names)
    vec_ok = D % 4 == 0 and pow2(D // 4) and al("z", "gout", "dz", "att")
    v = 4 if vec_ok else 1
    if not (vec_ok or pow2(D)) or D // v > 64:                   # (the second: a head's D / VEC lanes must fit one group of 64)
        return ("refuse", v, None, None)
    part_al = al("ws") if part_out_aligned is None else part_out_aligned
    datt = "part_w" if K == 4 and D == 64 and al("z") and part_al else "part%d" % min(256, -(-K * D // 64) * 64)
    if vec_ok and K == 4 and D == 64 and al("adst", "asrc", "mx", "den", "ws"):
        return ("wave", 4, 64, datt)
    return ("rows", v, group_for(K * D, v), datt)


def _case(name, K, D, fwd, bwd, j, mis=frozenset(), asc=False, **over):
    """axes of variant j of a path: every value of p, relu, bias and slope occurs within j = 0..3 (and p > 0 at odd j)"""
    c = {"name": name, "K": K, "D": D, "fwd": fwd, "bwd": bwd, "mis": frozenset(mis), "asc": asc,
         "p": 0.3 if j % 2 else 0.0, "relu": (j // 2) % 2, "bias": ((j + 1) // 2) % 2, "slope": 0.2 if (j // 3) % 2 == 0 else 0.0}
    c.update(over)
    return c


def _build_cases():
    cs = []
    # the wave family: K = 4, D = 64 (DROP and non-DROP builds of the three kernels, k_gat_datt_part_w)
    for j in range(4):
        cs.append(_case("wave-%d" % j, 4, 64, "wave", "wave", j))
    cs.append(_case("wave-asc", 4, 64, "wave", "wave", 0, asc=True))
    cs.append(_case("wave-asc-drop", 4, 64, "wave", "wave", 1, asc=True))
    # the fused forward, LH = D / 4 (every LH and G, G == LH, G > LH, idle lanes, 1.5 and 2 column passes); its backward is
    # k_gat_bwd_dst_c<4, G> / k_gat_bwd_src<4, G>
    fused = [(1, 4), (5, 4), (3, 8), (4, 8), (8, 8), (2, 16), (6, 16), (1, 32), (4, 32), (1, 64), (2, 64), (8, 64), (1, 128), (3, 128),
             (1, 256), (2, 256)]
    for j, (K, D) in enumerate(fused):
        cs.append(_case("fused-%dx%d" % (K, D), K, D, "fused", "rows4", j))
    cs.append(_case("fused-2x16-asc", 2, 16, "fused", "rows4", 1, asc=True))
    # the two-pass VEC = 4 forward (D % 4 == 0, D / 4 no power of two); the backward refuses
    for j, (K, D) in enumerate([(4, 12), (3, 12), (2, 20), (1, 24)]):
        cs.append(_case("twopass-%dx%d" % (K, D), K, D, "twopass4", "refuse", j))
    # VEC = 1 by shape
    for j, (K, D) in enumerate([(4, 1), (7, 1), (4, 2), (16, 2), (32, 2), (40, 2)]):
        cs.append(_case("vec1-%dx%d" % (K, D), K, D, "twopass1", "rows1", j))
    cs.append(_case("vec1-4x2-asc", 4, 2, "twopass1", "rows1", 3, asc=True, slope=0.2))
    for j, (K, D) in enumerate([(3, 3), (4, 5), (1, 7)]):
        cs.append(_case("vec1-%dx%d" % (K, D), K, D, "twopass1", "refuse", j + 6))
    # VEC = 1 by alignment: operands one float past a 16 B boundary
    for j, (K, D) in enumerate([(1, 16), (4, 32), (4, 64)]):
        cs.append(_case("mis-io-%dx%d" % (K, D), K, D, "twopass1", "rows1", j + 1, mis=MIS_IO))
    cs.append(_case("mis-att-4x32", 4, 32, "twopass4", "rows1", 0, mis={"att"}))
    cs.append(_case("mis-bias-4x32", 4, 32, "twopass1", "rows4", 3, mis={"bias"}, bias=1))
    # the wave family declined: one of its 16 B operands misaligned
    for j, m in enumerate(["adst", "asrc", "mx", "den"]):
        cs.append(_case("nowave-%s" % m, 4, 64, "fused", "rows4", j, mis={m}))
    cs.append(_case("nowave-ws", 4, 64, "wave", "rows4", 1, mis={"ws"}))
    return cs


CASES = _build_cases()
# a head wider than a lane group of the backward: the forward runs on the scalar-scores path, the backward must be right or refuse
WIDE = [_case("wide-1x512", 1, 512, "twopass4", "refuse", 1), _case("wide-1x128-mis-z", 1, 128, "twopass1", "refuse", 1, mis={"z"}),
        _case("wide-1x256-mis-z", 1, 256, "twopass1", "refuse", 3, mis={"z"}, slope=0.2)]
FWD_FAMILY = {"wave": ("wave", 4), "fused": ("fused", 4), "twopass4": ("twopass", 4), "twopass1": ("twopass", 1)}
BWD_FAMILY = {"wave": ("wave", 4), "rows4": ("rows", 4), "rows1": ("rows", 1), "refuse": ("refuse", None)}


def case_by_name(name):
    return next(c for c in CASES + WIDE if c["name"] == name)


def seed_of(case):
    return 4000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"]))


@functools.lru_cache(maxsize=None)
def sorted_rows(key):
    """the ladder batch with the slots of every by-destination row in ascending order of the neighbour (the ascending operand
    set); the by-source view keeps its order"""
    b = dict(ladder_batch(key))
    ptr, nbr, eid = sref.csr_view(b["ei"], N, 1)
    order = np.lexsort((nbr, np.repeat(np.arange(N), np.diff(ptr))))
    b["dst"] = (ptr, nbr[order], eid[order])
    b["src"] = sref.csr_view(b["ei"], N, 0)
    return b


@functools.lru_cache(maxsize=None)
def views(key):
    b = dict(ladder_batch(key))
    b["dst"], b["src"] = sref.csr_view(b["ei"], N, 1), sref.csr_view(b["ei"], N, 0)
    return b


def batch_of(case, key):
    return sorted_rows(key) if case["asc"] else views(key)


def operands(case, key):
    """fp32 operands of a case on the ladder batch whose view `key` carries the ladder -> dict (torch CPU tensors).
    z has a non-zero mean, att is scaled so that a_dst and a_src each have a standard deviation of about 1.3: the logits of a
    row span several units with both signs.  Ascending set: a_src rises with the node id from -60 to 110 (times 1 - 0.1 k for
    head k), the slots of a row are in ascending order of the neighbour, so every batch of the online softmax moves the
    maximum, and in the long rows terms fall below 2^-126 of it."""
    K, D = case["K"], case["D"]
    g = torch.Generator().manual_seed(seed_of(case) + key)
    z = torch.randn(N, K, D, generator=g) * 0.8 + 0.2
    att = torch.randn(K, 2 * D, generator=g) * (1.6 / D ** 0.5)
    bias = torch.randn(K * D, generator=g) * 0.5 if case["bias"] else None
    gout = torch.randn(N, K * D, generator=g) + 0.1
    if case["asc"]:
        att[:, 0], att[:, D] = 0.0, 1.0
        rest = (z.double()[:, :, 1:] * att.double()[:, D + 1:]).sum(-1)                           # [N, K]
        rank = torch.arange(N, dtype=F64)
        rank[:N0] = rank[:N0] / (N0 - 1)
        rank[N0:] = (rank[N0:] - N0) / (N - N0 - 1)
        target = (-60.0 + 170.0 * rank)[:, None] * (1.0 - 0.1 * torch.arange(K, dtype=F64))
        z[:, :, 0] = (target - rest).float()
    return {"z": z.reshape(N, K * D), "att": att, "bias": bias, "gout": gout}
