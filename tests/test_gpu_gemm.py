"""The 64 x 64 tile GEMM (gemm.hip: k_gemm) and the K-split GEMM (gemm_ks.hip: k_gemm_ks) through the public cal_gemm /
cal_gemm_ws / cal_gemm_ks entries, against torch in fp64 on the CPU: the three bounds modes of the operand tiles, the
preloaded and the streaming K loop, all four (transA, transB) layouts, bias + ReLU, and split-K with the re-cut chunk.

Bound: max |C - ref| / max |ref| < 2e-5, the figure of the TN weight-gradient test at K up to 49 k
(test_weight_gradient_gemm_over_node_counts_around_the_split_window).  Every case prints its ratio (run with -s).  The worst
ratios measured on MI355X with the operand-tile and epilogue code in gemm_tile.hpp are in each test's docstring (6.2e-7 over
the whole file).  Expected from the number format: fp32 products summed in fp32 over K terms, about sqrt(K) * 6e-8 relative
to the largest entry -- 4e-6 at K = 4096; split-K sums slabs of 128, which is why K = 4096 stays at 2e-7.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 2e-5
CANARY = 12345.0

# (M, N, K): interior + preloaded path | interior, 5 K tiles: streaming loop | ragged in mn only: mode 1 |
# unaligned leading dimensions, ragged everywhere: mode 2, preloaded | mode 2, streaming loop
SHAPES = [(64, 64, 32), (128, 64, 160), (68, 72, 64), (67, 33, 10), (67, 33, 170)]
SHAPES_BIAS_RELU = [(64, 64, 32), (68, 72, 64), (67, 33, 10)]
# K = 4096: 32 slices of 128; K = 800: gemm_set_split re-cuts the chunk of 160 to 128 and makes S + 1 = 7 slices
SHAPES_SPLITK = [(64, 64, 4096), (64, 64, 800)]
SHAPES_KS = [(32, 32, 128), (33, 31, 10), (70, 40, 200)]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _operands(M, N, K, ta, tb, with_bias, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(K, N, generator=g)
    bias = torch.randn(N, generator=g) if with_bias else None
    ref = a.double() @ b.double()
    if with_bias:
        ref = torch.relu(ref + bias.double())
    a_st = (a.t().contiguous() if ta else a).to(DEV)            # transA: A stored [K, M]
    b_st = (b.t().contiguous() if tb else b).to(DEV)            # transB: B stored [N, K]
    return a_st, b_st, None if bias is None else bias.to(DEV), ref


def _ratio(c, ref):
    assert bool(torch.isfinite(c).all().item()), "C holds entries the kernel never wrote"
    return ((c.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _run_gemm(M, N, K, ta, tb, with_bias, seed):
    from cal_amd import _lib
    from cal_amd.plan import _p, _stream
    a, b, bias, ref = _operands(M, N, K, ta, tb, with_bias, seed)
    n_ws = _lib.query("cal_gemm_ws", M, N, K)
    ws = torch.full((n_ws + 1024,), float("nan"), device=DEV)
    ws[n_ws:].fill_(CANARY)                                     # canary behind the workspace the entry point asked for
    c = torch.full((M, N), float("nan"), device=DEV)
    _lib.call("cal_gemm", ta, tb, _p(a), _p(b), _p(c), _p(bias), int(with_bias), _p(ws), M, N, K, _stream())
    r = _ratio(c, ref)
    print("cal_gemm M=%d N=%d K=%d ta=%d tb=%d bias_relu=%d ws=%d ratio=%.3e" % (M, N, K, ta, tb, with_bias, n_ws, r))
    assert bool((ws[n_ws:] == CANARY).all().item()), "write past the split-K workspace"
    return r, n_ws


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_layouts_and_bounds_modes(shape):
    """Worst ratio on MI355X per shape, in the order of SHAPES: 1.6e-7, 6.2e-7, 2.2e-7, 7.8e-8, 4.7e-7."""
    for i, (ta, tb) in enumerate(LAYOUTS):
        r, n_ws = _run_gemm(*shape, ta, tb, False, 10 + i)
        assert n_ws == 0, "these shapes are single-slice launches"
        assert r < BOUND, (shape, ta, tb, r)


@pytest.mark.parametrize("shape", SHAPES_BIAS_RELU, ids=lambda s: "x".join(map(str, s)))
def test_gemm_bias_relu_epilogue(shape):
    """Worst ratio on MI355X: 1.7e-7 (68 x 72 x 64, NN)."""
    for i, (ta, tb) in enumerate(LAYOUTS):
        r, _ = _run_gemm(*shape, ta, tb, True, 20 + i)
        assert r < BOUND, (shape, ta, tb, r)


@pytest.mark.parametrize("shape", SHAPES_SPLITK, ids=lambda s: "x".join(map(str, s)))
def test_gemm_split_k_slabs_stay_inside_the_workspace(shape):
    """Worst ratio on MI355X: 2.0e-7 at K = 4096, 2.1e-7 at K = 800 (both NN)."""
    M, N, K = shape
    for i, (ta, tb) in enumerate(LAYOUTS):
        r, n_ws = _run_gemm(M, N, K, ta, tb, False, 30 + i)
        assert n_ws > 0 and n_ws % (M * N) == 0, "split-K launch expected"
        assert r < BOUND, (shape, ta, tb, r)


@pytest.mark.parametrize("shape", SHAPES_KS, ids=lambda s: "x".join(map(str, s)))
def test_gemm_ks_matches_torch(shape):
    """Worst ratio on MI355X: 2.7e-7 (70 x 40 x 200, transB, bias + ReLU)."""
    from cal_amd import _lib
    from cal_amd.plan import _p, _stream
    M, N, K = shape
    for tb in (0, 1):
        for with_bias in (False, True):
            a, b, bias, ref = _operands(M, N, K, 0, tb, with_bias, 40 + 2 * tb + int(with_bias))
            c = torch.full((M, N), float("nan"), device=DEV)
            _lib.call("cal_gemm_ks", tb, _p(a), _p(b), _p(c), _p(bias), int(with_bias), M, N, K, _stream())
            r = _ratio(c, ref)
            print("cal_gemm_ks M=%d N=%d K=%d tb=%d bias_relu=%d ratio=%.3e" % (M, N, K, tb, with_bias, r))
            assert r < BOUND, (shape, tb, with_bias, r)
