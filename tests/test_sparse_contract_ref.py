"""tests/sparse_contract_ref.py tied to what the project already trusts: oracle.cal_oracle (the reference's GCNConv, add-pool)
and torch autograd / softmax / linear, all in float64.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests import sparse_contract_ref as ref

F64 = torch.float64
TOL = dict(rtol=1e-12, atol=1e-13)


def _graph(seed=0, N=23, B=3):
    """block-diagonal batch of B random graphs with input self loops and one directed edge"""
    g = torch.Generator().manual_seed(seed)
    sizes = [N - 2 * (N // 3), N // 3, N // 3][:B]
    batch = np.repeat(np.arange(B), sizes)
    src, dst = [], []
    off = 0
    for n in sizes:
        a = torch.rand(n, n, generator=g) < 0.35
        a = a | a.t()
        a.fill_diagonal_(False)
        s, d = a.nonzero().t().numpy()
        src += list(s + off); dst += list(d + off)
        off += n
    src += [0, 5, 5]; dst += [0, 5, 5]                # input self loops (one of them twice)
    src += [1]; dst += [sizes[0] - 1]                 # directed: no reverse edge, possibly a duplicate
    perm = torch.randperm(len(src), generator=g).numpy()
    ei = np.stack([np.asarray(src)[perm], np.asarray(dst)[perm]]).astype(np.int64)
    return ei, batch, sum(sizes), g


def _oracle_dis(ei, N, w, improved):
    """deg ** -0.5 as the oracle's own gcn_norm has it: the norm of added self loop i is dis[i] * loop_w * dis[i]"""
    _, norm = O.gcn_norm(torch.from_numpy(ei), N, w, improved, F64)
    return (norm[-N:] / (2.0 if improved else 1.0)).sqrt()


@pytest.mark.parametrize("improved", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_forward_aggregation_is_gcn_conv_with_identity_weight(weighted, improved):
    ei, _, N, g = _graph(1)
    H = 12
    x = torch.randn(N, H, generator=g, dtype=F64)
    bias = torch.randn(H, generator=g, dtype=F64)
    w = (0.05 + 0.95 * torch.rand(ei.shape[1], generator=g, dtype=F64)) if weighted else None
    want = O.gcn_conv(x, torch.from_numpy(ei), torch.eye(H, dtype=F64), bias, w, improved)
    dis = _oracle_dis(ei, N, w, improved)
    ptr, nbr, eid = ref.csr_view(ei, N, 1)
    assert ptr[-1] == ei.shape[1] - 3                 # the three input self loops have no slot
    for relu in (0, 1):
        out, T, n = ref.aggregate(ptr, nbr, eid, x, dis, w, 2.0 if improved else 1.0, bias, relu)
        assert torch.allclose(out, torch.relu(want) if relu else want, **TOL)
        assert bool((T >= out.abs() - 1e-12).all()) and int(n.sum()) == ptr[-1] + N
    out, _, _ = ref.aggregate(ptr, nbr, eid, x, dis, w, 2.0 if improved else 1.0, None, 0)
    assert torch.allclose(out, want - bias, **TOL)


def _coef_forward(ei, N, z, c_e, c_n):
    """out[dst_e] += c_e z[src_e] over the edges that are no self loops, out[i] += c_n[i] z[i]"""
    keep = torch.from_numpy(ei[0] != ei[1])
    s, d = torch.from_numpy(ei[0])[keep], torch.from_numpy(ei[1])[keep]
    return torch.zeros_like(z).index_add(0, d, c_e[keep][:, None] * z[s]) + c_n[:, None] * z


@pytest.mark.parametrize("loop_w", [1.0, 2.0])
def test_transposed_aggregation_and_sddmm_are_the_autograd_gradients(loop_w):
    ei, _, N, g = _graph(2)
    H, E = 8, ei.shape[1]
    z = torch.randn(N, H, generator=g, dtype=F64, requires_grad=True)
    dout = torch.randn(N, H, generator=g, dtype=F64)
    w = 0.05 + 0.95 * torch.rand(E, generator=g, dtype=F64)
    dis = _oracle_dis(ei, N, w, loop_w == 2.0)
    c_e = (dis[torch.from_numpy(ei[0])] * w * dis[torch.from_numpy(ei[1])]).requires_grad_(True)
    c_n = (dis * dis * loop_w).requires_grad_(True)
    out = _coef_forward(ei, N, z, c_e, c_n)
    assert torch.allclose(out, O.gcn_conv(z.detach(), torch.from_numpy(ei), torch.eye(H, dtype=F64), None, w, loop_w == 2.0), **TOL)
    (out * dout).sum().backward()
    ptr, nbr, eid = ref.csr_view(ei, N, 0)            # by source: row i gathers dOut[dst]
    dz, _, _ = ref.aggregate(ptr, nbr, eid, dout, dis, w, loop_w, None, 0)
    assert torch.allclose(dz, z.grad, **TOL)
    gn, gself, gn_mag, gs_mag = ref.sddmm(ptr, nbr, eid, dout, z.detach(), E)
    loops = torch.from_numpy(ei[0] == ei[1])
    assert bool(torch.isnan(gn[loops]).all()) and int(loops.sum()) == 3
    assert torch.allclose(gn[~loops], c_e.grad[~loops], **TOL) and bool((c_e.grad[loops] == 0).all())
    assert torch.allclose(gself, c_n.grad, **TOL)
    assert bool((gn_mag[~loops] >= gn[~loops].abs() - 1e-12).all()) and bool((gs_mag >= gself.abs() - 1e-12).all())


def test_pool_backward_rows_are_autograd_through_relu_and_add_pool():
    ei, batch, N, g = _graph(3)
    H, E, B = 8, ei.shape[1], 3
    z = torch.randn(N, H, generator=g, dtype=F64, requires_grad=True)
    bias = torch.randn(H, generator=g, dtype=F64)
    gpool = torch.randn(B, H, generator=g, dtype=F64)
    w = 0.05 + 0.95 * torch.rand(E, generator=g, dtype=F64)
    dis = _oracle_dis(ei, N, w, False)
    c_e = (dis[torch.from_numpy(ei[0])] * w * dis[torch.from_numpy(ei[1])]).requires_grad_(True)
    c_n = (dis * dis).requires_grad_(True)
    act = torch.relu(_coef_forward(ei, N, z, c_e, c_n) + bias)
    pooled = O.global_add_pool(act, torch.from_numpy(batch), B)
    (pooled * gpool).sum().backward()
    rows = ref.feature_rows(act.detach(), gpool, batch)
    assert 0.2 < float((rows == 0).double().mean()) < 0.8
    ptr, nbr, eid = ref.csr_view(ei, N, 0)
    dz, _, _ = ref.aggregate(ptr, nbr, eid, rows, dis, w, 1.0, None, 0)
    assert torch.allclose(dz, z.grad, **TOL)
    gn, gself, _, _ = ref.sddmm(ptr, nbr, eid, rows, z.detach(), E)
    loops = torch.from_numpy(ei[0] == ei[1])
    assert torch.allclose(gn[~loops], c_e.grad[~loops], **TOL) and torch.allclose(gself, c_n.grad, **TOL)
    # the forward side of the same pair: per-graph sums and positive counts
    gptr = np.searchsorted(batch, np.arange(B + 1))
    s, mag, cnt, rows_per = ref.pool(act.detach(), gptr)
    assert torch.allclose(s, pooled.detach(), **TOL) and bool((mag >= s.abs() - 1e-12).all())
    assert torch.equal(cnt, O.global_add_pool((act.detach() > 0).double(), torch.from_numpy(batch), B))
    assert torch.equal(cnt, ref.pool_counts(act.detach(), batch, B)) and rows_per.tolist() == np.bincount(batch).tolist()


def test_statistics_are_column_sums():
    g = torch.Generator().manual_seed(4)
    v = torch.randn(37, 5, generator=g)
    s, q, a = ref.col_stats(v)
    assert torch.allclose(s, v.double().sum(0), **TOL) and torch.allclose(q, v.double().pow(2).sum(0), **TOL)
    assert torch.allclose(a, v.double().abs().sum(0), **TOL)


@pytest.mark.parametrize("fedge", [1.0, 0.0])
@pytest.mark.parametrize("loop_w", [1.0, 2.0])
def test_edge_attention_is_softmax_of_linear_and_its_degrees_are_gcn_norm(loop_w, fedge):
    ei, _, N, g = _graph(5)
    H, E = 6, ei.shape[1]
    x = torch.randn(N, H, generator=g, dtype=F64)
    W = torch.randn(2, 2 * H, generator=g, dtype=F64) * 0.3
    bb = torch.randn(2, generator=g, dtype=F64)
    row, col = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    want = torch.softmax(fedge * torch.nn.functional.linear(torch.cat([x[row], x[col]], -1), W, bb), -1).t()
    pq = torch.cat([x @ W[:, :H].t(), x @ W[:, H:].t()], 1)       # (x.We[0,:H], x.We[1,:H], x.We[0,H:], x.We[1,H:])
    ptr, nbr, eid = ref.csr_view(ei, N, 0)
    att, dis, deg, _ = ref.edge_attention(ptr, nbr, eid, pq, bb, fedge, loop_w, E)
    loops = row == col
    assert bool(torch.isnan(att[:, loops]).all())
    assert torch.allclose(att[:, ~loops], want[:, ~loops], **TOL)
    if fedge == 0.0:
        assert bool((att[:, ~loops] == 0.5).all())
    for k in range(2):
        assert torch.allclose(dis[k], _oracle_dis(ei, N, want[k], loop_w == 2.0), **TOL)
    assert bool((deg >= loop_w).all())
    # a node without out-edges and loop_w = 0: degree 0 -> dis 0, not inf
    ptr0 = np.zeros(3, np.int32)
    _, dis0, _, _ = ref.edge_attention(ptr0, np.zeros(0, np.int32), np.zeros(0, np.int32), pq[:2], bb, 1.0, 0.0, 1)
    assert bool((dis0 == 0).all())
