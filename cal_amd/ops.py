"""autograd wrappers around the C-ABI entry points (operator-level boundary).

Every Function hands its tensors to ``plan._c``, which calls straight into the
C ABI: CUDA tensors -> libcalhip.so (HIP kernels, torch's current stream), CPU
tensors -> libcalhost.so (the plain-C++ host implementation of the same
symbols).  Tensors of one call must live on one device.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from . import _lib
from .plan import GraphPlan, _c, _q


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    return t.contiguous()


def _empty(n: int, dev) -> torch.Tensor:
    return torch.empty(max(int(n), 4), dtype=torch.float32, device=dev)


class _GCNAggregate(Function):
    """norm + propagate + bias (+ReLU): gcn_conv.py:79-104 after the dense x @ W."""

    @staticmethod
    def forward(ctx, h, w, bias, plan: GraphPlan, loop_w: float, relu: bool):
        h = _f32(h, "h")
        N, H = h.shape
        if N != plan.N:
            raise ValueError("feature rows (%d) != plan nodes (%d)" % (N, plan.N))
        if w is None:
            dis, norm = plan.unit_norm(loop_w)
        else:
            w = _f32(w, "edge_weight").view(-1)
            if w.numel() != plan.E:
                raise AssertionError("edge_weight.size(0) != edge_index.size(1)")   # gcn_conv.py:54
            dis, norm = _empty(N, h.device), _empty(plan.E, h.device)
            _c("cal_gcn_norm_fwd", plan.rowptr_src, plan.eid_src, plan.row32, plan.col32,
                      w, loop_w, N, plan.E, dis, norm)
        if bias is not None:
            bias = _f32(bias, "bias")
        out = torch.empty_like(h)
        _c("cal_spmm_fwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, norm, dis,
                  loop_w, h, bias, int(relu), out, N, H)
        ctx.plan, ctx.loop_w, ctx.relu, ctx.has_bias = plan, loop_w, relu, bias is not None
        ctx.has_w = w is not None
        need_h = ctx.has_w and ctx.needs_input_grad[1]
        ctx.save_for_backward(h if need_h else None, w, dis, norm, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, w, dis, norm, out = ctx.saved_tensors
        plan, loop_w = ctx.plan, ctx.loop_w
        gout = _f32(gout, "grad_out")
        N, H = gout.shape
        dev = gout.device
        need_bias = ctx.has_bias and ctx.needs_input_grad[2]
        dz = torch.empty_like(gout) if ctx.relu else gout
        dbias = torch.empty(H, dtype=torch.float32, device=dev) if need_bias else None
        if ctx.relu or need_bias:
            part = _empty(_q(gout, "cal_colsum_parts", N) * H, dev) if need_bias else None
            _c("cal_relu_bwd_colsum", gout, out if ctx.relu else None,
                      dz if ctx.relu else None, dbias, part, N, H)
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty_like(gout)
            _c("cal_spmm_fwd", plan.rowptr_src, plan.nbr_src, plan.eid_src, norm, dis,
                      loop_w, dz, None, 0, dh, N, H)
        dw = None
        if ctx.has_w and ctx.needs_input_grad[1]:
            dw = _empty(plan.E, dev)[:plan.E]
            gn, gself, ddeg = _empty(plan.E, dev), _empty(N, dev), _empty(N, dev)
            _c("cal_gcn_norm_bwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst,
                      plan.rowptr_src, plan.nbr_src, plan.eid_src, plan.row32, plan.col32,
                      w, dis, loop_w, h, dz, gn, gself, ddeg, dw,
                      N, plan.E, H)
        return dh, dw, dbias, None, None, None


def gcn_aggregate(h, plan: GraphPlan, edge_weight=None, bias=None, improved: bool = False,
                  relu: bool = False):
    return _GCNAggregate.apply(h, edge_weight, bias, plan, 2.0 if improved else 1.0, relu)


class _EdgeAttention(Function):
    """model.py:97-104 -> [2, E] (row 0: edge_weight_c, row 1: edge_weight_o)."""

    @staticmethod
    def forward(ctx, x, W, b, plan: GraphPlan):
        x, W, b = _f32(x, "x"), _f32(W, "edge_att_mlp.weight"), _f32(b, "edge_att_mlp.bias")
        N, H = x.shape
        if W.shape != (2, 2 * H):
            raise ValueError("edge_att_mlp.weight must be [2, 2*hidden]")
        att = _empty(2 * plan.E, x.device)[:2 * plan.E].view(2, plan.E)
        pq = _empty(4 * N, x.device)
        _c("cal_edge_att_fwd", x, W, b, plan.row32, plan.col32, pq, att,
                  N, plan.E, H)
        ctx.plan = plan
        ctx.save_for_backward(x, W, att)
        return att

    @staticmethod
    def backward(ctx, datt):
        x, W, att = ctx.saved_tensors
        plan = ctx.plan
        datt = _f32(datt, "grad")
        N, H = x.shape
        dx = torch.empty_like(x)
        dW = torch.empty_like(W)
        db = torch.empty(2, dtype=torch.float32, device=x.device)
        ws = _empty(_q(x, "cal_edge_att_bwd_ws", N, plan.E, H), x.device)
        _c("cal_edge_att_bwd", x, W, att, datt, plan.rowptr_src, plan.eid_src,
                  plan.rowptr_dst, plan.eid_dst, dx, 0, dW, db, ws, N, plan.E, H)
        return dx, dW, db, None


def edge_attention(x, weight, bias, plan: GraphPlan):
    return _EdgeAttention.apply(x, weight, bias, plan)


class _NodeAttentionSplit(Function):
    """model.py:106-111 -> (xc, xo, node_att)."""

    @staticmethod
    def forward(ctx, x, Wn, bn):
        x, Wn, bn = _f32(x, "x"), _f32(Wn, "node_att_mlp.weight"), _f32(bn, "node_att_mlp.bias")
        N, H = x.shape
        att = _empty(2 * N, x.device)[:2 * N].view(N, 2)
        xc, xo = torch.empty_like(x), torch.empty_like(x)
        _c("cal_node_att_split_fwd", x, Wn, bn, att, xc, xo, N, H)
        ctx.save_for_backward(x, Wn, att)
        ctx.mark_non_differentiable(att)
        return xc, xo, att

    @staticmethod
    def backward(ctx, dxc, dxo, _datt):
        x, Wn, att = ctx.saved_tensors
        N, H = x.shape
        dxc = torch.zeros_like(x) if dxc is None else _f32(dxc, "grad_xc")
        dxo = torch.zeros_like(x) if dxo is None else _f32(dxo, "grad_xo")
        dx, dWn = torch.empty_like(x), torch.empty_like(Wn)
        dbn = torch.empty(2, dtype=torch.float32, device=x.device)
        ws = _empty(_q(x, "cal_node_att_bwd_ws", N, H), x.device)
        _c("cal_node_att_split_bwd", x, Wn, att, dxc, dxo, dx, dWn, dbn,
                  ws, N, H)
        return dx, dWn, dbn


def node_attention_split(x, weight, bias):
    return _NodeAttentionSplit.apply(x, weight, bias)


class _AddPool(Function):
    """global_add_pool (model.py:115-116)."""

    @staticmethod
    def forward(ctx, x, plan: GraphPlan):
        x = _f32(x, "x")
        N, H = x.shape
        B, S = plan.B, plan.pool_splits()
        out = torch.empty(B, H, dtype=torch.float32, device=x.device)
        part = _empty(S * B * H, x.device) if S > 1 else None
        _c("cal_add_pool_fwd", x, plan.gptr, out, part, B, H, S)
        ctx.plan, ctx.N = plan, N
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _f32(dout, "grad")
        H = dout.size(1)
        dx = torch.empty(ctx.N, H, dtype=torch.float32, device=dout.device)
        _c("cal_add_pool_bwd", dout, ctx.plan.batch, dx, ctx.N, H)
        return dx, None


def add_pool(x, plan: GraphPlan):
    if plan.batch is None:
        raise ValueError("plan was built without a batch vector")
    return _AddPool.apply(x, plan)


class _GATAggregate(Function):
    """GATConv after z = x @ W: scores, edge softmax, dropout, aggregation, bias (+ReLU)."""

    @staticmethod
    def forward(ctx, z, att, bias, plan: GraphPlan, heads: int, slope: float, p: float, seed: int,
                relu: bool):
        z, att = _f32(z, "z"), _f32(att, "att")
        N, H = z.shape
        K = int(heads)
        D = H // K
        if att.numel() != K * 2 * D:
            raise ValueError("att must have heads * 2 * out_channels elements")
        if bias is not None:
            bias = _f32(bias, "bias")
        dev = z.device
        out = torch.empty_like(z)
        adst, asrc, mx, den = (_empty(N * K, dev) for _ in range(4))
        _c("cal_gat_fwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, z, att, bias,
                  int(relu), slope, p, seed, out, adst, asrc, mx, den, N, plan.E, K, D)
        ctx.plan, ctx.K, ctx.D, ctx.slope, ctx.p, ctx.seed, ctx.relu = plan, K, D, slope, p, seed, relu
        ctx.has_bias = bias is not None
        ctx.att_shape = att.shape
        ctx.save_for_backward(z, att, adst, asrc, mx, den, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        z, att, adst, asrc, mx, den, out = ctx.saved_tensors
        plan, K, D = ctx.plan, ctx.K, ctx.D
        gout = _f32(gout, "grad")
        N, H = gout.shape
        dev = gout.device
        need_bias = ctx.has_bias and ctx.needs_input_grad[2]
        g = torch.empty_like(gout) if ctx.relu else gout
        dbias = torch.empty(H, dtype=torch.float32, device=dev) if need_bias else None
        if ctx.relu or need_bias:
            part = _empty(_q(gout, "cal_colsum_parts", N) * H, dev) if need_bias else None
            _c("cal_relu_bwd_colsum", gout, out if ctx.relu else None,
                      g if ctx.relu else None, dbias, part, N, H)
        dz = torch.empty_like(gout)
        datt = torch.empty(K * 2 * D, dtype=torch.float32, device=dev)
        ws = _empty(_q(gout, "cal_gat_bwd_ws", N, plan.E, K, D), dev)
        _c("cal_gat_bwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, plan.rowptr_src,
                  plan.nbr_src, plan.eid_src, z, att, adst, asrc, mx, den, g,
                  ctx.slope, ctx.p, ctx.seed, dz, datt, ws, N, plan.E, K, D)
        return dz, datt.view(ctx.att_shape), dbias, None, None, None, None, None, None


class _GATMaskAggregate(Function):
    """GATConv after z = x @ W with a mask ``m`` [E] >= 0 by edge column inside the edge softmax (no dropout):
    ``alpha_ij = m_ij exp(s_ij - max_i) / (sum_k m_ik exp(s_ik - max_i) + 1e-16)``, the added loop at weight 1, ``max_i`` over the
    loop and the columns with ``m > 0`` and a constant in the backward.  Differentiable in ``z`` and ``m``; ``att`` and ``bias``
    are frozen on this path (``cal_amd.gradient``): a backward with either requiring grad raises."""

    @staticmethod
    def forward(ctx, z, att, bias, m, plan: GraphPlan, heads: int, slope: float, relu: bool):
        z, att, m = _f32(z, "z"), _f32(att, "att"), _f32(m, "edge_mask").view(-1)
        N, H = z.shape
        K = int(heads)
        D = H // K
        if att.numel() != K * 2 * D:
            raise ValueError("att must have heads * 2 * out_channels elements")
        if N != plan.N:
            raise ValueError("feature rows (%d) != plan nodes (%d)" % (N, plan.N))
        if m.numel() != plan.E:
            raise ValueError("edge_mask must have one entry per edge column (%d, got %d)" % (plan.E, m.numel()))
        if bias is not None:
            bias = _f32(bias, "bias")
        dev = z.device
        out = torch.empty_like(z)
        adst, asrc, mx, den = (_empty(N * K, dev) for _ in range(4))
        _c("cal_gat_mask_fwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, z, att, bias, int(relu), slope, m,
                  out, adst, asrc, mx, den, N, plan.E, K, D)
        ctx.plan, ctx.K, ctx.D, ctx.slope, ctx.relu = plan, K, D, slope, relu
        ctx.save_for_backward(z, att, m, adst, asrc, mx, den, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise RuntimeError("the masked GATConv has no gradient for att / bias: freeze the parameters (cal_amd.gradient does)")
        z, att, m, adst, asrc, mx, den, out = ctx.saved_tensors
        plan, K, D = ctx.plan, ctx.K, ctx.D
        gout = _f32(gout, "grad")
        N, H = gout.shape
        dev = gout.device
        g = gout
        if ctx.relu:
            g = torch.empty_like(gout)
            _c("cal_relu_bwd_colsum", gout, out, g, None, None, N, H)
        dz = torch.empty_like(gout)
        dm = _empty(plan.E, dev)[:plan.E]
        ws = _empty(_q(gout, "cal_gat_mask_bwd_ws", N, plan.E, K, D), dev)
        _c("cal_gat_mask_bwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, plan.rowptr_src, plan.nbr_src, plan.eid_src,
                  z, att, adst, asrc, mx, den, g, ctx.slope, m, dz, dm, ws, N, plan.E, K, D)
        return dz, None, None, dm, None, None, None, None


def gat_aggregate(z, att, bias, plan: GraphPlan, heads: int, negative_slope: float = 0.2,
                  dropout: float = 0.0, seed: int = 0, relu: bool = False, edge_mask=None):
    if edge_mask is not None:
        if dropout > 0:
            raise ValueError("a GAT edge mask does not go through attention dropout")
        return _GATMaskAggregate.apply(z, att, bias, edge_mask, plan, heads, negative_slope, relu)
    return _GATAggregate.apply(z, att, bias, plan, heads, negative_slope, dropout, seed, relu)


def gat_dropout_mask(seed: int, plan: GraphPlan, heads: int, p: float) -> torch.Tensor:
    """The keep mask ([E + N, heads] of 0/1) the kernels derive from ``seed`` (for tests)."""
    m = torch.empty(plan.E + plan.N, heads, dtype=torch.float32, device=plan.device)
    _c("cal_gat_dropout_mask", seed, plan.E, plan.N, heads, p, m)
    return m


class _Linear(Function):
    """Dense layer on the fp32 MFMA GEMM (cal_gemm): y = x @ W (+b) for a GCN-style weight
    [in, out] (gcn_conv.py:75) or y = x @ W^T (+b) for an nn.Linear weight [out, in]
    (model.py:46-75), optional fused ReLU."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_in: bool, relu: bool):
        x, weight = _f32(x, "x"), _f32(weight, "weight")
        M, K = x.shape
        N = weight.size(0) if out_in else weight.size(1)
        if (weight.size(1) if out_in else weight.size(0)) != K:
            raise ValueError("weight shape does not match the input width")
        if bias is not None:
            bias = _f32(bias, "bias")
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        _c("cal_gemm", 0, 1 if out_in else 0, x, weight, y, bias, int(relu), None, M, N, K)
        ctx.out_in, ctx.relu, ctx.has_bias = out_in, relu, bias is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gy = _f32(gy, "grad")
        M, N = gy.shape
        K = x.size(1)
        dev = gy.device
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        g = torch.empty_like(gy) if ctx.relu else gy
        db = torch.empty(N, dtype=torch.float32, device=dev) if need_b else None
        if ctx.relu or need_b:
            part = _empty(_q(gy, "cal_colsum_parts", M) * N, dev) if need_b else None
            _c("cal_relu_bwd_colsum", gy, y if ctx.relu else None, g if ctx.relu else None,
                      db, part, M, N)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=torch.float32, device=dev)
            # out_in: dx = g @ W ([N,K] as stored);  else dx = g @ W^T (W stored [K,N])
            _c("cal_gemm", 0, 0 if ctx.out_in else 1, g, weight, dx, None, 0, None, M, K, N)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            if ctx.out_in:      # dW [N,K] = g^T @ x
                ws = _empty(_q(gy, "cal_gemm_ws", N, K, M), dev)
                _c("cal_gemm", 1, 0, g, x, dw, None, 0, ws, N, K, M)
            else:               # dW [K,N] = x^T @ g
                ws = _empty(_q(gy, "cal_gemm_ws", K, N, M), dev)
                _c("cal_gemm", 1, 0, x, g, dw, None, 0, ws, K, N, M)
        return dx, dw, db, None, None


def linear(x, weight, bias=None, relu: bool = False):
    """nn.Linear semantics (weight [out, in]) on the MFMA GEMM."""
    return _Linear.apply(x, weight, bias, True, relu)


def matmul(x, weight, relu: bool = False):
    """x @ weight with weight [in, out] (gcn_conv.py:75) on the MFMA GEMM."""
    return _Linear.apply(x, weight, None, False, relu)


class _GINAggregate(Function):
    """PyG GINConv's aggregation, (1 + eps) * x + sum_{j -> i} x_j (self loops of the input dropped),
    on the CSR aggregation kernel with unit coefficients (call site model.py:188)."""

    @staticmethod
    def forward(ctx, x, plan: GraphPlan, eps: float):
        x = _f32(x, "x")
        N, H = x.shape
        ones_n, ones_e = plan.ones()
        out = torch.empty_like(x)
        _c("cal_spmm_fwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, ones_e, ones_n,
                  1.0 + eps, x, None, 0, out, N, H)
        ctx.plan, ctx.eps = plan, eps
        return out

    @staticmethod
    def backward(ctx, g):
        g = _f32(g, "grad")
        N, H = g.shape
        plan = ctx.plan
        ones_n, ones_e = plan.ones()
        dx = torch.empty_like(g)
        _c("cal_spmm_fwd", plan.rowptr_src, plan.nbr_src, plan.eid_src, ones_e, ones_n,
                  1.0 + ctx.eps, g, None, 0, dx, N, H)
        return dx, None, None


class _GINWeightedAggregate(Function):
    """(1 + eps) * x_i + sum_{j -> i} w_ji x_j with a weight per edge column (self loops of the input dropped): forward and dx on the
    CSR aggregation kernel with norm = w, dis = 1, loop_w = 1 + eps; d w_e = <g[col_e], x[row_e]> by ``cal_edge_dot``."""

    @staticmethod
    def forward(ctx, x, w, plan: GraphPlan, eps: float):
        x, w = _f32(x, "x"), _f32(w, "edge_weight").view(-1)
        N, H = x.shape
        if N != plan.N:
            raise ValueError("feature rows (%d) != plan nodes (%d)" % (N, plan.N))
        if w.numel() != plan.E:
            raise ValueError("edge_weight must have one entry per edge column (%d, got %d)" % (plan.E, w.numel()))
        ones_n = plan.ones()[0]
        wk = w if plan.E else plan.ones()[1]
        out = torch.empty_like(x)
        _c("cal_spmm_fwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, wk, ones_n, 1.0 + eps, x, None, 0, out, N, H)
        ctx.plan, ctx.eps = plan, eps
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, wk)
        return out

    @staticmethod
    def backward(ctx, g):
        x, wk = ctx.saved_tensors
        g = _f32(g, "grad")
        N, H = g.shape
        plan = ctx.plan
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(g)
            _c("cal_spmm_fwd", plan.rowptr_src, plan.nbr_src, plan.eid_src, wk, plan.ones()[0], 1.0 + ctx.eps, g, None, 0, dx, N, H)
        if ctx.needs_input_grad[1]:
            dw = _empty(plan.E, g.device)[:plan.E]
            _c("cal_edge_dot", plan.row32, plan.col32, g, x, dw, N, plan.E, H)
        return dx, dw, None, None


def gin_aggregate(x, plan: GraphPlan, eps: float = 0.0, edge_weight=None):
    if edge_weight is not None:
        return _GINWeightedAggregate.apply(x, edge_weight, plan, eps)
    return _GINAggregate.apply(x, plan, eps)


class _NodeMaskColumns(Function):
    """n [N] -> n[row_e] * n[col_e] per edge column: what a node mask puts on the columns.  The backward gathers over the plan's two
    CSR views (the aggregation kernel at width 1), so it has a fixed summation order; a self-loop column, which no convolution
    reads, sends nothing back."""

    @staticmethod
    def forward(ctx, n, plan: GraphPlan):
        n = _f32(n, "node_mask").view(-1)
        if n.numel() != plan.N:
            raise ValueError("node_mask must have one entry per node (%d, got %d)" % (plan.N, n.numel()))
        ctx.plan = plan
        ctx.save_for_backward(n)
        if plan.E == 0:
            return n.new_empty(0)
        return n[plan.row32.long()] * n[plan.col32.long()]

    @staticmethod
    def backward(ctx, g):
        (n,) = ctx.saved_tensors
        plan = ctx.plan
        N = plan.N
        if plan.E == 0 or N == 0:
            return torch.zeros_like(n), None
        g = _f32(g, "grad")
        h = n.view(N, 1)
        ones_n = plan.ones()[0]
        a, b = torch.empty_like(h), torch.empty_like(h)
        _c("cal_spmm_fwd", plan.rowptr_src, plan.nbr_src, plan.eid_src, g, ones_n, 0.0, h, None, 0, a, N, 1)
        _c("cal_spmm_fwd", plan.rowptr_dst, plan.nbr_dst, plan.eid_dst, g, ones_n, 0.0, h, None, 0, b, N, 1)
        return (a + b).view(-1), None


def node_mask_columns(n, plan: GraphPlan):
    return _NodeMaskColumns.apply(n, plan)


class _EdgeMlpMask(Function):
    """The parametric explainer's edge MLP on the node projections ``pq`` [N, 2 Hd] (``cal_edge_mlp_fwd`` / ``_bwd``, include/cal_hip.h)
    -> ``(mask [E], terms [B, 2], omega [P], z [P])``; only ``mask`` carries a gradient.  The backward takes ``dmask``, adds the
    gradients of ``l_size * sum m + l_ent / P_g * sum H(m)`` in closed form and returns ``dpq, dw2, db2``."""

    @staticmethod
    def forward(ctx, pq, w2, b2, plan: GraphPlan, players, tau: float, seed: int, step: int, l_size: float, l_ent: float):
        pq, w2, b2 = _f32(pq, "pq"), _f32(w2, "w2"), _f32(b2, "b2")
        if pq.dim() != 2 or pq.size(0) != plan.N or pq.size(1) % 2:
            raise ValueError("pq must be [nodes (%d), 2 * hidden]" % plan.N)
        N, Hd = plan.N, pq.size(1) // 2
        if Hd < 4 or Hd > 256 or Hd % 4:
            raise ValueError("the hidden width must be a multiple of 4 in [4, 256] (got %d)" % Hd)
        if w2.numel() != Hd or b2.numel() != 1:
            raise ValueError("w2 must have one entry per hidden unit (%d) and b2 one" % Hd)
        if players.E != plan.E:
            raise ValueError("the players belong to another batch (%d columns, the plan has %d)" % (players.E, plan.E))
        dev, B, P = pq.device, players.B, players.P
        mask = torch.ones(plan.E, dtype=torch.float32, device=dev)
        terms = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        omega, z = torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.float32, device=dev)
        _c("cal_edge_mlp_fwd", pq, w2, b2, plan.row32, plan.col32, players.pptr, players.rep, players.mate, omega, z, mask, terms,
           N, plan.E, Hd, B, P, tau, seed, step)
        ctx.plan, ctx.players, ctx.tau, ctx.l_size, ctx.l_ent = plan, players, tau, l_size, l_ent
        ctx.shapes = (w2.shape, b2.shape)
        ctx.save_for_backward(pq, w2, z)
        ctx.mark_non_differentiable(terms, omega, z)
        return mask, terms, omega, z

    @staticmethod
    def backward(ctx, dmask, _dterms, _domega, _dz):
        pq, w2, z = ctx.saved_tensors
        plan, players = ctx.plan, ctx.players
        dev, N, Hd = pq.device, plan.N, w2.numel()
        gmask = torch.zeros(plan.E, dtype=torch.float32, device=dev) if dmask is None else _f32(dmask, "grad")
        if players.B == 0 or players.P == 0:                    # (the entry point launches nothing)
            return torch.zeros_like(pq), torch.zeros(ctx.shapes[0], device=dev), torch.zeros(ctx.shapes[1], device=dev), \
                None, None, None, None, None, None, None
        dpq = torch.empty_like(pq)
        dw2, db2 = torch.empty(Hd, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
        ws = _empty(_q(pq, "cal_edge_mlp_bwd_ws", N, plan.E, Hd), dev)
        rs, es, rd, ed = players.csr(plan)
        _c("cal_edge_mlp_bwd", pq, w2, plan.row32, plan.col32, rs, es, rd, ed, players.pptr, players.rep, players.mate, z, gmask,
           dpq, dw2, db2, ws, N, plan.E, Hd, players.B, players.P, ctx.tau, ctx.l_size, ctx.l_ent)
        return dpq, dw2.view(ctx.shapes[0]), db2.view(ctx.shapes[1]), None, None, None, None, None, None, None


def edge_mlp_mask(pq, w2, b2, plan: GraphPlan, players, tau: float = 1.0, seed: int = 0, step: int = 0, size_coeff: float = 0.0,
                  ent_coeff: float = 0.0, full: bool = False):
    """``(mask float32 [E], terms fp64 [B, 2])`` of the edge MLP over ``players`` (``cal_amd.pgexplain.EdgePlayers``: ``pptr`` /
    ``rep`` / ``mate`` and the two CSRs); ``full``: also ``omega`` and ``z`` [P].  ``mask`` is 1 outside the players.  ``seed = 0``:
    no noise."""
    out = _EdgeMlpMask.apply(pq, w2, b2, plan, players, float(tau), int(seed), int(step), float(size_coeff), float(ent_coeff))
    return out if full else out[:2]
