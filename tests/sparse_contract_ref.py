"""Float64 restatement of the node-level sparse operations of csrc/engine_kernels.hpp (k_espmm in its six kinds,
k_edge_att_deg, k_pool2 / k_pool2_sum, k_pool_cnt), written from their definitions over the slots of a CSR view, with the
magnitude sums the error bounds of tests/test_gpu_sparse_contract.py need.  tests/test_sparse_contract_ref.py ties it to
oracle.cal_oracle and to torch autograd.  Everything is torch float64 on the device of the operands (the CPU test runs it on the
CPU, the GPU test where the kernels' operands already are); index arrays are numpy.

A CSR view of edge_index [2, E] by key k (1: by destination, 0: by source): the edges without input self loops, stably sorted
by edge_index[k]; row i owns the slots [ptr[i], ptr[i + 1]), slot s gathers node nbr[s] = edge_index[1 - k][eid[s]].
"""
import numpy as np
import torch

F64 = torch.float64


def csr_view(edge_index, N, key):
    """-> ptr [N + 1], nbr [nnz], eid [nnz] (int32 numpy): stable sort by edge_index[key], self loops dropped"""
    ei = np.asarray(edge_index)
    eids = np.nonzero(ei[0] != ei[1])[0]
    order = eids[np.argsort(ei[key][eids], kind="stable")]
    ptr = np.zeros(N + 1, np.int64)
    np.add.at(ptr, ei[key][eids] + 1, 1)
    return np.cumsum(ptr).astype(np.int32), ei[1 - key][order].astype(np.int32), order.astype(np.int32)


def slot_rows(ptr, device="cpu"):
    """row of every slot"""
    ptr = np.asarray(ptr, np.int64)
    return torch.from_numpy(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))).to(device)


def _idx(a, device="cpu"):
    return torch.from_numpy(np.asarray(a, np.int64)).to(device)


def feature_rows(h, pb_g=None, pb_batch=None):
    """row(v): h[v], or with the add-pool backward folded in where(h[v] > 0, pb_g[pb_batch[v]], 0)"""
    h = h.to(F64)
    if pb_g is None:
        return h
    g = pb_g.to(F64)[_idx(pb_batch, h.device)]
    return torch.where(h > 0, g, torch.zeros_like(g))


def aggregate(ptr, nbr, eid, rows, dis, w, loop_w, bias, relu):
    """pre[i] = dis[i] (sum_s dis[nbr[s]] w[eid[s]] row(nbr[s]) + dis[i] loop_w row(i)) + bias; out = relu(pre) or pre.
    -> out, T (the same sum over absolute values, the scale of the fp32 error bound), n (terms per row: slots + 1)"""
    rows, dis = rows.to(F64), dis.to(F64)
    dev = rows.device
    ri, nb = slot_rows(ptr, dev), _idx(nbr, dev)
    coef = dis[nb] * (w.to(F64)[_idx(eid, dev)] if w is not None else 1.0)
    acc = torch.zeros_like(rows).index_add_(0, ri, coef[:, None] * rows[nb])
    mag = torch.zeros_like(rows).index_add_(0, ri, coef.abs()[:, None] * rows[nb].abs())
    own = (dis * loop_w)[:, None]
    pre = dis[:, None] * (acc + own * rows)
    T = dis[:, None] * (mag + own * rows.abs())
    if bias is not None:
        pre = pre + bias.to(F64)
        T = T + bias.to(F64).abs()
    n = _idx(np.diff(np.asarray(ptr, np.int64)), dev) + 1
    return (torch.relu(pre) if relu else pre), T, n


def sddmm(ptr, nbr, eid, rows, z, E):
    """gn[eid[s]] = <row(nbr[s]), z[i]> for the slots s of row i (NaN where an edge has no slot), gself[i] = <row(i), z[i]>;
    -> gn, gself, and the sums of |a_k b_k| behind them"""
    rows, z = rows.to(F64), z.to(F64)
    dev = rows.device
    ri, nb, ed = slot_rows(ptr, dev), _idx(nbr, dev), _idx(eid, dev)
    gn = torch.full((E,), float("nan"), dtype=F64, device=dev)
    gn_mag = torch.zeros(E, dtype=F64, device=dev)
    gn[ed] = (rows[nb] * z[ri]).sum(1)
    gn_mag[ed] = (rows[nb] * z[ri]).abs().sum(1)
    return gn, (rows * z).sum(1), gn_mag, (rows * z).abs().sum(1)


def col_stats(out):
    """column sums of out and out^2 with their magnitude sums (sum |v|, sum v^2)"""
    v = out.to(F64)
    return v.sum(0), (v * v).sum(0), v.abs().sum(0)


def edge_attention(ptr, nbr, eid, pq, be, fedge, loop_w, E):
    """by-source CSR.  att[:, e] = softmax2(fedge (pq[src, 0:2] + pq[dst, 2:4] + be)) on the slotted edges (NaN elsewhere),
    dis_k[v] = (loop_w + sum of att[k] over the slots of v) ** -0.5, 0 where that degree is 0.
    -> att [2, E], dis [2, N], deg [2, N], logits [nnz, 2]"""
    pq, be = pq.to(F64), be.to(F64)
    dev = pq.device
    ri, nb, ed = slot_rows(ptr, dev), _idx(nbr, dev), _idx(eid, dev)
    logits = fedge * (pq[ri, 0:2] + pq[nb, 2:4] + be)
    a = torch.softmax(logits, -1)
    att = torch.full((2, E), float("nan"), dtype=F64, device=dev)
    att[:, ed] = a.t()
    N = len(ptr) - 1
    deg = torch.full((2, N), float(loop_w), dtype=F64, device=dev).index_add_(1, ri, a.t().contiguous())
    dis = torch.where(deg == 0, torch.zeros_like(deg), deg.clamp_min(1e-300) ** -0.5)
    return att, dis, deg, logits


def pool(h, gptr):
    """per graph b = rows [gptr[b], gptr[b + 1]): column sums, sums of |x|, counts of entries > 0, rows"""
    h = h.to(F64)
    gptr = np.asarray(gptr, np.int64)
    B = len(gptr) - 1
    bi = _idx(np.repeat(np.arange(B), np.diff(gptr)), h.device)
    z = torch.zeros(B, h.shape[1], dtype=F64, device=h.device)
    rows = h[int(gptr[0]):int(gptr[-1])]
    return (z.clone().index_add_(0, bi, rows), z.clone().index_add_(0, bi, rows.abs()),
            z.clone().index_add_(0, bi, (rows > 0).to(F64)), _idx(np.diff(gptr), h.device))


def pool_counts(h, batch, B):
    """counts of entries > 0 per graph of a node -> graph map (any layout)"""
    return torch.zeros(B, h.shape[1], dtype=F64, device=h.device).index_add_(0, _idx(batch, h.device), (h > 0).to(F64))
