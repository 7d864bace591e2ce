"""Model-level explanations: Weisfeiler-Lehman signatures of subgraphs, and the census of explanation shapes per class.

Every other explanation method of the package answers an instance-level question -- which edges of *this* graph the model calls
causal.  This module answers the dataset-level one: for class c, which subgraph does the model rely on?  It needs a canonical,
order-independent signature of a subgraph, computed on the device for a whole batch of extracted explanations:

* ``wl_refine(data, iters=3, labels=...)`` -> ``WLColors``: 1-WL colour refinement of every graph of a batch in 64-bit integers
  (``cal_wl_refine``: one launch on the GPU, libcalhost for CPU tensors).  ``hash[g, t]`` is invariant under node relabelling and
  column order and does not depend on the rest of the batch.  Equal hashes mean *WL-equivalent*, not *isomorphic*: a 6-cycle and
  two triangles get the same hash at every depth.
* ``wl_match(a, protos)`` / ``wl_similarity(a, protos)``: the WL subtree kernel of every graph against a few prototype graphs
  (``cal_wl_match``: one launch) and its cosine normalisation.
* ``subgraph_census`` / ``explanation_census`` (also ``model.explanation_census``) / ``eval_explanation_census``: extract the
  explanation subgraphs, hash them, count the shapes per class and compare them with prototypes (``spmotif.motif_batch``).
"""
from __future__ import annotations

import struct
from collections import namedtuple

import torch

from . import _lib
from .explain import _eval_mode, _Layout, _log_probs, explain, extract_subgraph
from .plan import _p, _stream

__all__ = ["WLColors", "wl_refine", "wl_match", "wl_similarity", "subgraph_census", "explanation_census",
           "eval_explanation_census", "C_INIT", "C_SELF", "C_OUT", "C_IN", "C_NODE", "C_GRAPH"]

#: the constants of the operator (``CAL_WL_C_*``)
C_INIT = 0xD6E8FEB86659FD93
C_SELF = 0xC2B2AE3D27D4EB4F
C_OUT = 0x165667B19E3779F9
C_IN = 0x27D4EB2F165667C5
C_NODE = 0x85EBCA77C2B2AE63
C_GRAPH = 0xFF51AFD7ED558CCD

#: ``colors`` int64 [T + 1, N] (row t: the colours after t rounds), ``hash`` int64 [B, T + 1] (cumulative over the depths), ``ptr``
#: int64 [B + 1], ``ignored`` (int64 [1] on the device, not read back: the columns with an endpoint outside their graph) and the
#: host int ``max_nodes``.  The int64s carry uint64 bit patterns: compare them for equality only.
WLColors = namedtuple("WLColors", "colors hash ptr ignored max_nodes")


def _initial_labels(data, labels, N: int, dev):
    if labels is None:
        return None
    if isinstance(labels, str):
        if labels != "argmax":
            raise ValueError('labels must be None, "argmax" or an int64 tensor [N]')
        x = data.x if getattr(data, "x", None) is not None else getattr(data, "feat", None)
        if x is None or x.dim() != 2 or int(x.size(0)) != N or int(x.size(1)) < 1:
            raise ValueError('labels="argmax" needs features [N, F], F >= 1')
        return x.argmax(1).to(device=dev, dtype=torch.long).contiguous()
    t = torch.as_tensor(labels)
    if t.dim() != 1 or int(t.numel()) != N or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("labels must be a 1-D integer tensor with one entry per node")
    return t.to(device=dev, dtype=torch.long).contiguous()


def wl_refine(data, *, iters: int = 3, labels=None) -> WLColors:
    """1-WL colour refinement of every graph of the batch ``data``, ``iters`` = T rounds (``cal_wl_refine``; the definitions are
    in ``include/cal_hip.h``).

    ``labels``: the initial node labels -- ``None`` (all equal: pure structure), ``"argmax"`` (the argmax of every feature row: the
    one-hot node labels of TU data) or an int64 tensor [N].  A column counts iff both endpoints lie in its graph; self loops and
    duplicates count with multiplicity; direction matters (a batch that stores both directions of every edge is symmetric anyway).
    A batch whose columns are not grouped by graph is reordered by graph first, as ``extract_subgraph`` does; the result does not
    depend on the column order.  CUDA tensors: one launch on the current stream, no read-back; CPU tensors: libcalhost.  Both
    give the same bits."""
    T = int(iters)
    if not 0 <= T <= 4096:
        raise ValueError("iters must be in [0, 4096]")
    ei = data.edge_index
    dev, host = ei.device, not ei.is_cuda
    lay = _Layout(data)
    if lay.order is not None:
        ei = ei[:, lay.order]
    ei = ei.to(torch.long).contiguous()
    B, E, N = lay.B, int(ei.size(1)), int(data.batch.numel())
    init = _initial_labels(data, labels, N, dev)
    ptr, eptr = lay.ptr.to(torch.long).contiguous(), lay.edge_ptr.to(torch.long).contiguous()
    cap = _lib.query("cal_explain_lds_cap", host=host)
    wsb = _lib.query("cal_wl_ws", N, E, B, host=host) if lay.max_nodes > cap else 0
    sizes = ((T + 1) * N, B * (T + 1), 1, (wsb + 7) // 8)
    colors, hsh, ignored, ws = torch.split(torch.empty(sum(sizes), dtype=torch.long, device=dev), sizes)
    _lib.call("cal_wl_refine", _p(ei) if E else None, E, N, _p(ptr), _p(eptr), B, _p(init) if N else None, T, int(lay.max_nodes),
              _p(colors) if N else None, _p(hsh), _p(ignored), _p(ws) if wsb else None, 8 * sizes[-1],
              None if host else _stream(), host=host)
    return WLColors(colors.view(T + 1, N), hsh.view(B, T + 1), ptr, ignored, int(lay.max_nodes))


def wl_match(a: WLColors, protos: WLColors):
    """The WL subtree kernel of every graph of ``a`` against every graph of ``protos`` (both from ``wl_refine`` with the same
    ``iters`` and the same kind of labels) -> ``(K int64 [A, P, T + 1], self_a int64 [A, T + 1])``: ``K[a, p, t]`` counts the node
    pairs (one of each graph) with equal colours at depth t, ``self_a[a, t]`` those of a graph with itself.  One ``cal_wl_match``
    launch, no read-back; the prototype batch may hold 4096 nodes at the most."""
    T1 = int(a.colors.size(0))
    if int(protos.colors.size(0)) != T1:
        raise ValueError("the two refinements differ in depth")
    dev, host = a.colors.device, not a.colors.is_cuda
    ca = a.colors if a.colors.stride(-1) == 1 or a.colors.numel() == 0 else a.colors.contiguous()
    cp = protos.colors.to(dev)
    cp = cp if cp.stride(-1) == 1 or cp.numel() == 0 else cp.contiguous()
    pp = protos.ptr.to(dev).contiguous()
    A, P = int(a.ptr.numel()) - 1, int(pp.numel()) - 1
    Na, Np = int(ca.size(1)), int(cp.size(1))
    sizes = (A * P * T1, A * T1)
    K, own = torch.split(torch.empty(sum(sizes), dtype=torch.long, device=dev), sizes)
    _lib.call("cal_wl_match", _p(ca) if Na else None, int(ca.stride(0)) if Na and T1 > 1 else Na, Na, _p(a.ptr), A,
              _p(cp) if Np else None, int(cp.stride(0)) if Np and T1 > 1 else Np, Np, _p(pp), P, T1 - 1, int(a.max_nodes),
              _p(K) if A and P else None, _p(own) if A else None, None if host else _stream(), host=host)
    return K.view(A, P, T1), own.view(A, T1)


def _self_of(c: WLColors):
    return wl_match(c, c)[1]


def wl_similarity(a: WLColors, protos: WLColors, depths=None) -> torch.Tensor:
    """fp64 [A, P]: ``sum_t K[a, p, t] / sqrt(sum_t self_a[a, t] * sum_t self_p[p, t])`` over ``depths`` (a sequence of depths; all
    by default) -- the cosine of the two graphs' colour histograms, 1 for WL-equivalent graphs, 0 where a graph has no node.  The
    sums are integers and the root is correctly rounded (``_sqrt_rounded``): the GPU and the CPU give the same bits."""
    K, sa = wl_match(a, protos)
    sp = _self_of(protos).to(K.device)
    return _similarity(K, sa, sp, depths)


def _sqrt_rounded(d, x=None):
    """The correctly rounded fp64 square root of ``d`` (fp64, integers >= 1 below 2^53), the same bits on every device; ``x``: the
    root to start from (by default the device's).  fp64
    ``torch.sqrt`` is within an ulp but not correctly rounded on the GPU (about 1.4 % of random integers differ from the CPU's),
    while ``+ - * /`` are: so one Newton step from the device's root x with the exact residual ``d - x x``, the square taken
    as p + e by Dekker's product (Veltkamp's split of x at 27 bits; every product below is exact, and eager torch fuses
    nothing).  The step lands on the correctly rounded root from either neighbour of it unless the root lies within ~2e-16 ulp
    of a rounding boundary (a perfect square has residual 0 and stays exact)."""
    x = d.sqrt() if x is None else x
    c = x * 134217729.0                                                  # 2^27 + 1
    hi = c - (c - x)
    lo = x - hi
    p = x * x
    e = ((hi * hi - p) + (hi * lo) * 2.0) + lo * lo
    return x + ((d - p) - e) / (x * 2.0)


def _similarity(K, sa, sp, depths):
    if depths is not None:
        d = torch.as_tensor(list(depths), dtype=torch.long, device=K.device)
        K, sa, sp = K[:, :, d], sa[:, d], sp[:, d]
    num = K.sum(-1).double()
    sq = (sa.sum(-1)[:, None] * sp.sum(-1)[None, :]).double()            # (an integer below 2^53: nodes^4 (T + 1)^2)
    den = _sqrt_rounded(torch.where(sq > 0, sq, torch.ones_like(sq)))
    return torch.where(sq > 0, num / den, torch.zeros_like(den))


def subgraph_census(data, *, edge_mask=None, node_mask=None, iters: int = 3, labels=None, prototypes=None) -> dict:
    """The shapes of the subgraphs of ``data`` that the masks keep: ``extract_subgraph(..., relabel=True)`` (the kept nodes are
    ``node_mask``, else the nodes a kept edge touches), then ``wl_refine``.

    Returns ``hash`` int64 [B] (depth ``iters``), ``nodes`` / ``edges`` int64 [B] (the subgraph's node and column counts) and
    ``colors`` (the ``WLColors`` of the subgraphs).  ``labels`` as in ``wl_refine``; a tensor has one entry per node of ``data``.
    With ``prototypes`` (a batch, e.g. ``spmotif.motif_batch``, refined here with the same ``iters`` and ``labels``; or a
    ``WLColors``): ``sim`` fp64 [B, P] (``wl_similarity``), ``nearest`` int64 [B] (the most similar prototype, the lowest index on
    ties, -1 for a subgraph without a node) and ``exact`` bool [B, P] (the depth-``iters`` hashes are equal: the subgraph is
    WL-equivalent to the prototype).  One read-back, ``extract_subgraph``'s."""
    sub = extract_subgraph(data, edge_mask=edge_mask, node_mask=node_mask, relabel=True)
    lab = labels
    if torch.is_tensor(labels):
        lab = labels.to(sub.node_map.device)[sub.node_map]
    col = wl_refine(sub, iters=iters, labels=lab)
    res = {"hash": col.hash[:, -1], "nodes": sub.ptr[1:] - sub.ptr[:-1], "edges": sub.edge_ptr[1:] - sub.edge_ptr[:-1],
           "colors": col}
    if prototypes is not None:
        if isinstance(prototypes, WLColors):
            pc = prototypes
        else:
            if torch.is_tensor(labels):
                raise ValueError("a label tensor covers data's nodes only: pass the prototypes as WLColors")
            pc = wl_refine(prototypes, iters=iters, labels=labels)
        K, sa = wl_match(col, pc)
        sim = _similarity(K, sa, _self_of(pc).to(K.device), None)
        res["sim"] = sim
        res["nearest"] = torch.where(res["nodes"] > 0, sim.argmax(1), torch.full_like(res["nodes"], -1))
        res["exact"] = col.hash[:, -1:] == pc.hash[:, -1].to(col.hash.device)[None, :]
    return res


def explanation_census(model, data, *, ratio=None, k=None, undirected="mean", edge_gt=None, node_gt=None, iters: int = 3,
                       labels=None, prototypes=None) -> dict:
    """``explain(model, data, ratio / k, undirected)``, then ``subgraph_census`` on its edge mask: the shape of every graph's
    causal explanation.  Adds ``yhat`` int64 [B] (the argmax of the ``o`` head on the whole graph), ``y`` (``data.y`` or ``None``)
    and ``explanation``.  ``k="gt"`` needs ``edge_gt`` and ``node_gt`` (``spmotif.ground_truth``).  Leaves the model as
    ``explain`` does."""
    ex = explain(model, data, ratio=ratio, k=k, undirected=undirected, edge_gt=edge_gt, node_gt=node_gt)
    with _eval_mode(model):
        yhat = _log_probs(model, data)[1].argmax(-1)                     # (the o head)
    res = subgraph_census(data, edge_mask=ex.edge_mask, iters=iters, labels=labels, prototypes=prototypes)
    y = getattr(data, "y", None)
    res["yhat"], res["y"], res["explanation"] = yhat, None if y is None else y.view(-1).to(yhat.device), ex
    return res


def _class_report(cls, hashes, where, top: int) -> dict:
    """Per class of ``cls`` (a list of ints, -1: none): graphs, distinct shapes, the ``top`` shapes by count."""
    out = {}
    for c in sorted(set(cls) - {-1}):
        idx = [i for i, v in enumerate(cls) if v == c]
        cnt = {}
        for i in idx:
            cnt.setdefault(hashes[i], []).append(i)
        shapes = sorted(cnt.items(), key=lambda kv: (-len(kv[1]), kv[1][0]))
        out[c] = {"graphs": len(idx), "shapes": len(shapes),
                  "top": [{"hash": h & ((1 << 64) - 1), "count": len(m), "share": len(m) / len(idx), "example": where[m[0]]}
                          for h, m in shapes[:top]]}
    return out


def eval_explanation_census(model, loader, device, *, ratio=None, k=None, undirected="mean", iters: int = 3, labels=None,
                            prototypes=None, top: int = 3) -> dict:
    """``explanation_census`` over a loader.  The hashes stay on the device batch by batch; one ``torch.unique`` and one read-back
    at the end (besides ``extract_subgraph``'s per batch).

    ``k="gt"`` ranks against ``spmotif.ground_truth`` (as many edges as the motif has).  Returns ``graphs``, ``shapes`` (distinct
    depth-``iters`` hashes over the loader), ``by_label`` / ``by_prediction``: per class ``graphs``, ``shapes`` and ``top`` -- the
    ``top`` most frequent shapes with ``hash`` (the uint64), ``count``, ``share`` and one ``example`` ``(batch, graph)``, ties by
    first appearance.  With ``prototypes``: ``exact`` (per prototype, the share of graphs whose explanation is WL-equivalent to
    it), ``sim`` (per prototype, the mean similarity) and ``exact_rate``, the share of graphs whose explanation is WL-equivalent
    to the prototype of their own label (labels index the prototypes)."""
    from .spmotif import ground_truth
    pc = None
    if prototypes is not None:
        pc = prototypes if isinstance(prototypes, WLColors) else wl_refine(prototypes.to(device), iters=iters, labels=labels)
    P = 0 if pc is None else int(pc.hash.size(0))
    rows, exact, sims = [], [], []
    for b, data in enumerate(loader):
        data = data.to(device)
        ngt, egt = ground_truth(data) if k == "gt" else (None, None)
        r = explanation_census(model, data, ratio=ratio, k=k, undirected=undirected, edge_gt=egt, node_gt=ngt, iters=iters,
                               labels=labels, prototypes=pc)
        y = r["y"] if r["y"] is not None else torch.full_like(r["yhat"], -1)
        rows.append(torch.stack([r["hash"], y, r["yhat"], torch.full_like(y, b), torch.arange(int(y.numel()), device=y.device)], 1))
        if P:
            exact.append(r["exact"])
            sims.append(r["sim"])
    tab = torch.cat(rows) if rows else torch.zeros(0, 5, dtype=torch.long, device=device)
    G = int(tab.size(0))
    shapes = int(torch.unique(tab[:, 0]).numel())
    packs = [tab.reshape(-1)]
    if P and G:
        ex, sim = torch.cat(exact), torch.cat(sims)
        yl = tab[:, 1]
        own = ex.gather(1, yl.clamp(0, P - 1)[:, None]).view(-1) & (yl >= 0) & (yl < P)
        packs += [ex.sum(0), own.sum().view(1), sim.sum(0).view(torch.long)]     # (the fp64 sums travel as their bits)
    flat = torch.cat(packs).tolist()                                         # the one read-back
    t = [flat[5 * i:5 * i + 5] for i in range(G)]
    hashes, where = [r[0] for r in t], [(r[3], r[4]) for r in t]
    res = {"graphs": G, "shapes": shapes, "by_label": _class_report([r[1] for r in t], hashes, where, top),
           "by_prediction": _class_report([r[2] for r in t], hashes, where, top)}
    if P and G:
        tail = flat[5 * G:]
        res["exact"] = [c / G for c in tail[:P]]
        res["exact_rate"] = tail[P] / G
        res["sim"] = [struct.unpack("<d", struct.pack("<q", v))[0] / G for v in tail[P + 1:]]
    return res
