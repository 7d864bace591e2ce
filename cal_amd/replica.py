"""What the replica builders (``splice_batches``, ``occlude_batch``, ``coalition_batch``, ``noise_batch``, ``subset_batch``) and the drivers on top of
them share: the builders' plumbing (``_Source`` ... ``_built_batch``, ``_twin_in_order``, ``_node_map_rows``), the whole batch on the replicas' route (``_grouped``,
``_whole``), one replica forward (``_replica_log_probs``), the players of a batch (``_Players``, ``_representatives``, ``_members``),
the causal score in graph order and the rho / tau / jaccard report.  It imports from ``explain`` and ``plan`` only; a new
replica-based attribution method starts from these pieces instead of copying a sibling driver.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from .explain import _HEADS, _k_code, _keep8, _Layout, _log_probs, _reduce_code, _scores, rank_segment_pairs, rank_segments
from .plan import _p, _stream


# ---- the builders' plumbing ---------------------------------------------------------------------------------------------------
class _Source:
    """What the operator reads of one batch: features, grouped edge columns, the two offset arrays."""

    def __init__(self, data):
        from .data import Batch
        self.is_x = getattr(data, "x", None) is not None
        self.x = data.x if self.is_x else getattr(data, "feat", None)
        ei = data.edge_index
        self.order = None
        if isinstance(data, Batch) and data.ptr is not None and data.edge_ptr is not None:
            self.B, self.ptr, self.edge_ptr = int(data.num_graphs), data.ptr, data.edge_ptr
            self.no_self_loops = bool(data.no_self_loops)
        else:
            lay = _Layout(data)
            self.B, self.ptr, self.edge_ptr, self.no_self_loops, self.order = lay.B, lay.ptr, lay.edge_ptr, lay.no_self_loops, lay.order
            if self.order is not None:                     # columns not grouped by graph: stable graph order first
                ei = ei[:, self.order]
        self.dev = ei.device
        self.ei = ei.to(torch.long).contiguous()
        self.ptr = self.ptr.to(device=self.dev, dtype=torch.long).contiguous()
        self.edge_ptr = self.edge_ptr.to(device=self.dev, dtype=torch.long).contiguous()
        self.E = int(ei.size(1))
        self.N = int(data.batch.numel()) if getattr(data, "batch", None) is not None else int(self.x.size(0))
        self.y = getattr(data, "y", None)

    def args(self):
        return [_p(self.ei) if self.E else None, self.E, self.N, _p(self.ptr), _p(self.edge_ptr), self.B]


def _pairs(t, n: int, dev, what: str):
    if t is None:
        return torch.arange(n, dtype=torch.long, device=dev)
    t = torch.as_tensor(t)
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("%s must be a 1-D integer tensor" % what)
    return t.to(device=dev, dtype=torch.long).contiguous()


def _feature_width(S, name: str) -> int:
    """F of a replica builder's one source (0: no features); ``name`` is the builder's, for the message."""
    if S.x is None:
        return 0
    if S.x.dtype != torch.float32:
        raise TypeError("%s copies float32 features" % name)
    if S.x.dim() != 2:
        raise ValueError("the features must be [N, F]")
    return int(S.x.size(1))


#: what ``_rebatch`` returns: the offsets, ``tot`` (the totals and the bad count as host ints: nodes, columns, largest node count,
#: largest column count, result graphs without a node, ..., bad), the outputs (``edge_index`` flat [2 Eout], ``x`` or ``None``)
_Built = namedtuple("_Built", "ptr edge_ptr tot batch node_src edge_index edge_src x")


def _rebatch(stem: str, ws_args, inputs, R: int, ntot: int, srcs, F: int, bad):
    """The calls of one batch builder, ``stem`` + ``_ws`` / ``_count`` / ``_write``: the workspace query, one allocation for the
    offsets, ``totals`` [ntot] and the workspace, the count, the one read-back, the outputs' allocation, the write.  ``inputs``:
    the arguments both entry points start with; ``srcs``: the ``_Source`` objects whose rows (F columns) are copied; ``bad()``: a
    bool tensor whose count is read back with the totals -- a callable, so that its torch launches are issued while the count
    kernel runs, not in front of it.  -> ``_Built``."""
    dev, host = srcs[0].dev, not srcs[0].ei.is_cuda
    wsb = _lib.query(stem + "_ws", *ws_args, host=host)
    sizes = (R + 1, R + 1, ntot, (wsb + 7) // 8)
    ptr_o, eptr_o, totals, ws = torch.split(torch.empty(sum(sizes), dtype=torch.long, device=dev), sizes)
    st = None if host else _stream()
    _lib.call(stem + "_count", *inputs, _p(ptr_o), _p(eptr_o), _p(totals), _p(ws), 8 * sizes[-1], st, host=host)
    # the one read-back: the Batch needs the totals as host ints (and y whether every result graph has its source of y)
    tot = torch.cat([totals, bad().sum().view(1)]).tolist()
    n2, e2 = tot[:2]
    ints = torch.empty(2 * n2 + 3 * e2, dtype=torch.long, device=dev)
    batch_o, nsrc, ei_o, esrc = torch.split(ints, (n2, n2, 2 * e2, e2))
    x_o = torch.empty(n2, F, dtype=torch.float32, device=dev) if F else None
    xs = [s.x.contiguous() if F and s.N else None for s in srcs]
    _lib.call(stem + "_write", *inputs, *map(_p, xs), F, _p(ptr_o), _p(eptr_o), n2, e2,
              _p(batch_o) if n2 else None, _p(x_o) if F and n2 else None, _p(ei_o) if e2 else None, _p(nsrc) if n2 else None,
              _p(esrc) if e2 else None, _p(ws), 8 * sizes[-1], st, host=host)
    return _Built(ptr_o, eptr_o, tot, batch_o, nsrc, ei_o, esrc, x_o)


def _built_batch(S, b, picks, no_self_loops: bool, edge_src):
    """The ``Batch`` of ``b`` (``_Built``): features as ``S`` carries them, ``y = S.y[picks]`` unless a pick was bad; ``edge_src``
    in the caller's column numbering."""
    from .data import Batch
    out = Batch()
    out.x, out.feat = (b.x, None) if S.is_x or S.x is None else (None, b.x)
    out.edge_index, out.batch = b.edge_index.view(2, b.tot[1]), b.batch
    out.y = S.y.view(-1)[picks] if S.y is not None and not b.tot[-1] else None
    out.ptr, out.edge_ptr, out.num_graphs = b.ptr, b.edge_ptr, int(picks.numel())
    out.max_nodes, out.max_edges = int(b.tot[2]), int(b.tot[3])
    out.no_self_loops = no_self_loops
    out.node_src, out.edge_src = b.node_src, edge_src
    out.empty_graphs = int(b.tot[4])
    return out


def _caller_columns(S, esrc, n_cols: int):
    """``edge_src`` of a one-source builder in the caller's column numbering: columns that were reordered (``S.order``) are
    mapped back, negative entries (an inserted column) stay."""
    if S.order is None or not n_cols:
        return esrc
    return torch.where(esrc >= 0, S.order[esrc.clamp(min=0)], esrc)


def _twin_in_order(S, twin):
    """``twin`` (int32 [E] as ``edge_twins`` gives it for the caller's columns, or ``None``) as the builders of ``S`` take it: int32,
    contiguous, and for columns that were reordered (``S.order``) a map between positions in graph order."""
    if twin is None:
        return None
    if not torch.is_tensor(twin) or twin.dim() != 1 or int(twin.numel()) != S.E:
        raise ValueError("twin must be a 1-D tensor with one entry per edge column")
    tw = twin.to(device=S.dev, dtype=torch.int32).contiguous()
    if S.order is not None and S.E:
        inv = torch.empty_like(S.order)
        inv[S.order] = torch.arange(S.E, device=S.dev)
        tw = tw[S.order]
        tw = torch.where(tw >= 0, inv[tw.clamp(min=0).long()].to(torch.int32), tw).contiguous()
    return tw


def _node_map_rows(S, data) -> int:
    """The row length of a node-mode builder's per-replica node map: a bound on every graph's node count (a ``Batch``'s own
    ``max_nodes`` when it knows it, else one read-back)."""
    from .data import Batch
    if not (S.N and S.B):
        return 0
    mx = int(getattr(data, "max_nodes", 0) or 0) if isinstance(data, Batch) else 0
    return mx if mx > 0 else int((S.ptr[1:] - S.ptr[:-1]).max())


# ---- argument checks ----------------------------------------------------------------------------------------------------------
def _check_use(use):
    if use not in ("nodes", "edges"):
        raise ValueError('use must be "nodes" or "edges"')


def _check_head(head):
    if head not in _HEADS:
        raise ValueError('head must be "c", "o" or "co"')
    return _HEADS.index(head)


def _check_driver_args(use, undirected, head, chunk):
    """-> (the head's index, ``chunk`` as an int) of a driver over edge columns, undirected edges or nodes."""
    _check_use(use)
    _reduce_code(undirected)
    if undirected is not None and use != "edges":
        raise ValueError('undirected needs use="edges"')
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    return _check_head(head), chunk


def _check_topk(ratio, k, who: str):
    """``_k_code`` for a caller without a ground truth (``who``, for the message) -> (k, ratio) as ``cal_explain_rank`` takes them."""
    kc, rt = _k_code(ratio, k)
    if kc == -2:
        raise ValueError('%s has no ground truth: k must be an int >= 0' % who)
    return kc, rt


# ---- the whole batch and one chunk of replicas --------------------------------------------------------------------------------
def _grouped(data, lay):
    """``data`` with its edge columns in graph order and the layout facts of ``lay``, no tile packing: the source of the
    replicas, and the whole batch on the route the replicas take (``explain._untiled`` for grouped columns)."""
    from .data import Batch
    b = Batch()
    b.x, b.feat, b.batch, b.y = getattr(data, "x", None), getattr(data, "feat", None), data.batch, getattr(data, "y", None)
    b.edge_index = (data.edge_index if lay.order is None else data.edge_index[:, lay.order]).contiguous()
    b.ptr, b.edge_ptr, b.num_graphs = lay.ptr, lay.edge_ptr, lay.B
    b.max_nodes, b.max_edges, b.no_self_loops = lay.max_nodes, lay.max_edges, lay.no_self_loops
    return b


def _p_at(lp, yhat):
    """The probability of class ``yhat`` [...] under the log-probabilities ``lp`` [..., C]."""
    return lp.gather(-1, yhat.unsqueeze(-1)).squeeze(-1).exp()


def _whole(model, src, h):
    """-> (ŷ int64 [B], p_full [B], C): the whole batch on the route the replicas take."""
    full = _log_probs(model, src)[h]                                     # [B, C]
    yhat = full.argmax(-1)
    return yhat, _p_at(full, yhat), int(full.size(-1))


def _check_replicas(rb):
    if rb.empty_graphs:
        raise ValueError("%d replicas have no node (the engine does not run zero-node graphs)" % rb.empty_graphs)


def _replica_log_probs(model, rb, h):
    """Head ``h``'s log-probabilities [R, C] of the replica batch ``rb``: one forward."""
    _check_replicas(rb)
    return _log_probs(model, rb)[h]


# ---- the players --------------------------------------------------------------------------------------------------------------
def _representatives(twin):
    """bool [M]: one column per undirected edge of the twin map -- the lower column of a pair, an unpaired column, a self loop."""
    return ~((twin >= 0) & (twin < torch.arange(twin.numel(), device=twin.device)))


def _members(elements, M: int, lay, use, twin):
    """``elements`` (a mask [M] in the caller's order) as a bool mask over ``lay``'s graph order; with ``twin`` an undirected edge
    is asked for by either column."""
    want = _keep8(elements, M, lay.ptr.device, "elements").view(torch.bool)
    if use == "edges" and lay.order is not None:
        want = want[lay.order]
    if twin is not None:
        want = want | (want[twin.clamp(min=0).long()] & (twin >= 0))
    return want


class _Players:
    """The elements of a batch as the drivers see them, over the edge columns in ``lay``'s graph order: ``M`` elements in the
    segments ``seg`` (bound ``max_seg``) with graph ids ``gid``; ``twin`` (int32 [M], ``undirected`` only) and ``rep`` (bool [M]
    or ``None``: ``_representatives``); ``nodes`` int64 [B], every graph's node count."""

    def __init__(self, data, lay, src, use, undirected):
        dev = src.edge_index.device
        self.nodes = (lay.ptr[1:] - lay.ptr[:-1]).to(dev)
        self.twin = self.rep = None
        B = lay.B
        if use == "edges":
            self.M, self.seg, self.max_seg = int(src.edge_index.size(1)), lay.edge_ptr.to(dev), lay.max_edges
            self.gid = torch.repeat_interleave(torch.arange(B, device=dev), self.seg[1:] - self.seg[:-1], output_size=self.M)
            if undirected is not None:
                self.twin = lay.twins(data.edge_index)[0]
                self.rep = _representatives(self.twin)
        else:
            self.M, self.seg, self.max_seg, self.gid = int(src.batch.numel()), lay.ptr.to(dev), lay.max_nodes, src.batch
        self.B, self.dev, self.undirected = B, dev, undirected

    def count(self, mask):
        """int64 [B]: the marked elements of every graph."""
        return torch.zeros(self.B, dtype=torch.long, device=self.dev).index_add_(0, self.gid, mask.long())

    def rank(self, score):
        """int32 [M]: every element's 0-based position inside its graph under ``score`` (float32 [M], descending, NaN last, then
        index ascending); with ``undirected`` the position of its undirected edge among the graph's undirected edges."""
        score = score.contiguous()
        if self.twin is None:
            return rank_segments(score, self.seg, self.max_seg, k=0)[1]
        return rank_segment_pairs(score, self.seg, self.max_seg, self.twin, self.undirected, k=0)[1]


# ---- the causal score against another ranking ---------------------------------------------------------------------------------
def _causal_in_order(model, data, use):
    """-> (the causal score as ``explain`` reads it, a copy, edge columns in graph order; the ``_Layout``): one forward."""
    edge, node = _scores(model, data)
    causal = (edge if use == "edges" else node).clone()
    lay = _Layout(data)
    if use == "edges" and lay.order is not None:
        causal = causal[lay.order].contiguous()
    return causal, lay


def _symmetrised(causal, lay, twin, undirected):
    """One score per undirected edge, as ``explain`` symmetrises it (edge columns in graph order): one ranking call."""
    return rank_segment_pairs(causal, lay.edge_ptr, lay.max_edges, twin, undirected, k=0)[3]


AGREE = ("rho", "tau", "jaccard")


def _agree_sums(met):
    """``rank_agreement``'s metrics [B, 3] -> fp64 [6] on the device: the three sums over where each figure is defined, then
    the three counts of rows where it is."""
    defined = ~torch.isnan(met)
    return torch.cat([torch.where(defined, met, torch.zeros_like(met)).sum(0), defined.sum(0).double()])


def _agree_report(sums6, n) -> dict:
    """The means of ``_agree_sums`` (host numbers) and, of ``n`` rows, how many left each figure undefined."""
    res = {}
    for j, key in enumerate(AGREE):
        res[key] = sums6[j] / sums6[3 + j] if sums6[3 + j] else float("nan")
        res[key + "_undefined"] = int(n - sums6[3 + j])
    return res
