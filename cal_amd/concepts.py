"""Concept discovery: deterministic k-means on the node embeddings of a dataset (GCExplainer's recipe, model-level).

The other explanation drivers look at one graph at a time; ``wl.py`` / ``motif.py`` look at the structure of extracted
explanations.  This module looks at what the backbone has learned: the rows ``x`` [N, H] that both attention MLPs read
(``model._node_embeddings``) of every node of a loader are clustered, every cluster is called a concept, and a table says of every
concept whether it is pure, whether it is the planted motif, whether the causal attention looks at it -- and of the table whether
the concepts alone predict the label.

The operator is Lloyd's k-means (``cal_kmeans``: two launches per iteration on the GPU, distances on the matrix cores, the rows
read once per iteration, no ``[N, K]`` matrix; libcalhost for CPU tensors).  A row goes to the centroid with the smallest key
(distance, then the lower centroid), the sums run in a fixed order (rules.hpp), so two calls give the same bits and the concept
table of a model is one table.

* ``kmeans(rows, k, iters=, init=, seed=, restarts=, span_rows=)`` -> ``KMeansResult``; ``assign(rows, centroids)`` -> ``(assign, dist)``.
* ``node_bank(model, loader, device, max_rows=None)`` -> ``NodeBank``: the rows with their graph, label, motif mark, causal
  attention and context.
* ``discover_concepts(model, loader, device, k=)`` -> ``Concepts``; ``assign_concepts(model, data, concepts)`` places a new batch.
* ``concept_report(concepts, examples=5)``: the table; ``eval_concepts(model, loader, device, k=, test_loader=None)``: over a loader.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import _lib, ops, spmotif
from .explain import _eval_mode
from .neighbors import MAX_C as _CLASSES
from .neighbors import knn
from .plan import _p, _stream

__all__ = ["KMeansResult", "NodeBank", "Concepts", "kmeans", "assign", "seed_rows", "node_bank", "discover_concepts",
           "assign_concepts", "concept_report", "eval_concepts", "MAX_H", "MAX_K"]

#: limits of the GPU path; the host library takes any sizes
MAX_H = 256
MAX_K = 64
_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def seed_rows(n: int, k: int, seed: int) -> List[int]:
    """``kmeans_seed_rows`` of rules.hpp: the ``k`` distinct initial rows of a seed, a splitmix64 walk with repeats rejected."""
    if not 1 <= k <= n:
        raise ValueError("seeding needs 1 <= k <= N (got k = %d, N = %d)" % (k, n))
    out, x = [], int(seed) & _M64
    while len(out) < k:
        x = _splitmix64(x)
        r = x % n
        if r not in out:
            out.append(r)
    return out


@dataclass
class KMeansResult:
    """``centroids`` float32 [K, H]; ``assign`` int32 [N]: every row's centroid under the centroids the last iteration run
    started from (-1: a row with a non-finite coordinate); ``counts`` int64 [K] of that assignment (``centroids`` are its means;
    an empty cluster keeps its centroid); ``inertia`` float64 [iters] and ``moved`` int64 [iters] per iteration (0 behind
    ``iters_run``); ``iters_run`` int32 scalar tensor: the iterations run, the first with ``moved == 0`` being the last."""
    centroids: torch.Tensor
    assign: torch.Tensor
    counts: torch.Tensor
    inertia: torch.Tensor
    moved: torch.Tensor
    iters_run: torch.Tensor


def _check_rows(rows: torch.Tensor, what: str = "rows"):
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise ValueError("%s must be a 2-D float32 tensor" % what)
    if int(rows.size(1)) < 1:
        raise ValueError("the rows are empty (H == 0)")
    if int(rows.size(0)) >= 2 ** 31:
        raise ValueError("k-means takes N < 2^31 rows")


def _check_limits(rows: torch.Tensor, K: int):
    if rows.is_cuda:
        if int(rows.size(1)) > MAX_H:
            raise ValueError("the GPU path takes 1 <= H <= %d (got H = %d)" % (MAX_H, int(rows.size(1))))
        if K > MAX_K:
            raise ValueError("the GPU path takes 1 <= K <= %d (got K = %d)" % (MAX_K, K))


def _lloyd(rows: torch.Tensor, c0: torch.Tensor, iters: int, span_rows: int) -> KMeansResult:
    N, H, K, dev = int(rows.size(0)), int(rows.size(1)), int(c0.size(0)), rows.device
    host = not rows.is_cuda
    cout = c0.clone()
    asg = torch.full((N,), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(K, dtype=torch.int64, device=dev)
    inertia = torch.zeros(iters, dtype=torch.float64, device=dev)
    moved = torch.zeros(iters, dtype=torch.int64, device=dev)
    run = torch.zeros(1, dtype=torch.int32, device=dev)
    if N:
        wsb = _lib.query("cal_kmeans_ws", N, K, H, int(span_rows), host=host)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
        _lib.call("cal_kmeans", _p(rows), N, H, _p(c0), K, iters, int(span_rows), _p(cout), _p(asg), _p(counts), _p(inertia),
                  _p(moved), _p(run), _p(ws), wsb, None if host else _stream(), host=host)
    return KMeansResult(cout, asg, counts, inertia, moved, run.view(()))


def kmeans(rows: torch.Tensor, k: int, *, iters: int = 25, init: Optional[torch.Tensor] = None, seed: int = 0,
           restarts: int = 1, span_rows: int = 0) -> KMeansResult:
    """Lloyd's k-means of ``rows`` [N, H] (float32) with ``k`` centroids, at most ``iters`` iterations; the iteration in which
    no row changes its centroid is the last (decided on the device: no read-back, the call can be captured).  ``init``: int64
    [k] distinct rows, or float32 [k, H] centroids; default the rows ``seed_rows(N, k, seed)``.  ``restarts > 1`` (seeded
    starts only): the seeds ``seed, seed + 1, ..``; the run with the lowest final inertia wins, the lower seed on ties -- one
    read-back, at the end.  ``span_rows``: 0, or the rows of a superblock (a multiple of 128); the summation order and so the
    BITS of the centroids depend on it, the assignment of a single step does not.  CUDA tensors: ``cal_kmeans`` on the current
    stream, ``2 * iters`` launches (``H <= 256``, ``k <= 64``); CPU tensors: libcalhost, any sizes.  Two calls give the same
    bits."""
    _check_rows(rows)
    N, H, k, iters, restarts = int(rows.size(0)), int(rows.size(1)), int(k), int(iters), int(restarts)
    if k < 1:
        raise ValueError("k must be >= 1 (got %d)" % k)
    if iters < 1:
        raise ValueError("iters must be >= 1 (got %d)" % iters)
    if restarts < 1:
        raise ValueError("restarts must be >= 1 (got %d)" % restarts)
    if span_rows < 0 or span_rows % 128:
        raise ValueError("span_rows must be 0 or a positive multiple of 128")
    _check_limits(rows, k)
    rows = rows.contiguous()
    dev = rows.device
    if init is not None:
        if restarts != 1:
            raise ValueError("restarts need seeded starts (init=None)")
        if init.device != dev:
            raise ValueError("rows and init must be on one device")
        if init.dtype == torch.float32 and init.dim() == 2:
            if tuple(init.shape) != (k, H):
                raise ValueError("init centroids must be [%d, %d]" % (k, H))
            c0 = init.contiguous()
        elif init.dtype == torch.int64 and init.dim() == 1:
            if init.numel() != k:
                raise ValueError("init rows must be [%d]" % k)
            picks = init.tolist() if not init.is_cuda else None      # (a device index list is taken as it is: no read-back)
            if picks is not None and (len(set(picks)) != k or min(picks) < 0 or max(picks) >= N):
                raise ValueError("init rows must be distinct rows in [0, N)")
            c0 = rows.index_select(0, init).contiguous()
        else:
            raise ValueError("init must be int64 [k] rows or float32 [k, H] centroids")
        return _lloyd(rows, c0, iters, span_rows)
    runs = []
    for r in range(restarts):
        idx = torch.tensor(seed_rows(N, k, int(seed) + r), dtype=torch.long).to(dev)
        runs.append(_lloyd(rows, rows.index_select(0, idx).contiguous(), iters, span_rows))
    if restarts == 1:
        return runs[0]
    final = torch.stack([r.inertia[(r.iters_run.long() - 1).clamp(min=0)] for r in runs])
    best = int(torch.argmin(final))                                # the first minimum: the lower seed on ties
    return runs[best]


def assign(rows: torch.Tensor, centroids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(assign int32 [N], dist float32 [N])``: for every row its centroid by the key of ``kmeans`` and the squared distance
    to it; -1 and ``+inf`` for a row whose distance to every centroid is non-finite.  One launch on the GPU."""
    _check_rows(rows)
    _check_rows(centroids, "centroids")
    if centroids.device != rows.device:
        raise ValueError("rows and centroids must be on one device")
    N, H, K = int(rows.size(0)), int(rows.size(1)), int(centroids.size(0))
    if int(centroids.size(1)) != H:
        raise ValueError("rows [*, %d] and centroids [*, %d] must have one width" % (H, int(centroids.size(1))))
    if K < 1:
        raise ValueError("there is no centroid (K == 0)")
    _check_limits(rows, K)
    host = not rows.is_cuda
    rows, centroids = rows.contiguous(), centroids.contiguous()
    asg = torch.empty(N, dtype=torch.int32, device=rows.device)
    dist = torch.empty(N, dtype=torch.float32, device=rows.device)
    if N:
        _lib.call("cal_kmeans_assign", _p(rows), N, H, _p(centroids), K, _p(asg), _p(dist), None if host else _stream(), host=host)
    return asg, dist


@dataclass
class NodeBank:
    """The node rows of the graphs of a loader: ``x`` float32 [N, H] the eval-mode ``_node_embeddings`` rows; ``graph`` int64 [N]
    the running number of the row's graph in its loader; ``y`` int64 [N] its graph's label; ``node_gt`` bool [N] its motif mark
    (``spmotif.ground_truth``) or ``None`` when that does not apply to every graph; ``att`` float32 [N] the causal node attention
    (column 1); ``context`` int64 [N] its graph's context (``spmotif.context_of``) or ``None``; ``num_graphs``."""
    x: torch.Tensor
    graph: torch.Tensor
    y: torch.Tensor
    node_gt: Optional[torch.Tensor]
    att: torch.Tensor
    context: Optional[torch.Tensor]
    num_graphs: int = 0

    def __len__(self) -> int:
        return int(self.graph.numel())


def _node_rows(model, data):
    """(x [N, H], att [N]) of a batch inside ``_eval_mode``: the backbone rows and the causal node attention they give."""
    x = model._embed(data)[0]
    if getattr(model, "without_node_attention", False):
        att = torch.full((x.size(0),), 0.5, dtype=x.dtype, device=x.device)
    else:
        att = ops.node_attention_split(x, model.node_att_mlp.weight, model.node_att_mlp.bias)[2][:, 1]
    return x, att


def node_bank(model, loader, device, max_rows: Optional[int] = None) -> NodeBank:
    """``NodeBank`` of every node of every graph of ``loader`` (eval mode, no grad) on ``device``; at most ``max_rows`` rows (the
    first ones) when given.  Leaves parameters, optimizer state, BatchNorm statistics and both RNG states as they were, like
    ``embedding_bank``."""
    cols, n, g0 = [], 0, 0
    with _eval_mode(model):
        for data in loader:
            data = data.to(device)
            x, att = _node_rows(model, data)
            B = int(data.num_graphs)
            bvec = data.batch
            ctx = spmotif.context_of(data)
            gt = spmotif.ground_truth(data)[0] if int(data.y.numel()) == B else torch.zeros_like(bvec, dtype=torch.bool)
            yc = data.y.view(-1)
            safe = (yc >= 0) & (yc < len(spmotif.CLASS_LIST))
            if not bool(safe.all()):                                # ground_truth indexes the motif table by the label
                gt = torch.zeros_like(bvec, dtype=torch.bool)
            cols.append((x, bvec + g0, yc[bvec], gt, att, ctx[bvec]))
            g0 += B
            n += int(x.size(0))
            if max_rows is not None and n >= max_rows:
                break
    if not cols:
        raise ValueError("the loader is empty")
    x, graph, y, gt, att, ctx = (torch.cat(c)[:max_rows].contiguous() for c in zip(*cols))
    known = bool((ctx >= 0).all())
    num = int(graph[-1]) + 1 if graph.numel() else 0
    return NodeBank(x, graph, y, gt if known else None, att, ctx if known else None, num)


@dataclass
class Concepts:
    """``result``: the ``KMeansResult`` over ``bank.x``; ``bank``: the ``NodeBank`` the concepts were found in."""
    result: KMeansResult
    bank: NodeBank

    @property
    def k(self) -> int:
        return int(self.result.centroids.size(0))


def discover_concepts(model, loader, device, k: int = 8, *, max_rows: Optional[int] = None, **kmeans_kw) -> Concepts:
    """The ``k`` concepts of a model over a loader: ``node_bank``, then ``kmeans`` of its rows (``kmeans_kw``: ``iters``, ``init``,
    ``seed``, ``restarts``, ``span_rows``)."""
    bank = node_bank(model, loader, device, max_rows)
    return Concepts(kmeans(bank.x, k, **kmeans_kw), bank)


def assign_concepts(model, data, concepts: Concepts) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(concept int32 [N], dist float32 [N])`` of every node of the batch ``data``: one eval-mode backbone forward, then
    ``assign`` against the concepts' centroids.  Leaves the model as ``node_bank`` does."""
    return assign(model._node_embeddings(data).contiguous(), concepts.result.centroids)


def _histograms(asg: torch.Tensor, graph: torch.Tensor, B: int, K: int) -> torch.Tensor:
    """int64 [B, K]: how many nodes of graph b carry concept c (rows at -1 are in no column)."""
    ok = asg >= 0
    return torch.bincount(graph[ok] * K + asg[ok].long(), minlength=B * K)[:B * K].view(B, K)


def _graph_values(bank: NodeBank, v: torch.Tensor) -> torch.Tensor:
    """[B]: the value of a graph's rows (every row of a graph carries the same), -1 for a graph without rows."""
    out = torch.full((bank.num_graphs,), -1, dtype=torch.long, device=v.device)
    out[bank.graph] = v                                            # equal values: any write order gives the same
    return out


def concept_report(concepts: Concepts, examples: int = 5, *, k: int = 5, queries: Optional[Tuple[NodeBank, torch.Tensor]] = None) -> dict:
    """The concept table.  Per concept ``c`` (``["concepts"][c]``): ``size``; ``purity_y`` and ``purity_context`` -- the share of
    its rows that carry its most frequent label / context (``None`` without a context; ``nan`` for an empty concept);
    ``motif_share``, the share of its rows that are motif nodes (``None`` without ground truth); ``attention``, the mean causal
    node attention of its rows; ``examples``: the ``examples`` bank rows nearest to its centroid as ``{"row", "graph", "node",
    "dist"}`` (``node``: the row's number inside its graph), from one ``knn(centroids, bank.x, examples)`` call.

    Over the table: ``completeness``, the leave-one-out ``k``-NN accuracy of the label from the per-graph concept histograms
    ``[B, K]`` (integer counts cast to float32; one ``knn`` call with ``skip`` and ``votes``, the majority of ``knn_majority``:
    the lowest label on ties) -- this stands in for the decision tree GCExplainer fits on the same histograms: a non-parametric
    probe this package already has, reproducible bit for bit.  With ``queries = (bank, assign)`` of other graphs (test graphs
    placed with ``assign``): their histograms against the table's, nothing skipped.  ``chance``: the share of the most frequent
    label among the table's graphs.  ``motif_concepts``: the concepts whose motif share exceeds 1/2; ``attention_gap``: the mean
    attention of the rows in those concepts less that of the rows in the others (``nan`` when either side is empty; ``None``
    without ground truth).  Labels and contexts count in [0, 64).  All counts are integers on the device, read back once."""
    res, bank = concepts.result, concepts.bank
    K, N, B, dev = concepts.k, len(bank), bank.num_graphs, bank.x.device
    examples = int(examples)
    a = res.assign.long()
    ok = a >= 0
    ac = a.clamp(min=0)
    size = torch.bincount(a[ok], minlength=K)[:K]

    def table(v):                                                  # [K] the rows of the most frequent value of v per concept
        good = ok & (v >= 0) & (v < _CLASSES)
        return torch.bincount(a[good] * _CLASSES + v[good], minlength=K * _CLASSES)[:K * _CLASSES].view(K, _CLASSES).max(1).values

    parts = [size, table(bank.y)]
    parts.append(table(bank.context) if bank.context is not None else torch.zeros_like(size))
    gt = bank.node_gt
    motif = torch.bincount(a[ok & gt], minlength=K)[:K] if gt is not None else torch.zeros_like(size)
    parts.append(motif)
    # attention sums per concept in a fixed order: rows sorted by concept (stable), one fp64 running sum, differences at the ends
    order = torch.argsort(torch.where(ok, a, torch.full_like(a, K)), stable=True)
    run = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), bank.att.double()[order].cumsum(0)])
    ends = size.cumsum(0)
    att_sum = run[ends] - run[ends - size]
    is_motif = (2 * motif > size) if gt is not None else torch.zeros(K, dtype=torch.bool, device=dev)
    in_motif = is_motif[ac] & ok
    att_ok = torch.where(ok, bank.att.double(), torch.zeros((), dtype=torch.float64, device=dev))
    gap = torch.stack([torch.where(in_motif, att_ok, torch.zeros_like(att_ok)).sum(), in_motif.sum().double(),
                       torch.where(in_motif, torch.zeros_like(att_ok), att_ok).sum(), (ok & ~in_motif).sum().double()])

    ex = min(examples, N)
    if ex > 0:
        near = knn(res.centroids, bank.x, ex)
        has = near.idx >= 0
        at = near.idx.clamp(min=0).long()
        first = torch.zeros(B + 1, dtype=torch.long, device=dev)
        first[1:] = torch.bincount(bank.graph, minlength=B)[:B].cumsum(0)
        g = bank.graph[at]
        ex_parts = [torch.where(has, t, torch.full_like(t, -1)).double().view(-1) for t in (at, g, at - first[g])]
        ex_parts.append(near.dist.double().view(-1))
    else:
        ex_parts = []

    gy = _graph_values(bank, bank.y)
    hist = _histograms(res.assign, bank.graph, B, K).float()
    if queries is None:
        qy, qh, skip = gy, hist, torch.arange(B, device=dev)
    else:
        qb, qa = queries
        qy, qh, skip = _graph_values(qb, qb.y), _histograms(qa, qb.graph, qb.num_graphs, K).float(), None
    kk = int(k)
    if B > (1 if queries is None else 0) and qh.size(0) > 0:
        votes = knn(qh, hist, kk, skip=skip, labels=gy, num_classes=_CLASSES).votes.long()
        major = (votes * _CLASSES + torch.arange(_CLASSES - 1, -1, -1, device=dev)).argmax(1)       # knn_majority
        hits = ((major == qy) & (votes.sum(1) > 0)).sum()
    else:
        hits = torch.zeros((), dtype=torch.long, device=dev)
    known = (gy >= 0) & (gy < _CLASSES)
    top = torch.bincount(gy[known], minlength=_CLASSES).max()

    flat = torch.cat([torch.stack(parts).double().view(-1), att_sum, is_motif.double(), gap,
                      torch.stack([hits, top]).double()] + ex_parts).tolist()          # the one read-back
    nan = float("nan")
    it = iter(flat)
    take = lambda n: [next(it) for _ in range(n)]
    size_l, py, pc, mo, at_l, im = (take(K) for _ in range(6))
    g_in, n_in, g_out, n_out = take(4)
    hits_v, top_v = take(2)
    ex_l = [take(K * ex) for _ in range(4)] if ex > 0 else None
    rows = []
    for c in range(K):
        n = int(size_l[c])
        e = []
        for p in range(ex if ex_l else 0):
            i = c * ex + p
            if ex_l[0][i] >= 0:
                e.append({"row": int(ex_l[0][i]), "graph": int(ex_l[1][i]), "node": int(ex_l[2][i]), "dist": ex_l[3][i]})
        rows.append({"size": n, "purity_y": py[c] / n if n else nan,
                     "purity_context": None if bank.context is None else (pc[c] / n if n else nan),
                     "motif_share": None if gt is None else (mo[c] / n if n else nan),
                     "attention": at_l[c] / n if n else nan, "examples": e})
    nq = int(qh.size(0))
    return {"k": K, "rows": N, "graphs": B, "queries": nq, "concepts": rows,
            "completeness": hits_v / nq if nq else nan, "chance": top_v / B if B else nan,
            "motif_concepts": [c for c in range(K) if im[c]] if gt is not None else None,
            "attention_gap": None if gt is None else ((g_in / n_in - g_out / n_out) if n_in and n_out else nan)}


def eval_concepts(model, loader, device, k: int = 8, *, test_loader=None, examples: int = 5, knn_k: int = 5, **kmeans_kw) -> dict:
    """``concept_report`` of a model over a loader: ``discover_concepts`` there; with ``test_loader`` the completeness is that of
    the test graphs, placed in the table with ``assign``, against the histograms of the graphs of ``loader``."""
    concepts = discover_concepts(model, loader, device, k, **kmeans_kw)
    queries = None
    if test_loader is not None:
        tb = node_bank(model, test_loader, device)
        queries = (tb, assign(tb.x, concepts.result.centroids)[0])
    return concept_report(concepts, examples, k=knn_k, queries=queries)
