"""Exact motif matching: does an explanation *contain* the planted motif, *is* it the motif, and *where* does the motif sit.

``cal_amd.wl`` answers these up to 1-WL equivalence and all-or-nothing: the house plus one stray edge is a miss, a 6-cycle and two
triangles are the same shape.  Here the answer is exact.  Motifs have at most 8 nodes and the graphs at most 256, so counting the
embeddings by backtracking is cheap, integer-only and independent per graph:

* ``motif_match(data, patterns, induced=False, labels=None, pattern_labels=None, budget=1 << 17)`` -> ``MotifMatch``: for every
  graph of ``data`` and every pattern the number of embeddings, the smallest one and the roots the step budget cut short
  (``cal_motif_match``: one launch on the GPU, one workgroup per graph; libcalhost for CPU tensors; the definitions are in
  ``include/cal_hip.h``).
* ``automorphisms(patterns)``, ``contains(m)``, ``isomorphic(m, data_ptr, pattern_ptr)``.
* ``motif_census`` / ``explanation_motifs`` (also ``model.explanation_motifs``) / ``eval_explanation_motifs``: extract the
  explanation subgraphs and match them against prototypes (``spmotif.motif_batch``); over a loader also how often the WL census
  said "the motif" of a subgraph that is not isomorphic to it.
"""
from __future__ import annotations

import copy
from collections import namedtuple

import torch

from . import _lib
from .explain import _eval_mode, _Layout, _log_probs, explain, extract_subgraph
from .plan import _p, _stream

__all__ = ["MotifMatch", "MotifPatterns", "motif_match", "automorphisms", "contains", "isomorphic", "motif_census",
           "explanation_motifs", "eval_explanation_motifs", "MAX_PATTERN", "MAX_NODES", "MAX_PATTERNS", "DEFAULT_BUDGET"]

#: the limits of the operator (``CAL_MOTIF_MAX_*``)
MAX_PATTERN = 8
MAX_NODES = 256
MAX_PATTERNS = 64
#: steps a root may take; above the largest need of a root on whole SPMotif graphs of node_num 15 (78 920)
DEFAULT_BUDGET = 1 << 17

#: ``count`` int64 [B, P] (-1: the graph has more than 256 nodes and was skipped), ``first`` int32 [B, P, 8] (the
#: lexicographically smallest embedding found, local node ids by pattern node; -1 where there is none and beyond the pattern's
#: size), ``truncated`` int64 [B, P] (roots stopped by the budget), ``tgt_edges`` int64 [B] / ``pat_edges`` int64 [P] (adjacent
#: unordered pairs; -1 for a skipped graph, and everywhere when B = 0 or P = 0: nothing ran), ``ignored`` int64 [1] (the columns
#: of ``data`` with an endpoint outside their graph; on the device, not read back).
MotifMatch = namedtuple("MotifMatch", "count first truncated tgt_edges pat_edges ignored")


class MotifPatterns:
    """A pattern batch made ready for ``motif_match``: its columns (grouped by graph), ``ptr`` and ``edge_ptr`` as contiguous int64
    tensors in host memory, where the launcher plans the match orders.  Built once from a batch on any device (a batch on the
    GPU is copied to the host here, never inside a loop over ``motif_match``); ``automorphisms`` is cached on it."""

    def __init__(self, patterns):
        lay = _Layout(patterns)
        ei = patterns.edge_index
        if lay.order is not None:
            ei = ei[:, lay.order]
        self.edge_index = ei.to(device="cpu", dtype=torch.long).contiguous()
        self.ptr = lay.ptr.to(device="cpu", dtype=torch.long).contiguous()
        self.edge_ptr = lay.edge_ptr.to(device="cpu", dtype=torch.long).contiguous()
        self.P, self.PN, self.PE = lay.B, int(patterns.batch.numel()), int(ei.size(1))
        self._aut = None
        self._on = {}

    def on(self, dev):
        """``(ptr, automorphisms)`` on ``dev`` (copied once per device)."""
        dev = torch.device(dev)
        if dev not in self._on:
            self._on[dev] = (self.ptr.to(dev), automorphisms(self).to(dev))
        return self._on[dev]


def _patterns(patterns) -> MotifPatterns:
    return patterns if isinstance(patterns, MotifPatterns) else MotifPatterns(patterns)


def _labels(t, n: int, dev, what: str):
    t = torch.as_tensor(t)
    if t.dim() != 1 or int(t.numel()) != n or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("%s must be a 1-D integer tensor with one entry per node" % what)
    return t.to(device=dev, dtype=torch.long).contiguous()


def _match(ei, ptr, eptr, B: int, N: int, labels, pp: MotifPatterns, plabels, induced: bool, budget: int) -> MotifMatch:
    dev, host = ei.device, not ei.is_cuda
    E, P = int(ei.size(1)), pp.P
    budget = int(budget)
    if budget < 0:
        raise ValueError("budget must be >= 0")
    sizes = (B * P, B * P, B, P, 1)
    ran = B > 0 and P > 0
    ints = torch.empty(sum(sizes), dtype=torch.long, device=dev) if ran else torch.full((sum(sizes),), -1, dtype=torch.long, device=dev)
    count, trunc, tgt, pat, ignored = torch.split(ints, sizes)
    first = torch.empty(B * P * MAX_PATTERN, dtype=torch.int32, device=dev)
    _lib.call("cal_motif_match", _p(ei) if E else None, E, N, _p(ptr), _p(eptr), B, _p(labels) if N else None,
              _p(pp.edge_index) if pp.PE else None, pp.PE, pp.PN, _p(pp.ptr), _p(pp.edge_ptr), P, _p(plabels) if pp.PN else None,
              int(bool(induced)), budget, _p(count), _p(trunc), _p(first), _p(tgt), _p(pat), _p(ignored),
              None if host else _stream(), host=host)
    return MotifMatch(count.view(B, P), first.view(B, P, MAX_PATTERN), trunc.view(B, P), tgt, pat, ignored)


def motif_match(data, patterns, *, induced: bool = False, labels=None, pattern_labels=None, budget: int = DEFAULT_BUDGET) -> MotifMatch:
    """The embeddings of every pattern in every graph of ``data`` (``cal_motif_match``).

    Both sides are read as simple undirected graphs (a column in either direction makes its endpoints adjacent; self loops and
    duplicates add nothing).  ``count[g, p]`` is the number of injective maps of the pattern's nodes into the graph's that keep
    adjacency -- and, with ``induced``, non-adjacency -- and the labels (``labels`` int64 [N] of ``data`` and ``pattern_labels``
    [PN], both or neither).  A pattern matched against itself with ``induced=True`` has |Aut| embeddings; ``count // |Aut|`` is
    the number of distinct occurrences.  ``budget``: the candidates one root of the search may try; the roots that needed more
    are counted in ``truncated`` (then ``count`` is a lower bound).  ``patterns``: a batch of connected graphs of 1 to 8 nodes,
    64 at the most, or a ``MotifPatterns`` made from one (do that outside a loop: a pattern batch on the GPU is copied to the
    host).  A batch whose columns are not grouped by graph is reordered by graph first, as ``wl_refine`` does.  CUDA tensors:
    one launch on the current stream, no read-back; CPU tensors: libcalhost.  Both give the same bits."""
    pp = _patterns(patterns)
    ei = data.edge_index
    dev = ei.device
    lay = _Layout(data)
    if lay.order is not None:
        ei = ei[:, lay.order]
    ei = ei.to(torch.long).contiguous()
    N = int(data.batch.numel())
    if (labels is None) != (pattern_labels is None):
        raise ValueError("labels and pattern_labels go together")
    lab = None if labels is None else _labels(labels, N, dev, "labels")
    plab = None if pattern_labels is None else _labels(pattern_labels, pp.PN, dev, "pattern_labels")
    return _match(ei, lay.ptr.to(torch.long).contiguous(), lay.edge_ptr.to(torch.long).contiguous(), lay.B, N, lab, pp, plab,
                  induced, budget)


def automorphisms(patterns) -> torch.Tensor:
    """int64 [P] (host memory): |Aut| of every pattern, the diagonal of the induced match of the pattern batch against itself."""
    pp = _patterns(patterns)
    if pp._aut is None:
        m = _match(pp.edge_index, pp.ptr, pp.edge_ptr, pp.P, pp.PN, None, pp, None, True, 1 << 40)
        pp._aut = m.count.diagonal().clone()
    return pp._aut


def contains(m: MotifMatch) -> torch.Tensor:
    """bool [B, P]: the graph has at least one embedding of the pattern."""
    return m.count > 0


def isomorphic(m: MotifMatch, data_ptr, pattern_ptr) -> torch.Tensor:
    """bool [B, P]: the graph IS the pattern up to isomorphism -- equal node counts (from the two ``ptr``), equal numbers of
    adjacent pairs and an embedding (which is then a bijection that maps the edges onto the edges)."""
    dev = m.count.device
    n = (data_ptr[1:] - data_ptr[:-1]).to(dev)
    k = (pattern_ptr[1:] - pattern_ptr[:-1]).to(dev)
    return (n[:, None] == k[None, :]) & (m.tgt_edges[:, None] == m.pat_edges[None, :]) & (m.count > 0)


def motif_census(data, *, edge_mask=None, node_mask=None, prototypes, induced: bool = False, budget: int = DEFAULT_BUDGET) -> dict:
    """The prototypes in the subgraphs of ``data`` that the masks keep: ``extract_subgraph(..., relabel=True)`` (the kept nodes
    are ``node_mask``, else the nodes a kept edge touches), then ``motif_match``.

    Returns ``contains`` / ``isomorphic`` bool [B, P], ``occurrences`` int64 [B, P] (``count // |Aut|``: the distinct
    occurrences; -1 for a skipped subgraph), ``truncated`` int64 [B, P], ``skipped`` bool [B] (more than 256 nodes), ``nodes`` /
    ``edges`` int64 [B] (the subgraph's nodes and adjacent pairs; -1 edges when skipped), ``match_nodes`` int64 [B, P, 8] (the
    smallest embedding as node ids of ``data``, by prototype node; -1 where there is none), ``match`` (the ``MotifMatch``, local
    ids) and ``subgraph`` (the extracted batch).  ``prototypes``: a batch (``spmotif.motif_batch``) or a ``MotifPatterns``.  One
    read-back, ``extract_subgraph``'s."""
    pp = _patterns(prototypes)
    sub = extract_subgraph(data, edge_mask=edge_mask, node_mask=node_mask, relabel=True)
    m = motif_match(sub, pp, induced=induced, budget=budget)
    dev = m.count.device
    pptr, aut = pp.on(dev)
    B, P = m.count.shape
    idx = sub.ptr[:-1].view(B, 1, 1) + m.first.long()
    nmap = sub.node_map
    if int(nmap.numel()):
        where = torch.where(m.first >= 0, nmap[idx.clamp(0, int(nmap.numel()) - 1)], torch.full_like(idx, -1))
    else:
        where = torch.full_like(idx, -1)
    skipped = sub.ptr[1:] - sub.ptr[:-1] > MAX_NODES
    occ = torch.where(m.count >= 0, m.count // aut.clamp(min=1)[None, :], m.count)
    return {"contains": contains(m), "isomorphic": isomorphic(m, sub.ptr, pptr), "occurrences": occ, "truncated": m.truncated,
            "skipped": skipped, "nodes": sub.ptr[1:] - sub.ptr[:-1], "edges": m.tgt_edges, "match_nodes": where, "match": m,
            "subgraph": sub}


def explanation_motifs(model, data, *, ratio=None, k=None, undirected="mean", edge_gt=None, node_gt=None, prototypes=None,
                       induced: bool = False, budget: int = DEFAULT_BUDGET) -> dict:
    """``explain(model, data, ratio / k, undirected)``, then ``motif_census`` on its edge mask: which prototypes every graph's
    causal explanation contains or is.  ``prototypes`` defaults to ``spmotif.motif_batch()``.  Adds ``yhat`` int64 [B] (the
    argmax of the ``o`` head on the whole graph), ``y`` (``data.y`` or ``None``) and ``explanation``; with ``edge_gt`` also
    ``planted`` bool [B, P]: the prototype is contained in the explanation's truly planted edges alone (a second census, on
    ``edge_mask & edge_gt``).  ``k="gt"`` needs ``edge_gt`` and ``node_gt`` (``spmotif.ground_truth``).  Leaves the model, the
    engine and the RNG states as ``explain`` does."""
    if prototypes is None:
        from .spmotif import motif_batch
        prototypes = motif_batch()
    pp = _patterns(prototypes)
    ex = explain(model, data, ratio=ratio, k=k, undirected=undirected, edge_gt=edge_gt, node_gt=node_gt)
    with _eval_mode(model):
        yhat = _log_probs(model, data)[1].argmax(-1)                     # (the o head)
    res = motif_census(data, edge_mask=ex.edge_mask, prototypes=pp, induced=induced, budget=budget)
    if edge_gt is not None:
        gt = edge_gt.to(device=ex.edge_mask.device, dtype=torch.bool)
        res["planted"] = motif_census(data, edge_mask=ex.edge_mask & gt, prototypes=pp, induced=induced, budget=budget)["contains"]
    y = getattr(data, "y", None)
    res["yhat"], res["y"], res["explanation"] = yhat, None if y is None else y.view(-1).to(yhat.device), ex
    return res


def eval_explanation_motifs(model, loader, device, *, ratio=None, k=None, undirected="mean", prototypes=None, induced: bool = False,
                            budget: int = DEFAULT_BUDGET, iters: int = 3) -> dict:
    """``explanation_motifs`` over a loader.  Everything stays on the device batch by batch; one read-back at the end (besides
    ``extract_subgraph``'s per batch).

    ``k="gt"`` ranks against ``spmotif.ground_truth`` (as many edges as the motif has).  Labels index the prototypes.  Returns
    ``graphs``; ``contain_rate`` / ``iso_rate``: the share of graphs whose explanation contains / is the prototype of their own
    label; with ``k="gt"`` ``planted_rate``: ... contains it in its truly planted edges alone; ``contains`` / ``isomorphic``: the
    shares per prototype; ``wl_not_iso``: the share of graphs whose explanation the WL census (``wl_refine`` at depth ``iters``)
    calls ``exact`` for their label's prototype although it is not isomorphic to it -- the error of the 1-WL answer;
    ``truncated`` (roots) and ``skipped`` (graphs), totals over the loader."""
    from .spmotif import ground_truth, motif_batch
    from .wl import wl_refine
    proto = motif_batch() if prototypes is None else prototypes
    if isinstance(proto, MotifPatterns):
        raise TypeError("eval_explanation_motifs refines the prototypes too: pass the batch, not MotifPatterns")
    pp = MotifPatterns(proto)
    P = pp.P
    phash = wl_refine(copy.copy(proto).to(device), iters=iters).hash[:, -1]      # (``to`` moves a batch in place: a copy's)
    rows = []
    for data in loader:
        data = data.to(device)
        ngt, egt = ground_truth(data) if k == "gt" else (None, None)
        r = explanation_motifs(model, data, ratio=ratio, k=k, undirected=undirected, edge_gt=egt, node_gt=ngt, prototypes=pp,
                               induced=induced, budget=budget)
        exact = wl_refine(r["subgraph"], iters=iters).hash[:, -1:] == phash[None, :]
        y = r["y"] if r["y"] is not None else torch.full_like(r["yhat"], -1)
        ok = (y >= 0) & (y < P)
        yc = y.clamp(0, max(P - 1, 0))[:, None]

        def own(t):
            return (t.gather(1, yc).view(-1) & ok).sum().view(1) if P else ok.sum().view(1) * 0
        planted = r.get("planted")
        rows.append(torch.cat([ok.new_tensor([int(y.numel())], dtype=torch.long), own(r["contains"]), own(r["isomorphic"]),
                               own(planted) if planted is not None else torch.zeros(1, dtype=torch.long, device=y.device),
                               own(exact & ~r["isomorphic"]), r["truncated"].sum().view(1), r["skipped"].sum().view(1),
                               r["contains"].sum(0), r["isomorphic"].sum(0)]))
    if not rows:
        tot = [0] * (7 + 2 * P)
    else:
        tot = torch.stack(rows).sum(0).tolist()                          # the one read-back
    G = tot[0]
    d = max(G, 1)
    res = {"graphs": G, "contain_rate": tot[1] / d, "iso_rate": tot[2] / d, "wl_not_iso": tot[4] / d, "truncated": tot[5],
           "skipped": tot[6], "contains": [c / d for c in tot[7:7 + P]], "isomorphic": [c / d for c in tot[7 + P:7 + 2 * P]]}
    if k == "gt":
        res["planted_rate"] = tot[3] / d
    return res
