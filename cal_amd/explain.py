"""Causal-subgraph explanations: the per-graph top-k of CAL's causal attention, and how well it finds a planted motif.

CAL splits every graph into a causal part and a trivial part with two soft masks (model.py:97-111): ``edge_att`` [E, 2]
and ``node_att`` [N, 2].  Column 0 is the context (trivial) branch ``c``, trained toward the uniform distribution
(train_causal.py:180); column 1 is the objects branch ``o``, trained on the label (:181).  So the **causal score is
column 1**: ``edge_att[:, 1]`` (``edge_weight_o``) per edge and ``node_att[:, 1]`` per node.

* ``explain(model, data, ratio=... | k=...)`` -> ``Explanation``: scores, per-graph ranks and top-k masks (and metrics
  against a ground truth) from one eval-mode forward and one ranking call each for edges and nodes
  (``cal_explain_rank``: HIP on the GPU, libcalhost for CPU-resident models).
* ``eval_explanation(model, loader, device)``: mean precision@k, recall@k and ROC-AUC of the causal edges / nodes
  against the SPMotif motif (``spmotif.ground_truth``), the explanation counterpart of ``eval_acc_causal``.
* ``extract_subgraph(data, edge_mask=..., node_mask=..., complement=..., relabel=...)`` -> ``Batch``: the masked batch,
  compacted in order on the device (``cal_subgraph_extract``: two launches and one read-back of the four totals), with the
  layout facts the engine's per-graph kernels need; ``Explanation.to_batch`` is the same through an explanation's masks.
* ``fidelity(model, data, ratio=... | k=...)`` / ``eval_fidelity(model, loader, device, ratios=...)``: does the prediction
  rest on the explanation?  The model runs on the whole graph, on the explanation alone and on the graph without it;
  accuracies, fidelity+ / fidelity- and sparsity per readout head.  Needs no ground truth.
* ``undirected="mean" | "max" | "min"`` on the four calls above: the graphs are undirected and stored as both directions of
  every edge, but CAL's edge attention is not symmetric, so ``(u, v)`` and ``(v, u)`` carry different scores.  With the
  keyword, ``edge_twins(data)`` (``cal_edge_twin``) pairs every column with its reverse and the pairs are ranked as one
  element each (``cal_explain_rank_pairs``): one symmetrised score per undirected edge, symmetric masks, metrics over
  undirected edges, and fidelity on subgraphs that are symmetric whenever the input was.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .plan import _p, _stream

__all__ = ["Explanation", "explain", "eval_explanation", "rank_segments", "rank_segment_pairs", "edge_twins",
           "extract_subgraph", "fidelity", "eval_fidelity"]

_REDUCE = {"mean": 0, "max": 1, "min": 2}


def _reduce_code(undirected) -> Optional[int]:
    """``None`` (directed ranking) or the ``reduce`` argument of cal_explain_rank_pairs."""
    if undirected is None:
        return None
    if undirected not in _REDUCE:
        raise ValueError('undirected must be None, "mean", "max" or "min"')
    return _REDUCE[undirected]


def _k_code(ratio, k) -> Tuple[int, float]:
    """(k, ratio) arguments of cal_explain_rank: k >= 0 top k, -1 ceil(ratio * m), -2 the ground-truth count."""
    if (ratio is None) == (k is None):
        raise ValueError("exactly one of ratio / k is required")
    if k is None:
        ratio = float(ratio)
        if not ratio >= 0.0:
            raise ValueError("ratio must be >= 0")
        return -1, ratio
    if isinstance(k, str):
        if k != "gt":
            raise ValueError('k must be an int >= 0 or "gt"')
        return -2, 0.0
    if int(k) < 0:
        raise ValueError("k must be >= 0")
    return int(k), 0.0


def _rank_call(score, seg_ptr, max_seg, twin, reduce_code, ratio, k, gt, metrics):
    """The one call behind ``rank_segments`` (``twin`` is ``None``: ``cal_explain_rank``) and ``rank_segment_pairs``
    (``cal_explain_rank_pairs`` under ``reduce_code``) -> ``(mask, rank, metrics or None, symmetrised score or None)``."""
    if score.dim() != 1 or score.dtype != torch.float32:
        raise TypeError("score must be a 1-D float32 tensor")
    kc, rt = _k_code(ratio, k)
    if kc == -2 and gt is None:
        raise ValueError('k="gt" needs the ground truth')
    dev, host = score.device, not score.is_cuda
    M, B = score.numel(), seg_ptr.numel() - 1
    pairs = twin is not None
    if pairs and twin.numel() != M:
        raise ValueError("twin must have one entry per score")
    seg_ptr = seg_ptr.to(device=dev, dtype=torch.long).contiguous()
    stride = max(int(score.stride(0)), 1) if M else 1
    mask = torch.empty(M, dtype=torch.uint8, device=dev)
    rank = torch.empty(M, dtype=torch.int32, device=dev)
    met = torch.empty(B, 4, dtype=torch.float64, device=dev) if metrics else None
    g8 = None
    if gt is not None:
        if gt.numel() != M:
            raise ValueError("gt must have one entry per score")
        g8 = gt.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
    out, wsb = None, 0
    if pairs:
        twin = twin.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty(M, dtype=torch.float32, device=dev)
        wsb = _lib.query("cal_explain_pairs_ws", M, B, host=host)
    elif max_seg > _lib.query("cal_explain_lds_cap", host=host):
        wsb = _lib.query("cal_explain_ws", M, B, host=host)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    sp, mp, rp = (_p(score), _p(mask), _p(rank)) if M else (None, None, None)      # (null when there is no element)
    st = None if host else _stream()
    if pairs:
        _lib.call("cal_explain_rank_pairs", sp, stride, _p(seg_ptr), B, M, int(max_seg), rt, kc, _p(g8), _p(twin) if M else None,
                  reduce_code, _p(out) if M else None, mp, rp, _p(met), _p(ws), wsb, st, host=host)
    else:
        _lib.call("cal_explain_rank", sp, stride, _p(seg_ptr), B, M, int(max_seg), rt, kc, _p(g8), mp, rp, _p(met), _p(ws), wsb, st,
                  host=host)
    return mask.view(torch.bool), rank, met, out


def rank_segments(score: torch.Tensor, seg_ptr: torch.Tensor, max_seg: int, *, ratio=None, k=None,
                  gt: Optional[torch.Tensor] = None, metrics: bool = False):
    """One ``cal_explain_rank`` call over the segments ``[seg_ptr[g], seg_ptr[g+1])`` of the 1-D ``score`` (any stride).

    Returns ``(mask bool [M], rank int32 [M], metrics fp64 [B, 4] or None)``; a metrics row is ``k_g, hits, P, AUC``.
    ``max_seg`` must bound every segment's length (host int)."""
    return _rank_call(score, seg_ptr, max_seg, None, None, ratio, k, gt, metrics)[:3]


def rank_segment_pairs(score: torch.Tensor, seg_ptr: torch.Tensor, max_seg: int, twin: torch.Tensor, reduce: str = "mean", *,
                       ratio=None, k=None, gt: Optional[torch.Tensor] = None, metrics: bool = False):
    """One ``cal_explain_rank_pairs`` call: ``rank_segments`` with every column and its ``twin`` (int32 [M], as ``edge_twins``
    gives it for columns grouped by graph) ranked as one element under the ``reduce`` of their two scores.

    Returns ``(mask bool [M], rank int32 [M], metrics fp64 [B, 4] or None, score float32 [M])``: both columns of a pair carry
    the pair's rank, mask and symmetrised score; ``k`` / ``ratio`` / the metrics count pairs, not columns."""
    rc = _reduce_code(reduce)
    if rc is None:
        raise ValueError('reduce must be "mean", "max" or "min"')
    return _rank_call(score, seg_ptr, max_seg, twin, rc, ratio, k, gt, metrics)


@dataclass
class Explanation:
    """Per-graph causal explanation of a batch.  Scores are column 1 (the objects branch ``o``) of the soft masks:
    ``edge_score = edge_att[:, 1]`` (``edge_weight_o``), ``node_score = node_att[:, 1]``; copies that survive later engine
    calls.  ``*_rank`` is the 0-based position inside the element's graph (score descending, index ascending), ``*_mask``
    the selection ``rank < k_g``.  ``ptr`` / ``edge_ptr`` [B + 1] give each graph's node / edge ranges; ``edge_ptr`` is
    ``None`` when the batch's edge columns are not grouped by graph.  ``metrics`` (when a ground truth was given):
    ``{"edge": [B, 4], "node": [B, 4]}`` fp64 rows ``k_g, hits, P, ROC-AUC``.  With ``explain(..., undirected=...)``:
    ``edge_twin`` int32 [E] is the reverse column of every edge column (-1: none, itself for a self loop), ``edge_score``
    the symmetrised score, ``edge_rank`` / ``edge_mask`` / the edge metrics count undirected edges and
    ``edge_mask[e] == edge_mask[edge_twin[e]]``; ``edge_twin`` is ``None`` otherwise."""
    edge_score: torch.Tensor
    node_score: torch.Tensor
    edge_mask: torch.Tensor
    node_mask: torch.Tensor
    edge_rank: torch.Tensor
    node_rank: torch.Tensor
    ptr: torch.Tensor
    edge_ptr: Optional[torch.Tensor]
    edge_index: torch.Tensor
    metrics: Optional[dict] = None
    edge_twin: Optional[torch.Tensor] = None

    def subgraph(self, g: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Graph ``g``'s selected nodes (global ids, ascending) and selected edges ([2, k] global edge_index columns)."""
        lo, hi = int(self.ptr[g]), int(self.ptr[g + 1])
        nodes = lo + self.node_mask[lo:hi].nonzero().view(-1)
        if self.edge_ptr is not None:
            elo, ehi = int(self.edge_ptr[g]), int(self.edge_ptr[g + 1])
            cols = elo + self.edge_mask[elo:ehi].nonzero().view(-1)
        else:
            src = self.edge_index[0]
            cols = (self.edge_mask & (src >= lo) & (src < hi)).nonzero().view(-1)
        return nodes, self.edge_index[:, cols]

    def to_batch(self, data, *, complement: bool = False, relabel: bool = False, use: str = "edges"):
        """``extract_subgraph(data, ...)`` through this explanation's masks: ``use`` = ``"edges"`` (``edge_mask``), ``"nodes"``
        (``node_mask``) or ``"both"``; ``complement``: the batch with the explanation removed.  ``data`` is the batch that
        was explained."""
        em, nm = _use_masks(use, self.edge_mask, self.node_mask)
        return extract_subgraph(data, edge_mask=em, node_mask=nm, complement=complement, relabel=relabel)


def _eval_forward(model, data):
    """``model``'s engine after one eval-mode forward of ``data`` with the identity permutation, or ``None`` (nothing ran)
    when the model has no engine for ``data``."""
    x = data.x if getattr(data, "x", None) is not None else data.feat
    eng = model._engine_for(x)
    if eng is not None:
        eng.forward(data, None, training=False)          # identity permutation: no host RNG
        eng._fwd_token = getattr(eng, "_fwd_token", 0) + 1    # (a pending training-mode backward would now read eval activations)
    return eng


@contextlib.contextmanager
def _eval_mode(model):
    """Eval mode under ``no_grad``; ``model.training`` is put back on the way out.  The scope of every driver that "leaves the
    model as ``explain`` does"."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


def _scores(model, data):
    """Eval-mode causal scores (edge [E], node [N]) of ``data`` with the identity permutation.  Engine-backed models: views
    into the engine's workspace; others: the operator-level backbone + attention (``_CausalBase._attention_scores``)."""
    eng = _eval_forward(model, data)
    return eng.attention_scores(data) if eng is not None else model._attention_scores(data)


class _Layout:
    """Node / edge segments of a batch: ``ptr``, ``edge_ptr`` (of the edge columns in ``order``), the bounds, and ``order``
    (``None`` when the edge columns are grouped by graph; else the stable sort of the columns by graph id)."""

    def __init__(self, data):
        from .engine import _layout_of
        B = int(data.num_graphs)
        dev = data.edge_index.device
        lay = _layout_of(data, B)
        self.B = B
        self.no_self_loops = bool(lay["no_self_loops"])
        self.ptr = lay["ptr"].to(dev)
        self.max_nodes = int(lay["max_nodes"] or 0)
        if self.max_nodes == 0 and B > 0 and data.batch.numel() > 0:
            self.max_nodes = int((self.ptr[1:] - self.ptr[:-1]).max())
        self.order = None
        if lay["edge_ptr"] is not None:
            self.edge_ptr = lay["edge_ptr"].to(dev)
            self.max_edges = int(lay["max_edges"] or 0)
        else:
            gid = data.batch[data.edge_index[0]]
            self.order = torch.argsort(gid, stable=True)
            self.edge_ptr = torch.searchsorted(gid[self.order], torch.arange(B + 1, device=dev, dtype=torch.long)).contiguous()
            self.max_edges = int((self.edge_ptr[1:] - self.edge_ptr[:-1]).max()) if B > 0 else 0
        if self.max_edges == 0 and B > 0 and data.edge_index.size(1) > 0:
            self.max_edges = int((self.edge_ptr[1:] - self.edge_ptr[:-1]).max())

    def _in_order(self, call, score, kw):
        """``call(score, **kw)`` over the columns in ``order``: ``score`` and ``gt`` reordered by graph, every per-column
        tensor of the result (all but the metrics, at index 2) scattered back to the caller's column order."""
        if self.order is None:
            return call(score, **kw)
        gt = kw.pop("gt", None)
        res = call(score[self.order].contiguous(), gt=None if gt is None else gt[self.order], **kw)

        def back(t):
            out = torch.empty_like(t)
            out[self.order] = t
            return out
        return tuple(r if i == 2 else back(r) for i, r in enumerate(res))

    def rank_edges(self, score, **kw):
        return self._in_order(lambda s, **k: rank_segments(s, self.edge_ptr, self.max_edges, **k), score, kw)

    def twins(self, edge_index):
        """``(twin int32 [E], totals int64 [2])`` of one ``cal_edge_twin`` call over the columns in ``order`` (twin indexes that
        order); totals = columns without a twin, self loops; both stay on the device.  Computed once per layout."""
        if getattr(self, "_twins", None) is None:
            ei = edge_index if self.order is None else edge_index[:, self.order]
            ei = ei.to(torch.long).contiguous()
            dev, host = ei.device, not ei.is_cuda
            E = int(ei.size(1))
            wsb = _lib.query("cal_edge_twin_ws", E, self.B, host=host)
            buf = torch.empty(2 + (wsb + 7) // 8, dtype=torch.long, device=dev)      # totals and the workspace
            twin = torch.empty(E, dtype=torch.int32, device=dev)
            _lib.call("cal_edge_twin", _p(ei) if E else None, E, _p(self.ptr.contiguous()), _p(self.edge_ptr.contiguous()), self.B,
                      int(self.max_edges), _p(twin) if E else None, _p(buf), _p(buf[2:]), 8 * (buf.numel() - 2),
                      None if host else _stream(), host=host)
            self._twins = (twin, buf[:2])
        return self._twins

    def caller_twin(self, twin):
        """``twin`` (over the columns in ``order``) as a map between the caller's columns."""
        if self.order is None:
            return twin
        out = torch.empty_like(twin)
        mapped = self.order[twin.clamp(min=0).long()].to(torch.int32)
        out[self.order] = torch.where(twin >= 0, mapped, twin)
        return out

    def rank_edge_pairs(self, score, edge_index, reduce, **kw):
        """``rank_edges`` over undirected edges -> ``(mask, rank, metrics, symmetrised score)`` in the caller's column order."""
        twin = self.twins(edge_index)[0]
        return self._in_order(lambda s, **k: rank_segment_pairs(s, self.edge_ptr, self.max_edges, twin, reduce, **k), score, kw)

    def rank_nodes(self, score, **kw):
        return rank_segments(score, self.ptr, self.max_nodes, **kw)


def edge_twins(data):
    """The reverse-edge map of a batch: ``(twin int32 [E], n_unpaired, n_self)`` from one ``cal_edge_twin`` call (HIP for CUDA
    tensors, libcalhost for CPU tensors; no read-back).

    Inside each graph the j-th column equal to ``(u, v)``, ``u != v``, pairs with the j-th column equal to ``(v, u)`` (both in
    ascending column order): ``twin[e]`` is the partner's column, ``-1`` without one; a self loop is its own twin; a column
    with an endpoint outside its graph pairs with nothing.  So ``twin[twin[e]] == e`` wherever ``twin[e] >= 0``.
    ``n_unpaired`` (columns with ``twin < 0``) and ``n_self`` (self loops) are 0-dim int64 tensors on ``data``'s device;
    ``int()`` reads one back.  A batch whose columns are not grouped by graph is reordered by graph (stable), as the ranking
    does, and the twin indices are mapped back to the caller's column order."""
    lay = _Layout(data)
    twin, totals = lay.twins(data.edge_index)
    return lay.caller_twin(twin), totals[0], totals[1]


def explain(model, data, *, ratio=None, k=None, node_ratio=None, node_k=None, edge_gt=None, node_gt=None,
            undirected=None) -> Explanation:
    """Per-graph causal explanation of ``data`` by ``model`` (a CausalGCN / CausalGAT / CausalGIN).

    Exactly one of ``ratio`` (select ``ceil(ratio * m_g)`` edges of each graph) or ``k`` (the top ``k``; ``"gt"``: as many
    as the graph has ground-truth edges, needs ``edge_gt``).  Nodes follow ``node_ratio`` / ``node_k``, by default the
    edges' rule.  ``edge_gt`` / ``node_gt``: bool ground truth ([E] / [N], e.g. ``spmotif.ground_truth``) -> per-graph
    metrics.  One eval-mode forward with the identity permutation (the scores come before the readout), then one ranking
    call each for edges and nodes.  Parameters, optimizer state, the engine's step counter, BatchNorm statistics and the
    Python / torch RNG states are left as they were, and ``model.training`` is restored.

    ``undirected`` = ``"mean"`` | ``"max"`` | ``"min"``: rank undirected edges.  Every edge column is paired with its reverse
    (``edge_twins``); a pair is one element with that reduction of its two scores (an unpaired column keeps its own), ``k`` /
    ``ratio`` / the edge metrics count pairs (one is ground truth iff either column is), and both columns receive the pair's
    score, rank and mask.  Two more launches than the directed ranking, plus the twin map's one; nodes are ranked as before."""
    _reduce_code(undirected)
    ek, er = k, ratio
    _k_code(er, ek)
    if node_ratio is None and node_k is None:
        node_ratio, node_k = ratio, k
    _k_code(node_ratio, node_k)
    if ek == "gt" and edge_gt is None:
        raise ValueError('k="gt" needs edge_gt')
    if node_k == "gt" and node_gt is None:
        raise ValueError('node_k="gt" needs node_gt')
    with _eval_mode(model):
        edge, node = _scores(model, data)
        lay = _Layout(data)
        twin = None
        if undirected is None:
            em, er_, emet = lay.rank_edges(edge, ratio=er, k=ek, gt=edge_gt, metrics=edge_gt is not None)
            edge = edge.clone()
        else:
            em, er_, emet, edge = lay.rank_edge_pairs(edge, data.edge_index, undirected, ratio=er, k=ek, gt=edge_gt,
                                                      metrics=edge_gt is not None)
            twin = lay.caller_twin(lay.twins(data.edge_index)[0])
        nm, nr, nmet = lay.rank_nodes(node, ratio=node_ratio, k=node_k, gt=node_gt, metrics=node_gt is not None)
        node = node.clone()
    metrics = None
    if emet is not None or nmet is not None:
        metrics = {"edge": emet, "node": nmet}
    return Explanation(edge_score=edge, node_score=node, edge_mask=em, node_mask=nm, edge_rank=er_, node_rank=nr,
                       ptr=lay.ptr, edge_ptr=lay.edge_ptr if lay.order is None else None, edge_index=data.edge_index,
                       metrics=metrics, edge_twin=twin)


_KEYS = ("precision", "recall", "auc")


def _accumulate(sums: torch.Tensor, met: torch.Tensor, off: int):
    """Add one batch's per-graph metric rows to sums[off:off+6] = (sum, count) of precision, recall, AUC."""
    kg, hits, P, auc = met[:, 0], met[:, 1], met[:, 2], met[:, 3]
    prec_ok, rec_ok, auc_ok = kg > 0, P > 0, ~torch.isnan(auc)
    one = torch.ones_like(kg)
    vals = torch.stack([
        torch.where(prec_ok, hits / torch.where(prec_ok, kg, one), torch.zeros_like(kg)).sum(), prec_ok.sum(),
        torch.where(rec_ok, hits / torch.where(rec_ok, P, one), torch.zeros_like(kg)).sum(), rec_ok.sum(),
        torch.where(auc_ok, auc, torch.zeros_like(auc)).sum(), auc_ok.sum()]).to(torch.float64)
    sums[off:off + 6] += vals


def eval_explanation(model, loader, device, *, k="gt", ratio=None, undirected=None) -> dict:
    """Mean edge / node precision@k, recall@k and ROC-AUC of the causal scores against the SPMotif motif
    (``spmotif.ground_truth``), over the graphs where each is defined (precision: k_g > 0; recall: a motif; AUC: a motif
    and a non-motif element).  ``k="gt"`` selects as many elements as the graph's motif has (precision@k = recall@k);
    ``ratio`` selects ``ceil(ratio * m_g)`` instead.  Per mini-batch: one eval forward, the ground truth and one ranking
    call each for edges and nodes; the sums stay on the device until one read-back at the end.  ``undirected`` (as in
    ``explain``): the edge figures are over undirected edges, one symmetrised score per edge."""
    from .spmotif import ground_truth
    _reduce_code(undirected)
    if ratio is not None:
        k = None
    sums = torch.zeros(12, dtype=torch.float64, device=device)
    with _eval_mode(model):
        for data in loader:
            data = data.to(device)
            edge, node = _scores(model, data)
            node_gt, edge_gt = ground_truth(data)
            lay = _Layout(data)
            if undirected is None:
                emet = lay.rank_edges(edge, ratio=ratio, k=k, gt=edge_gt, metrics=True)[2]
            else:
                emet = lay.rank_edge_pairs(edge, data.edge_index, undirected, ratio=ratio, k=k, gt=edge_gt, metrics=True)[2]
            _, _, nmet = lay.rank_nodes(node, ratio=ratio, k=k, gt=node_gt, metrics=True)
            _accumulate(sums, emet, 0)
            _accumulate(sums, nmet, 6)
    s = sums.tolist()
    out = {}
    for j, part in enumerate(("edge", "node")):
        for i, key in enumerate(_KEYS):
            tot, cnt = s[6 * j + 2 * i], s[6 * j + 2 * i + 1]
            out["%s_%s" % (part, key)] = tot / cnt if cnt else float("nan")
    return out


def _use_masks(use: str, edge_mask, node_mask):
    if use not in ("edges", "nodes", "both"):
        raise ValueError('use must be "edges", "nodes" or "both"')
    return (edge_mask if use != "nodes" else None), (node_mask if use != "edges" else None)


def _keep8(mask, n: int, dev, what: str):
    if mask is None:
        return None
    if mask.dim() != 1 or mask.numel() != n:
        raise ValueError("%s must have one entry per %s" % (what, what.split("_")[0]))
    return mask.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)


def extract_subgraph(data, *, edge_mask=None, node_mask=None, complement: bool = False, relabel: bool = False):
    """The batch ``data`` restricted by a per-edge and / or per-node keep mask, as a ``cal_amd.data.Batch`` the engine can run.

    ``edge_mask`` [E] / ``node_mask`` [N] (bool; ``None`` = keep all); ``complement`` reads each given mask inverted.  An edge
    stays iff its mask keeps it and, with a ``node_mask``, both endpoints stay.  ``relabel=False``: every node stays, ids
    unchanged, ``x`` / ``feat`` / ``batch`` are ``data``'s own tensors.  ``relabel=True``: the kept nodes are ``node_mask``
    when given, else the nodes touched by a kept edge; they are renumbered densely in their original order and their feature
    rows gathered (a graph may end with no node).  Kept elements keep their order, ``num_graphs`` and ``y`` are unchanged.
    The result carries ``ptr``, ``edge_ptr``, ``max_nodes``, ``max_edges``, ``no_self_loops`` (inherited) -- so the engine
    takes its per-graph route -- no tiles, and ``node_map`` / ``edge_map`` (int64: new element -> element of ``data``).

    One ``cal_subgraph_extract`` call (HIP for CUDA tensors, libcalhost for CPU tensors) on the current stream and one
    read-back of the four totals.  A batch whose edge columns are not grouped by graph is first reordered by graph (stable),
    as the ranking does; its result is grouped."""
    from .data import Batch
    x = data.x if getattr(data, "x", None) is not None else getattr(data, "feat", None)
    ei = data.edge_index
    dev, host = ei.device, not ei.is_cuda
    lay = _Layout(data)
    B, E, N = lay.B, int(ei.size(1)), int(data.batch.numel())
    ek = _keep8(edge_mask, E, dev, "edge_mask")
    nk = _keep8(node_mask, N, dev, "node_mask")
    if lay.order is not None:
        ei = ei[:, lay.order]
        ek = None if ek is None else ek[lay.order].contiguous()
    ei = ei.contiguous()
    gather = relabel and x is not None
    if gather and x.dtype != torch.float32:
        raise TypeError("relabel gathers float32 features")
    F = int(x.size(1)) if gather else 0
    wsb = _lib.query("cal_subgraph_ws", N, E, B, host=host)
    sizes = (2 * E, B + 1, B + 1, N if relabel else 0, N, E, 4, (wsb + 7) // 8)
    ints = torch.empty(sum(sizes), dtype=torch.long, device=dev)       # every integer output and the workspace: one allocation
    ei_o, ptr_o, eptr_o, batch_o, nmap, emap, totals, ws = torch.split(ints, sizes)
    x_o = torch.empty(N, F, dtype=torch.float32, device=dev) if gather else None
    xin = x.contiguous() if gather else None
    _lib.call("cal_subgraph_extract", _p(ei) if E else None, E, N, _p(lay.ptr.contiguous()), _p(lay.edge_ptr.contiguous()), B,
              _p(ek), _p(nk), int(bool(complement)), int(bool(relabel)), _p(xin) if gather and N else None, F,
              _p(ei_o) if E else None, _p(ptr_o), _p(eptr_o), _p(batch_o) if relabel and N else None,
              _p(x_o) if gather and N else None, _p(nmap) if N else None, _p(emap) if E else None, _p(totals), _p(ws), 8 * sizes[-1],
              None if host else _stream(), host=host)
    n2, e2, mn, me = totals.tolist()                                   # the one read-back: the Batch needs them as host ints
    b = Batch()
    if relabel:
        feats = None if x is None else x_o[:n2]
        b.x, b.feat = (feats, None) if getattr(data, "x", None) is not None else (None, feats)
        b.batch = batch_o[:n2]
    else:
        b.x, b.feat, b.batch = getattr(data, "x", None), getattr(data, "feat", None), data.batch
    b.edge_index = ei_o[:2 * e2].view(2, e2)
    b.y = getattr(data, "y", None)
    b.ptr, b.edge_ptr, b.num_graphs = ptr_o, eptr_o, B
    b.max_nodes, b.max_edges = int(mn), int(me)
    b.no_self_loops = lay.no_self_loops
    b.node_map = nmap[:n2]
    b.edge_map = emap[:e2] if lay.order is None else lay.order[emap[:e2]]
    return b


_HEADS = ("c", "o", "co")          # the order of the model's three outputs (and of eval_acc_causal's reports)
_FID = ("acc_full", "acc_keep", "acc_drop", "fid_plus", "fid_minus")


def _log_probs(model, data) -> torch.Tensor:
    """Eval-mode log-probabilities [3, B, C] (heads c, o, co) of ``data`` with the identity permutation: the engine's forward
    when the model has one, else the operator-level ``model(data)``."""
    eng = _eval_forward(model, data)
    if eng is not None:
        return torch.stack(eng.logp_copy())
    x = data.x if getattr(data, "x", None) is not None else data.feat
    return torch.stack(model(data, perm=torch.arange(int(data.num_graphs), device=x.device))[:3])


def _untiled(data, lay):
    """``data`` as the extractions of it look to the engine: the same tensors and layout facts, no tile packing -- so the
    whole batch takes the route its subgraphs take and an extraction that keeps everything reproduces it bit for bit."""
    if lay.order is not None or getattr(data, "tile_ptr", None) is None:
        return data
    from .data import Batch
    b = Batch()
    b.x, b.feat, b.edge_index, b.batch, b.y = data.x, data.feat, data.edge_index, data.batch, data.y
    b.ptr, b.edge_ptr, b.num_graphs = lay.ptr, lay.edge_ptr, lay.B
    b.max_nodes, b.max_edges, b.no_self_loops = lay.max_nodes, lay.max_edges, lay.no_self_loops
    return b


def _fidelity_sums(model, data, specs, use: str, undirected=None) -> torch.Tensor:
    """One batch's fidelity sums [len(specs), 18] fp64 on the device, ``specs`` a list of (ratio, k): per head (c, o, co) the
    hits on the full / kept / removed graph and the sums of p_full - p_drop and p_full - p_keep at the full graph's argmax;
    then the graph count, the kept and the total element count.  One forward for the scores, one on the whole graph, two per
    spec.  ``undirected``: the edge masks select undirected edges (both columns of a pair or neither); the twin map is built
    once per batch.  Called in eval mode under no_grad."""
    edge, node = _scores(model, data)
    edge, node = edge.clone(), node.clone()
    lay = _Layout(data)
    full = _log_probs(model, _untiled(data, lay))
    y = data.y.view(-1)
    yhat = full.argmax(-1, keepdim=True)                                # [3, B, 1]
    pf = full.gather(-1, yhat).exp()
    out = []
    for ratio, k in specs:
        if use == "nodes":
            em = None
        elif undirected is None:
            em = lay.rank_edges(edge, ratio=ratio, k=k)[0]
        else:
            em = lay.rank_edge_pairs(edge, data.edge_index, undirected, ratio=ratio, k=k)[0]
        nm = lay.rank_nodes(node, ratio=ratio, k=k)[0] if use != "edges" else None
        rows = [(yhat.squeeze(-1) == y).sum(-1)]
        gaps = []
        for comp in (False, True):
            sub = extract_subgraph(data, edge_mask=em, node_mask=nm, complement=comp, relabel=False)
            lp = _log_probs(model, sub)
            rows.append((lp.argmax(-1) == y).sum(-1))
            gaps.append((pf - lp.gather(-1, yhat).exp()).sum((1, 2)))
        kept = sum(m.sum() for m in (em, nm) if m is not None)
        total = sum(m.numel() for m in (em, nm) if m is not None)
        tail = torch.stack([torch.as_tensor(float(y.numel()), dtype=torch.float64, device=y.device), kept.to(torch.float64),
                            torch.as_tensor(float(total), dtype=torch.float64, device=y.device)])
        # [5, 3] -> head-major [3 x 5]: hits full, keep, drop, sum(p_full - p_drop), sum(p_full - p_keep)
        tab = torch.stack([rows[0].double(), rows[1].double(), rows[2].double(), gaps[1].double(), gaps[0].double()])
        out.append(torch.cat([tab.t().reshape(-1), tail]))
    return torch.stack(out)


def _fidelity_report(row) -> dict:
    n, kept, total = row[15], row[16], row[17]
    res = {}
    for h, head in enumerate(_HEADS):
        for j, key in enumerate(_FID):
            res["%s_%s" % (key, head)] = row[5 * h + j] / n if n else float("nan")
    res["sparsity"] = 1.0 - kept / total if total else float("nan")
    res["graphs"] = int(n)
    return res


def fidelity(model, data, *, ratio=None, k=None, use: str = "edges", undirected=None) -> dict:
    """Does ``model``'s prediction on ``data`` rest on its causal subgraph?  The top ``ratio`` / ``k`` of the causal scores
    (as ``explain`` selects them; ``use``: the edge masks, the node masks or both) is extracted twice with ``relabel=False``
    -- the explanation alone and the batch with it removed -- and the model runs in eval mode with the identity permutation
    on the whole batch and on both.  Per readout head ``h`` in ``c``, ``o``, ``co``, with ŷ the head's argmax on the whole
    graph and p its softmax probability:

    * ``acc_full_h``, ``acc_keep_h``, ``acc_drop_h``: accuracy against ``data.y`` on the whole graph / explanation / rest;
    * ``fid_plus_h``  = mean_g [p_full(ŷ_g) - p_drop(ŷ_g)] (high: the explanation is necessary);
    * ``fid_minus_h`` = mean_g [p_full(ŷ_g) - p_keep(ŷ_g)] (low: the explanation is sufficient);

    and ``sparsity`` = 1 - kept / total over the elements ``use`` names, ``graphs`` the batch size.  One read-back at the
    end.  Like ``explain``, it leaves parameters, optimizer state, the engine's step counter, BatchNorm statistics, the RNG
    states and ``model.training`` as they were.

    ``undirected`` (as in ``explain``): the edge masks select undirected edges, so the explanation and the rest are both
    symmetric graphs whenever ``data`` is -- the kind of graph the model was trained on.  ``ratio`` / ``k`` then count
    undirected edges; ``sparsity`` keeps counting edge columns."""
    _k_code(ratio, k)
    _reduce_code(undirected)
    if k == "gt":
        raise ValueError('fidelity has no ground truth: k must be an int >= 0')
    _use_masks(use, None, None)
    with _eval_mode(model):
        sums = _fidelity_sums(model, data, [(ratio, k)], use, undirected)
    return _fidelity_report(sums[0].tolist())


def eval_fidelity(model, loader, device, *, ratios=(0.1, 0.2, 0.3, 0.5), use: str = "edges", undirected=None) -> dict:
    """``fidelity`` over a loader at every ratio of ``ratios``: ``{ratio: report}``, each report as ``fidelity`` returns it
    with the means taken over all graphs of the loader.  The counterpart of ``eval_explanation`` for data without a ground
    truth.  Per mini-batch one forward for the scores, one on the whole batch and, per ratio, one ranking call each for edges
    and nodes, two extractions and two forwards; the sums stay on the device until one read-back at the end.  ``undirected``:
    as in ``fidelity`` (one twin map per mini-batch, shared by the ratios)."""
    _reduce_code(undirected)
    ratios = [float(r) for r in ratios]
    specs = [(r, None) for r in ratios]
    for r, _ in specs:
        _k_code(r, None)
    _use_masks(use, None, None)
    sums = torch.zeros(len(specs), 18, dtype=torch.float64, device=device)
    with _eval_mode(model):
        for data in loader:
            sums += _fidelity_sums(model, data.to(device), specs, use, undirected)
    return {r: _fidelity_report(row) for r, row in zip(ratios, sums.tolist())}
