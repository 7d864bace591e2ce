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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .plan import _p, _stream

__all__ = ["Explanation", "explain", "eval_explanation", "rank_segments"]


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


def rank_segments(score: torch.Tensor, seg_ptr: torch.Tensor, max_seg: int, *, ratio=None, k=None,
                  gt: Optional[torch.Tensor] = None, metrics: bool = False):
    """One ``cal_explain_rank`` call over the segments ``[seg_ptr[g], seg_ptr[g+1])`` of the 1-D ``score`` (any stride).

    Returns ``(mask bool [M], rank int32 [M], metrics fp64 [B, 4] or None)``; a metrics row is ``k_g, hits, P, AUC``.
    ``max_seg`` must bound every segment's length (host int)."""
    if score.dim() != 1 or score.dtype != torch.float32:
        raise TypeError("score must be a 1-D float32 tensor")
    kc, rt = _k_code(ratio, k)
    if kc == -2 and gt is None:
        raise ValueError('k="gt" needs the ground truth')
    dev = score.device
    host = not score.is_cuda
    M, B = score.numel(), seg_ptr.numel() - 1
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
    ws, wsb = None, 0
    if max_seg > _lib.query("cal_explain_lds_cap", host=host):
        wsb = _lib.query("cal_explain_ws", M, B, host=host)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.call("cal_explain_rank", _p(score) if M else None, stride, _p(seg_ptr), B, M, int(max_seg), rt, kc, _p(g8),
              _p(mask) if M else None, _p(rank) if M else None, _p(met), _p(ws), wsb, None if host else _stream(), host=host)
    return mask.view(torch.bool), rank, met


@dataclass
class Explanation:
    """Per-graph causal explanation of a batch.  Scores are column 1 (the objects branch ``o``) of the soft masks:
    ``edge_score = edge_att[:, 1]`` (``edge_weight_o``), ``node_score = node_att[:, 1]``; copies that survive later engine
    calls.  ``*_rank`` is the 0-based position inside the element's graph (score descending, index ascending), ``*_mask``
    the selection ``rank < k_g``.  ``ptr`` / ``edge_ptr`` [B + 1] give each graph's node / edge ranges; ``edge_ptr`` is
    ``None`` when the batch's edge columns are not grouped by graph.  ``metrics`` (when a ground truth was given):
    ``{"edge": [B, 4], "node": [B, 4]}`` fp64 rows ``k_g, hits, P, ROC-AUC``."""
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


def _scores(model, data):
    """Eval-mode causal scores (edge [E], node [N]) of ``data`` with the identity permutation.  Engine-backed models: views
    into the engine's workspace; others: the operator-level backbone + attention (``_CausalBase._attention_scores``)."""
    x = data.x if getattr(data, "x", None) is not None else data.feat
    eng = model._engine_for(x)
    if eng is not None:
        eng.forward(data, None, training=False)          # identity permutation: no host RNG
        eng._fwd_token = getattr(eng, "_fwd_token", 0) + 1    # (a pending training-mode backward would now read eval activations)
        return eng.attention_scores(data)
    return model._attention_scores(data)


class _Layout:
    """Node / edge segments of a batch: ``ptr``, ``edge_ptr`` (of the edge columns in ``order``), the bounds, and ``order``
    (``None`` when the edge columns are grouped by graph; else the stable sort of the columns by graph id)."""

    def __init__(self, data):
        from .engine import _layout_of
        B = int(data.num_graphs)
        dev = data.edge_index.device
        lay = _layout_of(data, B)
        self.B = B
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

    def rank_edges(self, score, **kw):
        if self.order is None:
            return rank_segments(score, self.edge_ptr, self.max_edges, **kw)
        gt = kw.pop("gt", None)
        mask_s, rank_s, met = rank_segments(score[self.order].contiguous(), self.edge_ptr, self.max_edges,
                                            gt=None if gt is None else gt[self.order], **kw)
        mask, rank = torch.empty_like(mask_s), torch.empty_like(rank_s)
        mask[self.order] = mask_s
        rank[self.order] = rank_s
        return mask, rank, met

    def rank_nodes(self, score, **kw):
        return rank_segments(score, self.ptr, self.max_nodes, **kw)


def explain(model, data, *, ratio=None, k=None, node_ratio=None, node_k=None, edge_gt=None, node_gt=None) -> Explanation:
    """Per-graph causal explanation of ``data`` by ``model`` (a CausalGCN / CausalGAT / CausalGIN).

    Exactly one of ``ratio`` (select ``ceil(ratio * m_g)`` edges of each graph) or ``k`` (the top ``k``; ``"gt"``: as many
    as the graph has ground-truth edges, needs ``edge_gt``).  Nodes follow ``node_ratio`` / ``node_k``, by default the
    edges' rule.  ``edge_gt`` / ``node_gt``: bool ground truth ([E] / [N], e.g. ``spmotif.ground_truth``) -> per-graph
    metrics.  One eval-mode forward with the identity permutation (the scores come before the readout), then one ranking
    call each for edges and nodes.  Parameters, optimizer state, the engine's step counter, BatchNorm statistics and the
    Python / torch RNG states are left as they were, and ``model.training`` is restored."""
    ek, er = k, ratio
    _k_code(er, ek)
    if node_ratio is None and node_k is None:
        node_ratio, node_k = ratio, k
    _k_code(node_ratio, node_k)
    if ek == "gt" and edge_gt is None:
        raise ValueError('k="gt" needs edge_gt')
    if node_k == "gt" and node_gt is None:
        raise ValueError('node_k="gt" needs node_gt')
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            edge, node = _scores(model, data)
            lay = _Layout(data)
            em, er_, emet = lay.rank_edges(edge, ratio=er, k=ek, gt=edge_gt, metrics=edge_gt is not None)
            nm, nr, nmet = lay.rank_nodes(node, ratio=node_ratio, k=node_k, gt=node_gt, metrics=node_gt is not None)
            edge, node = edge.clone(), node.clone()
    finally:
        model.train(was_training)
    metrics = None
    if emet is not None or nmet is not None:
        metrics = {"edge": emet, "node": nmet}
    return Explanation(edge_score=edge, node_score=node, edge_mask=em, node_mask=nm, edge_rank=er_, node_rank=nr,
                       ptr=lay.ptr, edge_ptr=lay.edge_ptr if lay.order is None else None, edge_index=data.edge_index,
                       metrics=metrics)


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


def eval_explanation(model, loader, device, *, k="gt", ratio=None) -> dict:
    """Mean edge / node precision@k, recall@k and ROC-AUC of the causal scores against the SPMotif motif
    (``spmotif.ground_truth``), over the graphs where each is defined (precision: k_g > 0; recall: a motif; AUC: a motif
    and a non-motif element).  ``k="gt"`` selects as many elements as the graph's motif has (precision@k = recall@k);
    ``ratio`` selects ``ceil(ratio * m_g)`` instead.  Per mini-batch: one eval forward, the ground truth and one ranking
    call each for edges and nodes; the sums stay on the device until one read-back at the end."""
    from .spmotif import ground_truth
    if ratio is not None:
        k = None
    was_training = model.training
    model.eval()
    sums = torch.zeros(12, dtype=torch.float64, device=device)
    try:
        with torch.no_grad():
            for data in loader:
                data = data.to(device)
                edge, node = _scores(model, data)
                node_gt, edge_gt = ground_truth(data)
                lay = _Layout(data)
                _, _, emet = lay.rank_edges(edge, ratio=ratio, k=k, gt=edge_gt, metrics=True)
                _, _, nmet = lay.rank_nodes(node, ratio=ratio, k=k, gt=node_gt, metrics=True)
                _accumulate(sums, emet, 0)
                _accumulate(sums, nmet, 6)
    finally:
        model.train(was_training)
    s = sums.tolist()
    out = {}
    for j, part in enumerate(("edge", "node")):
        for i, key in enumerate(_KEYS):
            tot, cnt = s[6 * j + 2 * i], s[6 * j + 2 * i + 1]
            out["%s_%s" % (part, key)] = tot / cnt if cnt else float("nan")
    return out
