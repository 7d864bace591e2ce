"""Gradient attributions: a soft mask on every edge column or node, saliency and integrated gradients.

Occlusion (``cal_amd.occlude``) and Shapley values (``cal_amd.coalition``) score an element by running replicas of its graph
with elements removed.  The gradient family needs no replica: the operator-level path runs the whole model under torch autograd,
and ``_CausalBase._masked_forward`` carries a weight ``m_e`` in [0, 1] per edge column through *every* convolution, so that
``m_e = 0`` is exactly the graph without that column and ``m = 1`` the model as it is.  The binary
corners of that cube are what ``coalition_batch`` builds as hard replicas; this module differentiates in its interior.

* ``masked_log_probs(model, data, edge_mask=..., node_mask=...)`` -> the three log-prob heads, differentiable in the masks.
* ``saliency(model, data, use=..., undirected=..., head=..., elements=...)`` (also ``model.saliency``) -> ``Gradients``:
  ``d sum_g p(ŷ_g) / d m`` at ``m = 1``; one forward and one backward of the batch.
* ``integrated_gradients(..., steps=32)`` (also ``model.integrated_gradients``) -> ``Gradients``: the midpoint-rule integral of
  that gradient from the players at 0 to the players at 1; its scores sum to ``p_full - p_baseline`` up to ``gap``.
* ``gradient_agreement(model, data, method=..., ...)``: the causal attention against either score, through ``rank_agreement``.

Mask values are not read back: the domain is ``m >= 0``, finite.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Optional

import torch

from .explain import _eval_mode
from .occlude import rank_agreement
from .replica import (_agree_report, _agree_sums, _causal_in_order, _check_driver_args, _check_topk, _p_at, _representatives,
                      _symmetrised)

__all__ = ["Gradients", "masked_log_probs", "saliency", "integrated_gradients", "gradient_agreement"]


@dataclass
class Gradients:
    """Gradient attributions of a batch.  ``score`` fp64 [E] (``use="edges"``) or [N] (``"nodes"``), signed, in the caller's order;
    NaN for an element that is no player (outside ``elements``); both columns of an undirected edge carry the pair's score.
    ``p_full`` [B] and ``yhat`` int64 [B]: the whole graph's probability of its own argmax at the chosen head, and that argmax.
    ``method``: ``"saliency"`` or ``"ig"``.  Integrated gradients also give ``p_baseline`` [B] (every player at 0), ``steps`` and
    ``gap`` fp64 [B] = the sum of the graph's player scores - (``p_full - p_baseline``), the quadrature error of the ``steps``
    midpoints; saliency leaves them ``None`` / 0.  ``forwards``: forwards of the batch it took.  ``twin``: the reverse-column map
    int32 [E] when ``undirected`` built one, else ``None``."""
    score: torch.Tensor
    p_full: torch.Tensor
    yhat: torch.Tensor
    method: str
    forwards: int
    steps: int = 0
    p_baseline: Optional[torch.Tensor] = None
    gap: Optional[torch.Tensor] = None
    twin: Optional[torch.Tensor] = None


@contextlib.contextmanager
def _frozen(model):
    """Eval mode, every parameter frozen, autograd on: only the masks collect a gradient, no ``.grad`` of a parameter is touched
    and no layer computes one.  Everything is put back on the way out."""
    was_training = model.training
    params = [p for p in model.parameters() if p.requires_grad]
    model.eval()
    for p in params:
        p.requires_grad_(False)
    try:
        with torch.enable_grad():
            yield
    finally:
        for p in params:
            p.requires_grad_(True)
        model.train(was_training)


def _check_mask(mask, n: int, dev, what: str):
    if mask is None:
        return None
    if not torch.is_tensor(mask) or mask.dtype != torch.float32:
        raise TypeError("%s must be a float32 tensor" % what)
    if mask.dim() != 1 or int(mask.numel()) != n:
        raise ValueError("%s must be 1-D with one entry per %s (%d)" % (what, "edge column" if what == "edge_mask" else "node", n))
    if mask.device != dev:
        raise ValueError("%s is on %s, the batch on %s" % (what, mask.device, dev))
    return mask


def _sizes(data):
    x = data.x if getattr(data, "x", None) is not None else data.feat
    return int(data.edge_index.size(1)), int(x.size(0)), data.edge_index.device


def masked_log_probs(model, data, *, edge_mask=None, node_mask=None):
    """The ``(c, o, co)`` log-probs [B, C] of ``data`` under a soft edge mask (float32 [E]) and / or node mask (float32 [N]),
    differentiable with respect to the masks: eval mode, identity intervention permutation, on the operator-level path (an
    engine-backed model's parameters are read from the same storage).  Mask semantics: ``_CausalBase._masked_forward``.

    Autograd is on inside whatever the caller's grad mode, so ``torch.autograd.grad(out, mask)`` works under ``no_grad``
    callers too.  Parameters are frozen for the call: the result's graph reaches the masks only.  ``model.training``,
    parameters and their ``.grad``, BatchNorm statistics, optimizer state, the engine's step counter and both RNG states are
    left as they were.  Mask values are not validated (no read-back): ``m >= 0`` and finite is the domain."""
    E, N, dev = _sizes(data)
    edge_mask = _check_mask(edge_mask, E, dev, "edge_mask")
    node_mask = _check_mask(node_mask, N, dev, "node_mask")
    with _frozen(model):
        return model._masked_forward(data, edge_mask, node_mask)


class _Setup:
    """What the two methods share: the players of ``data`` in the caller's order."""

    def __init__(self, data, use, undirected, elements):
        E, N, dev = _sizes(data)
        self.use, self.dev = use, dev
        self.M = M = E if use == "edges" else N
        self.B = int(data.num_graphs)
        batch = getattr(data, "batch", None)
        if batch is None:
            batch = torch.zeros(N, dtype=torch.long, device=dev)
        self.gid = batch[data.edge_index[0]] if use == "edges" else batch
        self.twin = None
        member = torch.ones(M, dtype=torch.bool, device=dev)
        if elements is not None:
            if not torch.is_tensor(elements) or elements.dtype != torch.bool:
                raise TypeError("elements must be a bool tensor")
            if elements.dim() != 1 or int(elements.numel()) != M:
                raise ValueError("elements must have one entry per %s (%d)" % ("edge column" if use == "edges" else "node", M))
            member = elements.to(dev)
        self.rep = member
        if undirected is not None:
            from .explain import edge_twins
            self.twin = twin = edge_twins(data)[0]
            t = twin.clamp(min=0).long()
            idx = torch.arange(M, device=dev)
            self.paired = (twin >= 0) & (t != idx)
            member = member | (member[t] & self.paired)             # an undirected edge is asked for by either column
            self.t = t
            self.rep = member & _representatives(twin)               # one representative per player
        self.member = member

    def mask(self, alpha: float):
        """float32 [M] leaf: ``alpha`` on the players, 1 elsewhere."""
        m = torch.ones(self.M, dtype=torch.float32, device=self.dev)
        if alpha != 1.0:
            m = torch.where(self.member, torch.full_like(m, alpha), m)
        return m.requires_grad_(True)

    def score(self, g):
        """fp64 [M] column / node gradients -> player scores: a pair's two gradients summed and given to both, NaN outside."""
        if self.twin is not None:
            g = torch.where(self.paired, g + g[self.t], g)
        return torch.where(self.member, g, torch.full_like(g, float("nan")))

    def graph_sums(self, score):
        """fp64 [B]: the player scores of every graph, each player once, summed in element order."""
        s = torch.where(self.rep, score, torch.zeros_like(score)).cpu()
        return torch.zeros(self.B, dtype=torch.float64).index_add_(0, self.gid.cpu(), s).to(self.dev)


def _p_of(model, data, S, m, h, yhat=None):
    """One forward at mask ``m`` -> ``(p(ŷ) [B], ŷ)``; ŷ is the argmax of head ``h`` unless given."""
    lp = model._masked_forward(data, m if S.use == "edges" else None, m if S.use == "nodes" else None)[h]
    if yhat is None:
        yhat = lp.argmax(-1)
    return _p_at(lp, yhat), yhat


def _grad(p, m):
    (g,) = torch.autograd.grad(p.sum(), m, allow_unused=True)
    return torch.zeros(m.numel(), dtype=torch.float64, device=m.device) if g is None else g.double()


def _check_args(use, undirected, head):
    return _check_driver_args(use, undirected, head, 1)[0]


def saliency(model, data, *, use: str = "edges", undirected=None, head: str = "o", elements=None) -> Gradients:
    """``score = d sum_g p(ŷ_g) / d m`` at ``m = 1``, signed, for every edge column (``use="edges"``) or node (``"nodes"``).

    ŷ_g is the argmax of ``head`` (``"c"``, ``"o"`` or ``"co"``) at ``m = 1``.  Graphs are independent in eval mode, so one
    forward and one backward serve the whole batch.  With ``undirected`` = ``"mean"`` / ``"max"`` / ``"min"`` (all three the
    same here: the names ``explain`` takes) a pair of twin columns (``edge_twins``) is one player with one mask variable: its
    score, the sum of its two columns' gradients, goes to both columns.  ``elements`` (bool [E] / [N]) names the players (an
    undirected edge when either of its columns is named); every other element scores NaN.  An input self-loop column is dropped
    by every convolution and scores exactly 0.  It leaves the model as ``masked_log_probs`` does."""
    h = _check_args(use, undirected, head)
    S = _Setup(data, use, undirected, elements)
    with _frozen(model):
        m = S.mask(1.0)
        p, yhat = _p_of(model, data, S, m, h)
        score = S.score(_grad(p, m))
    return Gradients(score=score, p_full=p.detach(), yhat=yhat, method="saliency", forwards=1, twin=S.twin)


def integrated_gradients(model, data, *, use: str = "edges", undirected=None, head: str = "o", elements=None,
                         steps: int = 32) -> Gradients:
    """Integrated gradients along the straight path from the players at 0 to the players at 1 (every other element stays at 1):
    ``score = (1 / S) sum_{s = 1..S} d sum_g p(ŷ_g) / d m`` at ``m = (s - 1/2) / S`` on the players, accumulated in fp64 on the
    device.  Players, ``head``, ``undirected`` and ``elements`` as in ``saliency``.

    One forward and one backward per step, plus one forward each for ``p_full`` (which fixes ŷ_g) and ``p_baseline`` (every
    player at 0): ``forwards = steps + 2``.  Per graph the player scores sum to ``p_full - p_baseline`` up to the quadrature
    error ``gap`` [B], which falls roughly as ``1 / steps`` (the model has ReLU kinks) and is reported, not bounded.  That is the
    efficiency identity ``shapley`` reports, so the two can be held against each other with ``rank_agreement``, and
    ``perturbation_curve(order=ig.score)`` takes the scores as a ranking.

    The baseline for nodes: with every node of a graph a player, ``p_baseline`` is the readout of a zero pooled row -- what the
    masked forward gives at ``n = 0`` -- not ``shapley``'s convention of ``1 / C`` for a replica without a node.  It leaves the
    model as ``masked_log_probs`` does."""
    h = _check_args(use, undirected, head)
    if isinstance(steps, bool) or not isinstance(steps, int):
        raise TypeError("steps must be an int >= 1")
    if steps < 1:
        raise ValueError("steps must be >= 1")
    S = _Setup(data, use, undirected, elements)
    with _frozen(model):
        with torch.no_grad():
            p_full, yhat = _p_of(model, data, S, S.mask(1.0).detach(), h)
            p_base, _ = _p_of(model, data, S, S.mask(0.0).detach(), h, yhat)
        acc = torch.zeros(S.M, dtype=torch.float64, device=S.dev)
        for s in range(1, steps + 1):
            m = S.mask((s - 0.5) / steps)
            acc += _grad(_p_of(model, data, S, m, h, yhat)[0], m)
        score = S.score(acc / steps)
        gap = S.graph_sums(score) - (p_full.double() - p_base.double())
    return Gradients(score=score, p_full=p_full, yhat=yhat, method="ig", forwards=steps + 2, steps=steps, p_baseline=p_base,
                     gap=gap, twin=S.twin)


def gradient_agreement(model, data, *, method: str = "ig", steps: int = 32, use: str = "edges", undirected=None,
                       head: str = "o", elements=None, ratio=None, k=None) -> dict:
    """Do ``model``'s causal scores rank the elements of ``data`` as their gradient scores do?

    The causal score (column 1 of the soft masks; for edges symmetrised by ``undirected`` exactly as ``explain`` does it) is
    compared per graph with ``integrated_gradients`` (``method="ig"``, ``steps``) or ``saliency`` (``"saliency"``), cast to
    float32, over the players (with ``undirected`` one representative per undirected edge) by one ``rank_agreement`` call.
    Returns ``rho``, ``tau``, ``jaccard`` and their ``_undefined`` counts, ``graphs``, ``elements`` (players compared) and
    ``forwards`` (the method's plus one for the scores): the shape of ``shapley_agreement`` without its ``replicas``."""
    if method not in ("ig", "saliency"):
        raise ValueError('method must be "ig" or "saliency"')
    _check_topk(ratio, k, "gradient_agreement")
    if method == "ig":
        res = integrated_gradients(model, data, use=use, undirected=undirected, head=head, elements=elements, steps=steps)
    else:
        res = saliency(model, data, use=use, undirected=undirected, head=head, elements=elements)
    return _agreement(model, data, res.score, res.forwards, use, undirected, ratio, k)


def _agreement(model, data, score, forwards, use, undirected, ratio, k) -> dict:
    """The causal score against ``score`` ([M], the caller's order) by one ``rank_agreement`` call -> the agreement dict."""
    with _eval_mode(model):
        causal, lay = _causal_in_order(model, data, use)
        score = score.float()
        sel = None
        if use == "edges":
            if lay.order is not None:
                score = score[lay.order].contiguous()
            seg, max_seg = lay.edge_ptr, lay.max_edges
            if undirected is not None:
                twin = lay.twins(data.edge_index)[0]
                causal = _symmetrised(causal, lay, twin, undirected)
                sel = _representatives(twin)
        else:
            seg, max_seg = lay.ptr, lay.max_nodes
        counts, met = rank_agreement(causal.contiguous(), score, seg, max_seg, sel=sel, ratio=ratio, k=k)
        row = torch.cat([_agree_sums(met), counts[:, 0].sum().double().view(1)]).tolist()
    out = _agree_report(row, lay.B)
    out["graphs"], out["elements"], out["forwards"] = lay.B, int(row[6]), forwards + 1
    return out
