"""Learned mask explanations: a soft mask per graph, trained to keep the model's prediction while being small and near-binary
(GNNExplainer's objective over this project's soft-mask forward).

``cal_amd.gradient`` differentiates ``masked_log_probs`` once (saliency) or along a straight path (integrated gradients).  This
module optimises over it: every player ``p`` (an edge column, an undirected edge or a node: the players of ``saliency``) has one
logit ``theta_p`` and carries ``m_p = sigmoid(theta_p)`` on its one or two elements; every other element stays at 1.  With ŷ_g
the argmax of ``head`` at ``m = 1`` and ``P_g`` the number of players of graph g the loss is

    L = sum_g [ -log p_m(ŷ_g) + size_coeff * sum_{p in g} m_p + ent_coeff / P_g * sum_{p in g} H(m_p) ]
    H(m) = -m log m - (1 - m) log(1 - m) = softplus(theta) - theta * sigmoid(theta)

and is minimised by Adam over ``theta`` with the model's parameters frozen.  One optimiser step is one masked forward, one
``autograd.grad`` with respect to the mask, and ONE launch of ``cal_mask_step`` (csrc/maskopt.hip) for everything else: the twin
gather of the gradient, both regularisers with their closed-form gradients, Adam with bias correction, the scatter of
``sigmoid(theta_new)`` back to the mask and the per-graph sums of the loss history.

* ``MaskOptimizer(model, data, ...)``: the state (``theta``, both Adam moments, ``mask``) and ``.step()`` / ``.result()``.
* ``learn_mask(model, data, steps=100, ...)`` (also ``model.learn_mask``) -> ``LearnedMask``.
* ``mask_agreement(model, data, steps=..., ratio= | k=, ...)``: the causal attention against the learned mask.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .explain import _Layout
from .gradient import _Setup, _agreement, _check_args, _frozen
from .plan import _c
from .replica import _check_topk, _p_at

__all__ = ["LearnedMask", "MaskOptimizer", "learn_mask", "mask_agreement"]


@dataclass
class LearnedMask:
    """A learned mask of a batch.  ``mask`` float32 [E] (``use="edges"``) or [N] (``"nodes"``) in the caller's order: the
    player's ``sigmoid(theta)``, NaN for an element that is no player; both columns of an undirected edge carry the same bits.
    ``theta`` float32 [P]: the players' logits, grouped by graph (in element order inside a graph).  ``yhat`` int64 [B] and
    ``p_full`` [B]: the argmax of the chosen head at ``m = 1`` and its probability; ``p_masked`` [B]: the probability of ŷ under
    the final mask.  ``loss`` fp64 [steps + 1, B, 3]: per graph ``(-log p_m(ŷ), size_coeff * sum m, ent_coeff / P_g * sum H(m))``
    of the mask each step differentiated at (row 0: the initial mask) and, in the last row, of the final mask; a graph's loss is
    the sum of its three.  ``forwards = steps + 2``.  ``twin``: the reverse-column map int32 [E] when ``undirected`` built one."""
    mask: torch.Tensor
    theta: torch.Tensor
    p_full: torch.Tensor
    p_masked: torch.Tensor
    yhat: torch.Tensor
    loss: torch.Tensor
    steps: int
    forwards: int
    twin: Optional[torch.Tensor] = None


def _number(v, what, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s must be a number" % what)
    if not (v > 0 if positive else v >= 0) or v != v or v == float("inf"):
        raise ValueError("%s must be %s and finite" % (what, "> 0" if positive else ">= 0"))
    return float(v)


def _player_tables(data, S):
    """The players of ``S`` (a ``gradient._Setup`` of ``data``) in graph order, the representatives of ``_Setup`` over the segments
    of ``_Layout`` -> ``(pptr int64 [B + 1], rep int32 [P], mate int32 [P])``: a player's first element and its twin column or
    -1; columns that are not grouped by graph need no reordering."""
    dev, M = S.dev, S.M
    lay = _Layout(data)
    order, seg = (lay.order, lay.edge_ptr) if S.use == "edges" else (None, lay.ptr)
    rep_o = S.rep if order is None else S.rep[order]
    elems = torch.arange(M, device=dev) if order is None else order
    rep = elems[rep_o]
    pptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(rep_o.long(), 0)])[seg.long()].contiguous()
    if S.twin is not None:
        mate = torch.where(S.paired[rep], S.t[rep], torch.full_like(rep, -1)).to(torch.int32).contiguous()
    else:
        mate = torch.full((int(rep.numel()),), -1, dtype=torch.int32, device=dev)
    return pptr, rep.to(torch.int32).contiguous(), mate


class MaskOptimizer:
    """Adam over the mask logits of ``data``'s players (``use``, ``undirected``, ``elements``, ``head`` as in ``saliency``).

    Holds ``theta``, ``exp_avg``, ``exp_avg_sq`` (float32 [P], players grouped by graph), ``mask`` (float32 [M], the caller's
    order; 1 outside the players), the player tables ``pptr`` int64 [B + 1] / ``rep`` / ``mate`` int32 [P] (the player's first
    element and its twin column or -1; built once, on the device of the batch; columns that are not grouped by graph need no
    reordering), and ``yhat`` / ``p_full`` from one forward at ``m = 1``.  ``init``: one float for every ``theta_p`` or a float32
    tensor with one entry per element (a player reads its first element's); nothing is drawn at random.

    An input self-loop column is an ordinary player: every convolution drops it, so its prediction gradient is exactly 0 and
    only the regularisers move it.  In eval mode the graphs of a batch are independent and Adam is per coordinate, so a graph's
    learned mask does not depend on the rest of its batch.

    Every call leaves the model as ``masked_log_probs`` does."""

    def __init__(self, model, data, *, use: str = "edges", undirected=None, head: str = "o", elements=None, lr: float = 0.01,
                 betas=(0.9, 0.999), eps: float = 1e-8, size_coeff: float = 0.005, ent_coeff: float = 1.0, init=1.0):
        self.h = _check_args(use, undirected, head)
        self.lr = _number(lr, "lr", positive=True)
        self.eps = _number(eps, "eps")
        self.size_coeff, self.ent_coeff = _number(size_coeff, "size_coeff"), _number(ent_coeff, "ent_coeff")
        if len(betas) != 2:
            raise ValueError("betas must be a pair")
        self.betas = tuple(_number(b, "betas") for b in betas)
        if max(self.betas) >= 1.0:
            raise ValueError("betas must be in [0, 1)")
        self.model, self.data = model, data
        self.S = S = _Setup(data, use, undirected, elements)
        dev, M, B = S.dev, S.M, S.B
        if torch.is_tensor(init):
            if init.dtype != torch.float32:
                raise TypeError("an init tensor must be float32")
            if init.dim() != 1 or int(init.numel()) != M:
                raise ValueError("an init tensor must have one entry per %s (%d)" % ("edge column" if use == "edges" else "node", M))
            init = init.to(dev)
        else:
            if isinstance(init, bool) or not isinstance(init, (int, float)):
                raise TypeError("init must be a float or a float32 tensor")
            init = torch.full((M,), float(init), dtype=torch.float32, device=dev)
        self.pptr, self.rep, self.mate = _player_tables(data, S)
        self.P = P = int(self.rep.numel())
        self.B, self.M = B, M
        self.theta = init[self.rep.long()].contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.mask = torch.ones(M, dtype=torch.float32, device=dev)
        self.t = 0
        self._cap = 128                                        # rows of the history; doubled when full
        self._pred = torch.zeros(self._cap, B, dtype=torch.float64, device=dev)
        self._terms = torch.zeros(self._cap, B, 2, dtype=torch.float64, device=dev)
        with _frozen(model), torch.no_grad():
            lp = self._forward(self.mask)
            self.yhat = lp.argmax(-1)
            self.p_full = _p_at(lp, self.yhat)
        self._kernel(0, None, None)                            # the initial scatter: mask = sigmoid(theta) on the players

    def _forward(self, m):
        e = self.S.use == "edges"
        return self.model._masked_forward(self.data, m if e else None, None if e else m)[self.h]

    def _kernel(self, step, grad, terms):
        _c("cal_mask_step", self.pptr, self.rep, self.mate, grad, self.theta, self.exp_avg, self.exp_avg_sq, self.mask, terms,
           self.B, self.P, self.M, step, self.lr, self.betas[0], self.betas[1], self.eps, self.size_coeff, self.ent_coeff)

    def _row(self, k):
        """Rows of the history up to ``k``: the buffers double when they are full (no read-back: ``k`` is a host counter)."""
        if k >= self._cap:
            self._cap *= 2
            for name in ("_pred", "_terms"):
                old = getattr(self, name)
                new = torch.zeros((self._cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
                new[:old.size(0)] = old
                setattr(self, name, new)
        return self._pred[k], self._terms[k]

    def step(self):
        """One optimiser step: one masked forward under frozen parameters, one ``autograd.grad`` of ``-sum_g log p_m(ŷ_g)``
        with respect to the mask, one ``cal_mask_step``.  The per-graph ``(pred, size, ent)`` of the mask it differentiated at
        go to the preallocated device history.  There is NO host read-back in here: every size is known from construction, the
        step number is a host counter, and nothing of the result is looked at."""
        pred, terms = self._row(self.t)
        with _frozen(self.model):
            m = self.mask.detach().requires_grad_(True)
            lp = self._forward(m)
            nll = -lp.gather(-1, self.yhat.unsqueeze(-1)).squeeze(-1)
            (g,) = torch.autograd.grad(nll.sum(), m, allow_unused=True)
        pred.copy_(nll.detach())
        g = torch.zeros_like(self.mask) if g is None else g.contiguous()
        self.t += 1
        self._kernel(self.t, g, terms)

    def result(self) -> LearnedMask:
        """One closing forward at the current mask -> ``LearnedMask`` (the state is not changed: more steps may follow)."""
        k = self.t
        pred, terms = self._row(k)
        with _frozen(self.model), torch.no_grad():
            nll = -self._forward(self.mask).gather(-1, self.yhat.unsqueeze(-1)).squeeze(-1)
        pred.copy_(nll)
        self._kernel(0, None, terms)
        cnt = (self.pptr[1:] - self.pptr[:-1]).double()
        w = torch.stack([torch.full_like(cnt, self.size_coeff),
                         torch.where(cnt > 0, self.ent_coeff / cnt.clamp(min=1.0), torch.zeros_like(cnt))], -1)
        loss = torch.cat([self._pred[:k + 1].unsqueeze(-1), self._terms[:k + 1] * w], -1)
        mask = torch.where(self.S.member, self.mask, torch.full_like(self.mask, float("nan")))
        return LearnedMask(mask=mask, theta=self.theta.clone(), p_full=self.p_full, p_masked=(-nll).exp(), yhat=self.yhat, loss=loss,
                           steps=k, forwards=k + 2, twin=self.S.twin)


def _check_steps(steps):
    if isinstance(steps, bool) or not isinstance(steps, int):
        raise TypeError("steps must be an int >= 1")
    if steps < 1:
        raise ValueError("steps must be >= 1")


def learn_mask(model, data, *, steps: int = 100, use: str = "edges", undirected=None, head: str = "o", elements=None,
               lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8, size_coeff: float = 0.005, ent_coeff: float = 1.0,
               init=1.0) -> LearnedMask:
    """``steps`` Adam steps of ``MaskOptimizer`` from ``init`` and one closing forward at the final mask -> ``LearnedMask``
    (``forwards = steps + 2``).  The defaults are GNNExplainer's.  Players, ``head``, ``undirected`` and ``elements`` as in
    ``saliency``; ``steps`` an int >= 1, ``lr > 0``, both coefficients >= 0, an ``init`` tensor float32 with one entry per
    element.  ``perturbation_curve(order=res.mask)`` takes the result as a ranking.  It leaves the model as ``masked_log_probs``
    does."""
    _check_steps(steps)
    opt = MaskOptimizer(model, data, use=use, undirected=undirected, head=head, elements=elements, lr=lr, betas=betas, eps=eps,
                        size_coeff=size_coeff, ent_coeff=ent_coeff, init=init)
    for _ in range(steps):
        opt.step()
    return opt.result()


def mask_agreement(model, data, *, steps: int = 100, use: str = "edges", undirected=None, head: str = "o", elements=None,
                   ratio=None, k=None, **kw) -> dict:
    """Do ``model``'s causal scores rank the elements of ``data`` as their learned mask does?  ``gradient_agreement`` with
    ``learn_mask(steps=steps, **kw)``'s mask in the place of the gradient score: ``rho``, ``tau``, ``jaccard`` and their
    ``_undefined`` counts, ``graphs``, ``elements`` (players compared) and ``forwards`` (``learn_mask``'s plus one)."""
    _check_topk(ratio, k, "mask_agreement")
    res = learn_mask(model, data, steps=steps, use=use, undirected=undirected, head=head, elements=elements, **kw)
    return _agreement(model, data, res.mask, res.forwards, use, undirected, ratio, k)
