"""Parametric edge explanations: one small MLP, trained once with the model frozen, that explains any graph (PGExplainer's
amortised form of the learned mask of ``cal_amd.maskopt``).

``learn_mask`` optimises a mask per batch from nothing, ``steps + 2`` masked forwards each time.  Here the mask is a function of
the model's own node embeddings: with ``x`` [N, H] the backbone output ``edge_att_mlp`` reads, hidden width ``Hd`` and

    PQ [N, 2 Hd] = x [W1a; W1b]^T + [b1; 0]                 (one ``ops.linear``; ``lin1.weight`` = [W1a | W1b])
    h_e = PQ[u, :Hd] + PQ[v, Hd:],    omega(e) = b2 + w2 . relu(h_e)          for a column e = (u -> v)

a player ``p`` (an edge column or an undirected edge: the players of ``saliency(use="edges")``) has ``omega_p`` = its column's, or
the mean of its two columns', a concrete sample ``z_p = (log u - log(1 - u) + omega_p) / tau`` and the mask value ``sigma(z_p)``
on its one or two columns.  Training minimises ``learn_mask``'s objective over a loader,

    sum_g [ -log p_m(ŷ_g) + size_coeff * sum_{p in g} m_p + ent_coeff / P_g * sum_{p in g} H(m_p) ]

with ``tau`` annealed geometrically; afterwards a graph is explained by one backbone pass and ONE launch (``seed = 0``, ``tau = 1``:
``mask = sigma(omega)``).  The MLP runs in ``cal_edge_mlp_fwd`` / ``cal_edge_mlp_bwd`` (csrc/edgemlp.hip) on gathered rows of ``PQ``:
no [E, 2 H] tensor exists.  CAL's ``edge_att_mlp`` is an MLP on the same ``[x_u || x_v]`` trained with the classifier; this is the
post-hoc one trained only to keep the prediction, and ``explainer_agreement`` holds the two against each other.

* ``EdgeExplainer(hidden_in, hidden=64)``: the MLP's parameters (``lin1``, ``lin2``; ``state_dict`` as two ``nn.Linear``).
* ``ExplainerTrainer(model, ...)``: ``.step(batch)`` / ``.fit(loader, device, epochs)``; ``fit_explainer`` wraps both.
* ``explain_edges(model, explainer, data)`` (also ``model.explain_edges``) -> ``ParametricMask``.
* ``explainer_agreement`` / ``eval_explainer``: against the causal attention, against SPMotif's motif.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .explain import _accumulate, _eval_mode, _Layout, _reduce_code, _KEYS
from .gradient import _Setup, _agreement, _check_args, _frozen
from .maskopt import _number, _player_tables
from .plan import plan_of
from .replica import _check_topk, _p_at

__all__ = ["EdgeExplainer", "EdgePlayers", "ExplainerTrainer", "ParametricMask", "fit_explainer", "explain_edges",
           "explainer_agreement", "eval_explainer"]


@dataclass
class ParametricMask:
    """The explainer's mask of a batch.  ``mask`` float32 [E] in the caller's order: the player's ``sigmoid(omega)``, NaN for a
    column that is no player; both columns of an undirected edge carry the same bits.  ``omega`` float32 [E]: the player's logit,
    laid out the same way.  ``yhat`` int64 [B] and ``p_full`` [B]: the argmax of the chosen head at ``m = 1`` and its probability;
    ``p_masked`` [B]: the probability of ŷ under the mask.  ``forwards = 2`` (the one at ``m = 1`` and the masked one; the MLP
    itself takes the backbone once more, up to the embeddings).  ``twin``: the reverse-column map int32 [E] when ``undirected``
    built one."""
    mask: torch.Tensor
    omega: torch.Tensor
    p_full: torch.Tensor
    p_masked: torch.Tensor
    yhat: torch.Tensor
    forwards: int = 2
    twin: Optional[torch.Tensor] = None


def _check_hidden(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError("%s must be an int" % what)
    if v < 4 or v > 256 or v % 4:
        raise ValueError("%s must be a multiple of 4 in [4, 256]" % what)
    return v


def _check_int(v, what, low):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError("%s must be an int >= %d" % (what, low))
    if v < low:
        raise ValueError("%s must be >= %d" % (what, low))
    return v


class EdgeExplainer(nn.Module):
    """The edge MLP ``[x_u || x_v] -> Hd -> 1``: ``lin1.weight`` [Hd, 2 hidden_in], ``lin1.bias`` [Hd], ``lin2.weight`` [1, Hd],
    ``lin2.bias`` [1], initialised as ``torch.nn.Linear`` does (uniform in ``+-1 / sqrt(fan_in)``) from a generator seeded with
    ``seed``: the global RNG is not touched.  ``hidden`` (``Hd``): a multiple of 4 in [4, 256]."""

    def __init__(self, hidden_in: int, hidden: int = 64, seed: int = 0):
        super().__init__()
        self.hidden_in, self.hidden = _check_int(hidden_in, "hidden_in", 1), _check_hidden(hidden, "hidden")
        g = torch.Generator().manual_seed(_check_int(seed, "seed", 0))
        with torch.random.fork_rng(devices=[]):
            self.lin1, self.lin2 = nn.Linear(2 * hidden_in, hidden), nn.Linear(hidden, 1)
        with torch.no_grad():
            for lin in (self.lin1, self.lin2):
                bound = 1.0 / math.sqrt(lin.in_features)
                lin.weight.copy_(torch.empty(lin.weight.shape).uniform_(-bound, bound, generator=g))
                lin.bias.copy_(torch.empty(lin.bias.shape).uniform_(-bound, bound, generator=g))

    def projection(self):
        """``([W1a; W1b] [2 Hd, H], [b1; 0] [2 Hd])``: the weight and bias of the node projection ``PQ``."""
        H = self.hidden_in
        w = self.lin1.weight
        return torch.cat([w[:, :H], w[:, H:]], 0).contiguous(), torch.cat([self.lin1.bias, torch.zeros_like(self.lin1.bias)])

    def forward(self, x, plan, players, tau: float = 1.0, seed: int = 0, step: int = 0, size_coeff: float = 0.0,
                ent_coeff: float = 0.0, full: bool = False):
        """``ops.edge_mlp_mask`` of this MLP on the embeddings ``x`` [N, hidden_in]: one ``ops.linear`` and one launch."""
        if x.dim() != 2 or x.size(1) != self.hidden_in:
            raise ValueError("the embeddings must be [N, %d]" % self.hidden_in)
        w, b = self.projection()
        pq = ops.linear(x, w, b)
        return ops.edge_mlp_mask(pq, self.lin2.weight.view(-1), self.lin2.bias, plan, players, tau, seed, step, size_coeff, ent_coeff,
                                 full=full)


class EdgePlayers:
    """The edge players of a batch for the kernels: ``pptr`` int64 [B + 1], ``rep`` / ``mate`` int32 [P] (``MaskOptimizer``'s
    tables), ``cnt`` fp64 [B] players per graph, ``member`` bool [E], ``twin``.  Built once per batch (it reads sizes back, as
    the plan of a batch does) and kept on the batch object when no ``elements`` are given."""

    def __init__(self, data, undirected=None, elements=None):
        S = _Setup(data, "edges", undirected, elements)
        self.pptr, self.rep, self.mate = _player_tables(data, S)
        self.B, self.E, self.P = S.B, S.M, int(self.rep.numel())
        self.cnt = (self.pptr[1:] - self.pptr[:-1]).double()
        self.member, self.twin = S.member, S.twin
        ei = data.edge_index
        self.loops = bool((ei[0] == ei[1]).any()) if self.E else False
        self._csr = None

    def csr(self, plan):
        """``(rowptr_src, eid_src, rowptr_dst, eid_dst)`` that list every column once per view: the plan's, unless the batch has
        input self loops (which the plan's leave out: no convolution reads them, but they are players here); then two of their
        own, slots of a row in column order."""
        if not self.loops:
            return plan.rowptr_src, plan.eid_src, plan.rowptr_dst, plan.eid_dst
        if self._csr is None:
            out = []
            for key in (plan.row32, plan.col32):
                key = key.long()
                ptr = torch.zeros(plan.N + 1, dtype=torch.int32, device=key.device)
                ptr[1:] = torch.cumsum(torch.bincount(key, minlength=plan.N), 0)
                out += [ptr, torch.argsort(key, stable=True).to(torch.int32).contiguous()]
            self._csr = tuple(out)
        return self._csr

    @staticmethod
    def of(data, undirected=None, elements=None):
        if elements is not None:
            return EdgePlayers(data, undirected, elements)
        cache = getattr(data, "_edge_players", None)
        if cache is None or cache[0] != data.edge_index.data_ptr():
            cache = (data.edge_index.data_ptr(), {})
            try:
                data._edge_players = cache
            except Exception:
                pass
        if undirected not in cache[1]:
            cache[1][undirected] = EdgePlayers(data, undirected)
        return cache[1][undirected]


def _check_explainer(model, explainer):
    if not isinstance(explainer, EdgeExplainer):
        raise TypeError("explainer must be an EdgeExplainer")
    H = model.edge_att_mlp.in_features // 2
    if explainer.hidden_in != H:
        raise ValueError("the explainer reads embeddings of width %d, the model's are %d" % (explainer.hidden_in, H))
    p0, q0 = next(model.parameters()), next(explainer.parameters())
    if p0.device != q0.device:
        raise ValueError("the explainer is on %s, the model on %s" % (q0.device, p0.device))
    return explainer


class ExplainerTrainer:
    """Adam over an ``EdgeExplainer``'s parameters with ``model`` frozen.

    ``temp = (t0, t1)``: ``tau`` of step ``t`` is ``t0 (t1 / t0)^(t / (total_steps - 1))``, held at ``t1`` afterwards
    (``total_steps``: ``fit`` sets it to ``epochs * len(loader)`` when it is ``None``; a bare ``step`` then stays at ``t0``).
    ``seed``: of the concrete noise (step ``t`` is keyed by ``(seed, t, player)``; 0: no noise) and, when no ``explainer`` is
    given, of the new one's initialisation.  ``head`` / ``undirected`` as in ``saliency``.  ``history`` fp64
    [steps, B_max, 3]: per graph ``(-log p_m(ŷ), size_coeff * sum m, ent_coeff / P_g * sum H(m))`` of every step's sampled
    mask, NaN beyond a batch's graphs.  Every call leaves the model as ``masked_log_probs`` does."""

    def __init__(self, model, explainer=None, *, hidden: int = 64, lr: float = 0.003, temp=(5.0, 2.0), size_coeff: float = 0.05,
                 ent_coeff: float = 1.0, head: str = "o", undirected="mean", seed: int = 1, total_steps=None):
        self.h = _check_args("edges", undirected, head)
        self.undirected = undirected
        self.lr = _number(lr, "lr", positive=True)
        self.size_coeff, self.ent_coeff = _number(size_coeff, "size_coeff"), _number(ent_coeff, "ent_coeff")
        if not isinstance(temp, (tuple, list)) or len(temp) != 2:
            raise ValueError("temp must be a pair (start, end)")
        self.temp = tuple(_number(t, "temp", positive=True) for t in temp)
        self.seed = _check_int(seed, "seed", 0)
        self.total_steps = None if total_steps is None else _check_int(total_steps, "total_steps", 1)
        if explainer is None:
            explainer = EdgeExplainer(model.edge_att_mlp.in_features // 2, _check_hidden(hidden, "hidden"), seed=self.seed)
            explainer.to(next(model.parameters()).device)
        self.model, self.explainer = model, _check_explainer(model, explainer)
        self.opt = torch.optim.Adam(self.explainer.parameters(), lr=self.lr)
        self.t = 0
        self._hist = None

    def temperature(self, t: int) -> float:
        t0, t1 = self.temp
        T = self.total_steps or 1
        return t0 * (t1 / t0) ** (min(t, T - 1) / max(T - 1, 1))

    def _row(self, k, B, dev):
        """Row ``k`` of the history for ``B`` graphs: the buffer doubles along either axis when it is too small (sizes known on the
        host: no read-back)."""
        old = self._hist
        if old is None or k >= old.size(0) or B > old.size(1):
            cap = 128 if old is None else old.size(0) * (2 if k >= old.size(0) else 1)
            new = torch.full((cap, B if old is None else max(B, old.size(1)), 3), float("nan"), dtype=torch.float64, device=dev)
            if old is not None:
                new[:old.size(0), :old.size(1)] = old
            self._hist = new
        return self._hist[k, :B]

    @property
    def history(self):
        dev = next(self.explainer.parameters()).device
        return torch.empty(0, 0, 3, dtype=torch.float64, device=dev) if self._hist is None else self._hist[:self.t].clone()

    def step(self, data, elements=None):
        """One training step on ``data``: the embeddings, one ``ops.linear``, one ``edge_mlp_mask``, one ``_masked_forward`` under
        frozen parameters, one backward, one Adam update.  ŷ comes from a forward at ``m = 1`` and stays on the device; the
        per-graph loss rows go to the preallocated history.  Nothing the step computes is read back (the player tables of a
        batch are built on its first visit, as its plan is)."""
        model, ex = self.model, self.explainer
        pl = EdgePlayers.of(data, self.undirected, elements)
        plan = plan_of(data)
        x = model._node_embeddings(data)
        row = self._row(self.t, pl.B, x.device)
        with _frozen(model):
            with torch.no_grad():
                yhat = model._masked_forward(data, None)[self.h].argmax(-1)
            mask, terms = ex(x, plan, pl, self.temperature(self.t), self.seed, self.t, self.size_coeff, self.ent_coeff)
            nll = -model._masked_forward(data, mask)[self.h].gather(-1, yhat.unsqueeze(-1)).squeeze(-1)
            self.opt.zero_grad(set_to_none=True)
            nll.sum().backward()
        self.opt.step()
        row[:, 0] = nll.detach()
        row[:, 1] = self.size_coeff * terms[:, 0]
        row[:, 2] = torch.where(pl.cnt > 0, self.ent_coeff * terms[:, 1] / pl.cnt.clamp(min=1.0), torch.zeros_like(pl.cnt))
        self.t += 1

    def fit(self, loader, device, epochs: int = 10):
        """``epochs`` passes over ``loader`` (batches are moved to ``device``) -> the history."""
        _check_int(epochs, "epochs", 1)
        if self.total_steps is None:
            self.total_steps = max(1, epochs * len(loader))
        for _ in range(epochs):
            for data in loader:
                self.step(data.to(device))
        return self.history


def fit_explainer(model, loader, device, *, epochs: int = 10, explainer=None, **kw):
    """Train an ``EdgeExplainer`` for ``model`` over ``loader`` (``ExplainerTrainer(model, explainer, **kw).fit``) ->
    ``(explainer, history)``."""
    tr = ExplainerTrainer(model, explainer, **kw)
    return tr.explainer, tr.fit(loader, device, epochs)


def explain_edges(model, explainer, data, *, undirected="mean", elements=None, head: str = "o") -> ParametricMask:
    """The explainer's mask of ``data``: one backbone pass for the embeddings, one ``ops.linear`` and ONE launch for
    ``mask = sigmoid(omega)`` (no noise, ``tau = 1``), then the forward at ``m = 1`` (ŷ, ``p_full``) and the masked one
    (``p_masked``): ``forwards = 2``.  Players, ``head``, ``undirected`` and ``elements`` as in ``saliency``.  In eval mode the
    embeddings of a graph do not depend on the rest of its batch, so neither does its mask.  ``perturbation_curve(order=res.mask)``
    takes the result as a ranking.  It leaves the model as ``masked_log_probs`` does."""
    h = _check_args("edges", undirected, head)
    _check_explainer(model, explainer)
    pl = EdgePlayers.of(data, undirected, elements)
    x = model._node_embeddings(data)
    with _frozen(model), torch.no_grad():
        mask, _, omega, _ = explainer(x, plan_of(data), pl, full=True)
        lp = model._masked_forward(data, None)[h]
        yhat = lp.argmax(-1)
        p_full = _p_at(lp, yhat)
        p_masked = _p_at(model._masked_forward(data, mask)[h], yhat)
    nan = torch.full_like(mask, float("nan"))
    om = nan.clone()
    om[pl.rep.long()] = omega
    has = pl.mate >= 0
    om[torch.where(has, pl.mate, pl.rep).long()] = omega
    return ParametricMask(mask=torch.where(pl.member, mask, nan), omega=om, p_full=p_full, p_masked=p_masked, yhat=yhat, forwards=2,
                          twin=pl.twin)


def explainer_agreement(model, explainer, data, *, undirected="mean", elements=None, head: str = "o", ratio=None, k=None) -> dict:
    """Do ``model``'s causal scores rank the edges of ``data`` as the explainer's mask does?  ``gradient_agreement`` with
    ``explain_edges``' mask in the place of the gradient score: ``rho``, ``tau``, ``jaccard`` and their ``_undefined`` counts,
    ``graphs``, ``elements`` (players compared) and ``forwards`` (3)."""
    _check_topk(ratio, k, "explainer_agreement")
    res = explain_edges(model, explainer, data, undirected=undirected, elements=elements, head=head)
    return _agreement(model, data, res.mask, res.forwards, "edges", undirected, ratio, k)


def eval_explainer(model, explainer, loader, device, *, k="gt", ratio=None, undirected="mean") -> dict:
    """Mean edge precision@k, recall@k and ROC-AUC of the explainer's mask against the SPMotif motif (``spmotif.ground_truth``)
    over the graphs where each is defined, as ``eval_explanation`` reports them for the causal attention, by the same ranking
    (``rank_segments`` / ``rank_segment_pairs``): ``precision``, ``recall``, ``auc``, and ``graphs`` and ``selected`` (the sum of
    the per-graph k: with ``k="gt"`` the number of motif edges).  Per mini-batch one backbone pass, one launch for the mask and
    one ranking call; the sums stay on the device until one read-back at the end."""
    from .spmotif import ground_truth
    _reduce_code(undirected)
    _check_explainer(model, explainer)
    if ratio is not None:
        k = None
    sums = torch.zeros(8, dtype=torch.float64, device=device)
    for data in loader:
        data = data.to(device)
        pl = EdgePlayers.of(data, undirected)
        x = model._node_embeddings(data)
        with torch.no_grad():
            score = explainer(x, plan_of(data), pl)[0]
        with _eval_mode(model):
            edge_gt = ground_truth(data)[1]
            lay = _Layout(data)
            if undirected is None:
                met = lay.rank_edges(score, ratio=ratio, k=k, gt=edge_gt, metrics=True)[2]
            else:
                met = lay.rank_edge_pairs(score, data.edge_index, undirected, ratio=ratio, k=k, gt=edge_gt, metrics=True)[2]
        _accumulate(sums, met, 0)
        sums[6] += met[:, 0].sum()
        sums[7] += met.size(0)
    s = sums.tolist()
    out = {key: (s[2 * i] / s[2 * i + 1] if s[2 * i + 1] else float("nan")) for i, key in enumerate(_KEYS)}
    out["selected"], out["graphs"] = int(s[6]), int(s[7])
    return out
