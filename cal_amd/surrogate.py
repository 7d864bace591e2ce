"""Surrogate attributions: KernelSHAP and a local linear fit, one weighted least-squares problem per graph.

The other attribution drivers assume that the model is additive around a graph; none fits an additive model, and none says how
additive the model is.  This module samples coalitions of a graph's players directly (``coalition_batch`` replicas: a random
order per draw, a prefix of it and, for KernelSHAP, the prefix's complement), runs them, and fits the replicas' ``p(ŷ)`` on the
players' membership bits:

* ``surrogate_fit(key, rep_ptr, rep_row, rep_thresh, value, pl_ptr, pl_elem, ...)`` -> ``(phi, phi0, r2, status)``: the fit
  (``cal_surrogate_fit``: ONE launch on the GPU, one workgroup per graph, the matrix in LDS, no workspace and no read-back;
  libcalhost for CPU tensors, the same bits).
* ``kernel_shap(model, data, samples=...)`` (also ``model.kernel_shap``) -> ``Surrogate``: Shapley values from a FIXED replica
  budget per graph, whatever the number of players; the scores of a graph sum to ``p_full - p_empty`` by construction.
* ``local_surrogate(model, data, samples=..., keep=..., width=...)`` (also ``model.local_surrogate``) -> ``Surrogate``: LIME's
  surrogate, a free intercept and a locality kernel; its weighted ``r2`` measures how additive the model is around the graph.
* ``surrogate_agreement(model, data, ...)`` / ``eval_surrogate(model, loader, device, ...)``: the causal attention against the
  surrogate's scores, through ``rank_agreement``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .coalition import _draw_keys, _run_replicas, coalition_batch
from .explain import _eval_mode, _Layout
from .occlude import rank_agreement
from .plan import _p, _stream
from .replica import (_agree_report, _agree_sums, _causal_in_order, _check_driver_args, _check_replicas, _check_topk, _grouped,
                      _members, _Players, _symmetrised, _whole)

__all__ = ["Surrogate", "surrogate_fit", "kernel_shap", "local_surrogate", "surrogate_agreement", "eval_surrogate", "MAX_PLAYERS",
           "STATUS"]

#: the largest player count of a graph on the GPU path (``kSurrogateMaxPlayers`` of rules.hpp); the host library has no limit
MAX_PLAYERS = 127
#: what ``status`` says
STATUS = {0: "fitted", 1: "rank-deficient", 2: "more than %d players" % MAX_PLAYERS, 3: "a non-finite value or a bad weight"}
_MODES = {"shap": 0, "lime": 1, 0: 0, 1: 1}


def _i64(t, what, dev):
    if not torch.is_tensor(t) or t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("%s must be a 1-D integer tensor" % what)
    if t.device != dev:
        raise ValueError("%s must be on the device of key" % what)
    return t.to(torch.long).contiguous()


def _f64(t, what, dev, n):
    if not torch.is_tensor(t) or t.dim() != 1 or int(t.numel()) != n:
        raise ValueError("%s must be a 1-D tensor of %d entries" % (what, n))
    if t.device != dev:
        raise ValueError("%s must be on the device of key" % what)
    return t.to(torch.float64).contiguous()


def surrogate_fit(key, rep_ptr, rep_row, rep_thresh, value, pl_ptr, pl_elem, *, rep_invert=None, weight=None, v_empty=None,
                  v_full=None, mode="shap", ridge: float = 0.0):
    """One weighted least-squares fit per graph of the replicas' values on the players' membership bits.

    ``key`` int32 [K, M] (or [M]) are the key rows ``coalition_batch`` took; graph g has the samples ``rep_ptr[g] ..
    rep_ptr[g + 1]`` (int64 [B + 1]; ``rep_row``, ``rep_thresh`` and the optional ``rep_invert`` int64 [R]; ``value`` [R], the
    optional ``weight`` [R], ones by default) and the players ``pl_elem[pl_ptr[g] .. pl_ptr[g + 1]]`` (the element of each
    player's representative).  Sample s holds player p iff ``(key[rep_row[s], pl_elem[p]] < rep_thresh[s]) != (rep_invert[s] !=
    0)``; a row outside ``[0, K)`` holds every player.

    ``mode="shap"``: n unknowns, ``y = v - v_empty[g]``, the solution corrected onto ``sum(phi) = v_full[g] - v_empty[g]``,
    ``phi0 = v_empty[g]``; one player is defined as ``phi = v_full - v_empty``.  ``mode="lime"``: a free intercept (``phi0``),
    ``y = v``, ``ridge`` on the players' diagonal entries only; ``v_empty`` / ``v_full`` are not read.  -> ``phi`` fp64 [P],
    ``phi0`` fp64 [B], ``r2`` fp64 [B] (weighted, NaN when the values do not vary) and ``status`` int32 [B] (``STATUS``: 0 fitted,
    1 rank-deficient by the pivot rule ``d_j > 2^-30 A_jj``, 2 more than 127 players -- GPU only --, 3 a non-finite value or a
    negative or non-finite weight; non-zero: NaN results).  Every sum has one order (the surrogate block of rules.hpp): CUDA
    tensors (``cal_surrogate_fit``, one launch on the current stream, nothing read back, safe to capture) and CPU tensors
    (libcalhost) give the same bits, and a graph's result does not depend on the rest of its batch."""
    if mode not in _MODES:
        raise ValueError('mode must be "shap" or "lime"')
    m = _MODES[mode]
    ridge = float(ridge)
    if not (ridge >= 0.0 and ridge != float("inf")):
        raise ValueError("ridge must be finite and >= 0")
    if not torch.is_tensor(key) or key.dtype != torch.int32 or key.dim() not in (1, 2):
        raise TypeError("key must be an int32 tensor [K, M] or [M]")
    key = (key.view(1, -1) if key.dim() == 1 else key).contiguous()
    K, M, dev = int(key.size(0)), int(key.size(1)), key.device
    rep_ptr, pl_ptr = _i64(rep_ptr, "rep_ptr", dev), _i64(pl_ptr, "pl_ptr", dev)
    B = int(rep_ptr.numel()) - 1
    if B < 0 or int(pl_ptr.numel()) != B + 1:
        raise ValueError("rep_ptr and pl_ptr must have B + 1 entries each")
    rrow, rth, pel = _i64(rep_row, "rep_row", dev), _i64(rep_thresh, "rep_thresh", dev), _i64(pl_elem, "pl_elem", dev)
    R, Pn = int(rrow.numel()), int(pel.numel())
    if int(rth.numel()) != R:
        raise ValueError("rep_row and rep_thresh must have one entry per replica each")
    rinv = None
    if rep_invert is not None:
        rinv = _i64(rep_invert, "rep_invert", dev)
        if int(rinv.numel()) != R:
            raise ValueError("rep_invert must have one entry per replica")
    val = _f64(value, "value", dev, R)
    wt = None if weight is None else _f64(weight, "weight", dev, R)
    ve = vf = None
    if m == 0:
        if v_empty is None or v_full is None:
            raise ValueError('mode "shap" needs v_empty and v_full')
        ve, vf = _f64(v_empty, "v_empty", dev, B), _f64(v_full, "v_full", dev, B)
    phi = torch.empty(Pn, dtype=torch.float64, device=dev)
    phi0, r2 = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    host = not key.is_cuda
    nz = lambda t: _p(t) if t is not None and t.numel() else None
    _lib.call("cal_surrogate_fit", nz(key), K, M, _p(rep_ptr), nz(rrow), nz(rth), nz(rinv), nz(val), nz(wt), R, _p(pl_ptr), nz(pel),
              Pn, B, nz(ve), nz(vf), m, ridge, nz(phi), nz(phi0), nz(r2), nz(status), None if host else _stream(), host=host)
    return phi, phi0, r2, status


# ---- the drivers ----------------------------------------------------------------------------------------------------------------
@dataclass
class Surrogate:
    """A surrogate fit of a batch.  ``score`` fp64 [E] (``use="edges"``) or [N] (``"nodes"``): the player's coefficient, on both
    columns of an undirected edge, NaN for an element that is no player.  ``phi0`` fp64 [B]: the surrogate's value with no player
    present (``kernel_shap``: ``p_empty``; ``local_surrogate``: the fitted intercept).  ``p_full`` [B], ``yhat`` int64 [B]: the
    whole graph's probability of its own argmax, and that argmax; ``p_empty`` fp64 [B]: the probability with no player present
    (``kernel_shap`` only, else ``None``).  ``r2`` fp64 [B]: the weighted coefficient of determination of the fit over its own
    samples, NaN where the values do not vary; ``status`` int32 [B] (all zero: anything else raised).  ``replicas``: graphs run
    besides the whole batch, in ``forwards`` forwards (the whole batch's included).  ``twin``: the reverse-column map int32 [E]
    when ``undirected`` built one.  ``keys`` int32 [K, M]: the key rows the replicas were built from -- the D random orders
    drawn and, for ``kernel_shap``, behind them the same orders reversed (``n - 1 - key``), -1 for an element that is no player;
    sample s of graph g -- the samples ``rep_ptr[g] .. rep_ptr[g + 1]`` -- keeps the players with ``keys[rows[s]] < thresh[s]``.
    ``invert`` is all zero: the drivers spell a complement as a prefix of the reversed order, which leaves the elements that
    are no player in place."""
    score: torch.Tensor
    phi0: torch.Tensor
    p_full: torch.Tensor
    p_empty: Optional[torch.Tensor]
    yhat: torch.Tensor
    r2: torch.Tensor
    status: torch.Tensor
    replicas: int
    forwards: int
    twin: Optional[torch.Tensor] = None
    keys: Optional[torch.Tensor] = None
    thresh: Optional[torch.Tensor] = None
    invert: Optional[torch.Tensor] = None
    rows: Optional[torch.Tensor] = None
    rep_ptr: Optional[torch.Tensor] = None


def _rand(shape, gen, dev):
    return torch.rand(*shape, generator=gen, device=gen.device).to(dev)


def _private_generator(generator):
    """The caller's generator (it advances), or a copy of the global CPU stream that leaves the global state as it was."""
    if generator is not None:
        return generator
    g = torch.Generator()
    g.set_state(torch.get_rng_state())
    return g


def _raise_on_status(status, ridge):
    counts = torch.bincount(status.long().clamp(0, 3), minlength=4).tolist()           # (the read-back of the statuses)
    if sum(counts[1:]):
        parts = ["%d graph%s: %s" % (c, "" if c == 1 else "s", STATUS[s]) for s, c in enumerate(counts) if s and c]
        hint = []
        if counts[1]:
            hint.append("raise samples (at least 2 (n - 1) for n players) or ridge (now %g)" % ridge)
        if counts[2]:
            hint.append("narrow the players with elements=")
        raise ValueError("the surrogate fit failed for " + "; ".join(parts) + (" -- " + ", ".join(hint) if hint else ""))


def _values(model, src, h, yhat, rg, rth, keys, rrow, use, chunk, out, slot, value_fn):
    """``_run_replicas`` (never inverted); with ``value_fn`` that callable in the model's place.  -> forwards."""
    if value_fn is None:
        return _run_replicas(model, src, h, yhat, rg, rth, keys, rrow, use, False, chunk, out, slot)
    forwards = 0
    for i in range(0, int(rg.numel()), chunk):
        g = rg[i:i + chunk]
        rb = coalition_batch(src, g, rth[i:i + chunk], keys, rep_row=rrow[i:i + chunk], use=use)
        _check_replicas(rb)
        out[slot[i:i + chunk]] = value_fn(rb, g).to(out.dtype)
        forwards += 1
    return forwards


def _surrogate(model, data, lay, mode, use, undirected, h, samples, elements, generator, ridge, chunk, keep, width, value_fn):
    """-> ``(Surrogate, players bool [M], _Players)`` over the edge columns in ``lay``'s graph order.  Called in eval mode under
    no_grad."""
    src = _grouped(data, lay)
    yhat, p_full, C = _whole(model, src, h)
    P = _Players(data, lay, src, use, undirected)
    dev, B, M = P.dev, P.B, P.M
    pl = torch.ones(M, dtype=torch.bool, device=dev) if P.rep is None else P.rep.clone()
    member = torch.ones(M, dtype=torch.bool, device=dev)
    if elements is not None:
        member = _members(elements, M, lay, use, P.twin)
        pl = pl & member
    n = P.count(pl)                                                      # players of every graph
    nmax = int(n.max()) if B else 0                                      # (a read-back: sizes the sampling tables)
    if samples is None:
        samples = max(2, 4 * nmax)
    samples = int(samples)
    if mode == 0 and (samples < 2 or samples % 2):
        raise ValueError("kernel_shap pairs every sample with its complement: samples must be even and >= 2")
    if samples < 1:
        raise ValueError("samples must be >= 1")
    D = samples // 2 if mode == 0 else samples
    gen = _private_generator(generator)
    keys = _draw_keys(P, member, D, gen)                                  # [D, M]
    nd = n.double()
    if mode == 0:                                                        # one size in [1, n - 1] per draw, p(k) ~ (n - 1) / (k (n - k))
        k = torch.arange(1, max(nmax, 2), device=dev).double().view(1, -1)
        wk = torch.where(k < nd.view(B, 1), (nd.view(B, 1) - 1) / (k * (nd.view(B, 1) - k)), torch.zeros_like(k))
        cdf = torch.cumsum(wk, 1) / wk.sum(1, keepdim=True).clamp(min=1e-300)
        u = _rand((D, B), gen, dev).double()
        size = 1 + (u.view(D, B, 1) >= cdf.view(1, B, -1)).sum(-1)
        size = torch.minimum(size, (n - 1).clamp(min=1).view(1, B))       # [D, B]
        cnt = torch.where(n >= 2, torch.full_like(n, samples), torch.zeros_like(n))   # one player (or none): nothing to sample
        # the complement of a prefix is a prefix of the REVERSED order: rows D .. 2 D - 1 hold n - 1 - key for the players and
        # -1 elsewhere, so an element that is no player is always present there too (an inverted compare would drop it)
        back = (n[P.gid].view(1, M) - 1 - keys.long()).to(torch.int32)
        keys = torch.cat([keys, torch.where(keys >= 0, back, keys)]).contiguous()
    else:                                                                # Binomial(n, keep) sizes
        u = _rand((D, B, max(nmax, 1)), gen, dev)
        live = torch.arange(max(nmax, 1), device=dev).view(1, 1, -1) < n.view(1, B, 1)
        size = ((u < keep) & live).sum(-1)                                # [D, B]
        cnt = torch.full_like(n, samples)
    rep_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(cnt, 0)])
    R = B * samples if mode == 1 else int(rep_ptr[-1])                   # (mode 0: a read-back)
    rg = torch.repeat_interleave(torch.arange(B, device=dev), cnt, output_size=R)
    j = torch.arange(R, device=dev) - rep_ptr[rg]                        # the sample's number inside its graph
    if mode == 0:                                                        # sample 2 q: the first k of order q; 2 q + 1: the other n - k
        q, comp = j // 2, j % 2 == 1
        rrow = torch.where(comp, q + D, q)
        rth = torch.where(comp, n[rg] - size[q, rg], size[q, rg]) if R else torch.zeros(0, dtype=torch.long, device=dev)
    else:
        rrow = j
        rth = size[rrow, rg] if R else torch.zeros(0, dtype=torch.long, device=dev)
    # the values: the fit's R replicas, then (mode 0) every graph's empty replica and, under value_fn, its full one
    t_lo = (n == P.nodes) if use == "nodes" else torch.zeros(B, dtype=torch.bool, device=dev)     # its empty replica has no node
    out = torch.full((R + 2 * B,), 1.0 / C, dtype=torch.float64, device=dev)
    run = ~(t_lo[rg] & (rth == 0))                                       # a replica without a node is not run: 1 / C
    slot = torch.arange(R, device=dev)
    forwards = 1 + _values(model, src, h, yhat, rg[run], rth[run], keys, rrow[run], use, chunk, out, slot[run], value_fn)
    replicas = int(run.sum())
    p_empty = None
    if mode == 0:
        ge = (~t_lo).nonzero().view(-1)
        zeros = torch.zeros_like(ge)
        forwards += _values(model, src, h, yhat, ge, zeros, keys, zeros, use, chunk, out, R + ge, value_fn)
        replicas += int(ge.numel())
        p_empty = out[R:R + B].clone()
        if value_fn is not None:                                         # the game's own full value: the control replica
            ga = torch.arange(B, device=dev)
            forwards += _values(model, src, h, yhat, ga, torch.zeros_like(ga), keys, torch.full_like(ga, -1), use, chunk, out,
                                R + B + ga, value_fn)
            replicas += B
            p_full = out[R + B:].clone()
    weight = None
    if mode == 1:
        frac = torch.where(n[rg] > 0, rth.double() / nd[rg].clamp(min=1), torch.ones(R, dtype=torch.float64, device=dev))
        weight = torch.exp(-((1.0 - frac) ** 2) / (width * width))
    pl_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(n, 0)])
    pl_elem = pl.nonzero().view(-1)
    phi, phi0, r2, status = surrogate_fit(keys, rep_ptr, rrow, rth, out[:R], pl_ptr, pl_elem, weight=weight,
                                          v_empty=p_empty, v_full=None if mode else p_full.double(), mode=mode, ridge=ridge)
    _raise_on_status(status, ridge)
    score = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
    score[pl_elem] = phi
    if P.twin is not None and M:                                         # the other column of a pair takes its representative's
        score = torch.where(P.rep | ~member, score, score[P.twin.clamp(min=0).long()])
    return Surrogate(score=score, phi0=phi0, p_full=p_full, p_empty=p_empty, yhat=yhat, r2=r2, status=status, replicas=replicas,
                     forwards=forwards, twin=P.twin, keys=keys, thresh=rth, invert=torch.zeros_like(rth), rows=rrow,
                     rep_ptr=rep_ptr), pl, P


def _check_args(use, undirected, head, samples, ridge, chunk):
    h, chunk = _check_driver_args(use, undirected, head, chunk)
    if samples is not None and (isinstance(samples, bool) or not isinstance(samples, int)):
        raise TypeError("samples must be an int or None")
    if not (float(ridge) >= 0.0 and float(ridge) != float("inf")):
        raise ValueError("ridge must be finite and >= 0")
    return h, chunk


def _caller_order(sg, lay, use):
    """``sg``'s per-column tensors back in the caller's column order."""
    if use == "edges" and lay.order is not None:
        score = torch.empty_like(sg.score)
        score[lay.order] = sg.score
        keys = torch.empty_like(sg.keys)
        keys[:, lay.order] = sg.keys
        sg.score, sg.keys = score, keys
        sg.twin = None if sg.twin is None else lay.caller_twin(sg.twin)
    return sg


def kernel_shap(model, data, *, samples=None, use: str = "edges", undirected=None, head: str = "o", elements=None, generator=None,
                ridge: float = 0.0, chunk: int = 512, value_fn=None) -> Surrogate:
    """KernelSHAP: Shapley values of every edge column (``use="edges"``), undirected edge (``undirected``) or node of ``data``
    from a fixed budget of ``samples`` replicas per graph, whatever its number of players.

    Players, ``elements``, ``undirected``, ``head``, the RNG discipline (a given ``generator`` advances and reproduces the
    scores bit for bit; without one the global states are left as they were), the caller's column order and what is left
    untouched (parameters, BatchNorm statistics, RNG states, ``model.training``) are exactly ``shapley``'s.

    Sampling is paired: each of ``samples / 2`` draws per graph is one random order of the players, one size ``k`` in
    ``[1, n - 1]`` with probability proportional to ``(n - 1) / (k (n - k))`` -- the Shapley kernel, so the samples enter the fit
    with weight 1 --, the replica that keeps the first ``k`` players of the order and the replica that keeps the others (built as the
    first ``n - k`` of the reversed order, a second key row, so that the elements that are no player stay in both).  One
    more replica per graph gives ``p_empty`` (with ``use="nodes"`` and every node a player it is *defined* as ``1 / C``, as in
    ``shapley``); ``p_full`` comes from the whole batch.  ``cal_surrogate_fit`` then solves, per graph, the least-squares problem
    under the constraint ``sum(score) = p_full - p_empty``, which therefore holds to rounding.  A graph with one player gets
    ``p_full - p_empty``; a graph with none has no score.

    ``samples=None`` means ``4 x`` the largest player count of the batch, made even.  A set and its complement span at most
    ``samples / 2 + 1`` directions of the n the fit needs, so ``samples >= 2 (n - 1)`` is NECESSARY for a graph of n players; with
    fewer the fit is rank-deficient.  Any graph that is not fitted raises ``ValueError`` naming the count per status:
    rank-deficient (raise ``samples``, or give ``ridge > 0``), more than 127 players on the GPU (narrow with ``elements=``), a
    non-finite value.  ``value_fn(replica_batch, rep_graph) -> [R]`` stands in for the model's forward on the replicas when
    given (a game with a known answer): the samples, ``p_empty`` and -- from one control replica per graph that keeps
    everything -- ``p_full`` are then all the callable's; ``yhat`` stays the model's.  Cost: ``samples + 1`` replicas per graph in chunks of at most ``chunk`` graphs."""
    h, chunk = _check_args(use, undirected, head, samples, ridge, chunk)
    with _eval_mode(model):
        lay = _Layout(data)
        sg = _surrogate(model, data, lay, 0, use, undirected, h, samples, elements, generator, float(ridge), chunk, None, None, value_fn)[0]
        sg = _caller_order(sg, lay, use)
    return sg


def _check_local(keep, width):
    if not 0.0 < float(keep) <= 1.0:
        raise ValueError("keep must be in (0, 1]")
    if not float(width) > 0.0:
        raise ValueError("width must be > 0")
    return float(keep), float(width)


def local_surrogate(model, data, *, samples=None, keep: float = 0.5, width: float = 0.25, use: str = "edges", undirected=None,
                    head: str = "o", elements=None, generator=None, ridge: float = 1e-3, chunk: int = 512, value_fn=None) -> Surrogate:
    """LIME's surrogate: a weighted linear model with a free intercept of ``p(ŷ)`` on the players' presence, around the whole
    graph.  Each of ``samples`` draws per graph (default ``4 x`` the largest player count) is one random order and one size
    ``k ~ Binomial(n, keep)``; the replica keeps the first k players of the order and enters the fit with the locality weight
    ``exp(-(1 - k / n)^2 / width^2)``.  ``ridge`` regularises the players' coefficients, not the intercept.  ``score`` holds the
    coefficients, ``phi0`` the intercept; ``r2``, the weighted coefficient of determination over the samples (<= 1), is the
    point: how additive the model is around this graph, which every other attribution method here assumes.  Everything else is
    ``kernel_shap``'s."""
    h, chunk = _check_args(use, undirected, head, samples, ridge, chunk)
    keep, width = _check_local(keep, width)
    with _eval_mode(model):
        lay = _Layout(data)
        sg = _surrogate(model, data, lay, 1, use, undirected, h, samples, elements, generator, float(ridge), chunk, keep, width, value_fn)[0]
        sg = _caller_order(sg, lay, use)
    return sg


def _method(method):
    if method not in ("shap", "lime"):
        raise ValueError('method must be "shap" or "lime"')
    return 0 if method == "shap" else 1


def _agreement(model, data, mode, use, undirected, h, samples, elements, generator, ridge, chunk, keep, width, ratio, k):
    """-> (the row ``_agree_sums`` + [players, sum of r2 where defined, graphs where it is], the ``Surrogate``, B)."""
    causal, lay = _causal_in_order(model, data, use)
    sg, pl, P = _surrogate(model, data, lay, mode, use, undirected, h, samples, elements, generator, ridge, chunk, keep, width, None)
    if P.twin is not None:
        causal = _symmetrised(causal, lay, P.twin, undirected)
    counts, met = rank_agreement(causal, sg.score.float(), P.seg, P.max_seg, sel=pl, ratio=ratio, k=k)
    ok = ~torch.isnan(sg.r2)
    tail = torch.stack([counts[:, 0].sum().double(), torch.where(ok, sg.r2, torch.zeros_like(sg.r2)).sum(), ok.sum().double()])
    return torch.cat([_agree_sums(met), tail]), sg, lay.B


def surrogate_agreement(model, data, *, method: str = "shap", samples=None, use: str = "edges", undirected=None, head: str = "o",
                        elements=None, generator=None, ridge=None, keep: float = 0.5, width: float = 0.25, ratio=None, k=None,
                        chunk: int = 512) -> dict:
    """Do ``model``'s causal scores rank the elements of ``data`` as the surrogate's coefficients do?  ``method``: ``"shap"``
    (``kernel_shap``) or ``"lime"`` (``local_surrogate``; ``ridge`` defaults to each one's own).  Returns ``rho``, ``tau``,
    ``jaccard`` and their ``_undefined`` counts as ``shapley_agreement`` does, ``r2`` (the mean over the graphs where it is
    defined), ``graphs``, ``elements``, ``replicas`` and ``forwards`` (the driver's plus one for the scores)."""
    _check_topk(ratio, k, "surrogate_agreement")
    mode = _method(method)
    ridge = (0.0 if mode == 0 else 1e-3) if ridge is None else ridge
    h, chunk = _check_args(use, undirected, head, samples, ridge, chunk)
    keep, width = _check_local(keep, width)
    with _eval_mode(model):
        row, sg, B = _agreement(model, data, mode, use, undirected, h, samples, elements, generator, float(ridge), chunk, keep, width,
                                ratio, k)
        row = row.tolist()
    res = _agree_report(row, B)
    res["r2"] = row[7] / row[8] if row[8] else float("nan")
    res["graphs"], res["elements"], res["replicas"], res["forwards"] = B, int(row[6]), sg.replicas, sg.forwards + 1
    return res


def eval_surrogate(model, loader, device, *, method: str = "shap", samples=None, use: str = "edges", undirected=None,
                   head: str = "o", generator=None, ridge=None, keep: float = 0.5, width: float = 0.25, ratio=None, k=None,
                   chunk: int = 512) -> dict:
    """``surrogate_agreement`` over a loader: the means over all its graphs, the sums kept on the device until one read-back at
    the end (besides the drivers' own)."""
    _check_topk(ratio, k, "eval_surrogate")
    mode = _method(method)
    ridge = (0.0 if mode == 0 else 1e-3) if ridge is None else ridge
    h, chunk = _check_args(use, undirected, head, samples, ridge, chunk)
    keep, width = _check_local(keep, width)
    sums = torch.zeros(9, dtype=torch.float64, device=device)
    graphs = replicas = forwards = 0
    with _eval_mode(model):
        for data in loader:
            row, sg, B = _agreement(model, data.to(device), mode, use, undirected, h, samples, None, generator, float(ridge), chunk,
                                    keep, width, ratio, k)
            sums += row
            graphs, replicas, forwards = graphs + B, replicas + sg.replicas, forwards + sg.forwards + 1
    row = sums.tolist()
    res = _agree_report(row, graphs)
    res["r2"] = row[7] / row[8] if row[8] else float("nan")
    res["graphs"], res["elements"], res["replicas"], res["forwards"] = graphs, int(row[6]), replicas, forwards
    return res
