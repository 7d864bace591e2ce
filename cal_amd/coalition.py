"""Shapley attributions and perturbation curves: replicas that keep a nested subset of a graph's elements.

Leave-one-out occlusion (``cal_amd.occlude``) has a blind spot: when two elements are redundant -- two edges of a cycle or house
motif -- removing either one alone changes nothing, and both score about 0 like an edge that truly does not matter.  The Shapley
value, an element's marginal contribution averaged over random orders in which the graph is assembled, credits redundant elements
jointly, and its scores sum to ``p(full) - p(empty)``.  Sampling it needs replicas that keep an arbitrary nested subset of a
graph's elements; the same primitive gives deletion and insertion curves on a fine grid in a handful of forwards.

* ``coalition_batch(data, rep_graph, rep_thresh, key, rep_row=..., use=..., invert=...)`` -> ``Batch``: replica r is graph
  ``rep_graph[r]`` of ``data`` with the elements whose integer key is below (``invert``: not below) ``rep_thresh[r]``
  (``cal_coalition_count`` / ``cal_coalition_write``: two launches and one read-back of the totals on the GPU, libcalhost for
  CPU tensors), with the layout facts that keep the engine on its per-graph route.
* ``shapley(model, data, use=..., undirected=..., perms=...)`` (also ``model.shapley``) -> ``Shapley``: permutation-sampled
  Shapley values of every edge column, undirected edge or node.
* ``perturbation_curve(model, data, ratios=..., order=...)`` (also ``model.perturbation_curve``) /
  ``eval_perturbation_curve(model, loader, device, ...)``: ``p(ŷ)`` with the top ``ceil(r n)`` elements of a ranking kept
  (insertion) and removed (deletion) at every ratio r, and the areas under the two curves.
* ``shapley_agreement(model, data, ...)``: the causal attention against the Shapley scores, through ``rank_agreement``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .explain import _eval_mode, _Layout, _scores
from .occlude import rank_agreement
from .plan import _p
from .replica import (_agree_report, _agree_sums, _built_batch, _caller_columns, _causal_in_order, _check_driver_args, _check_topk,
                      _check_use, _feature_width, _grouped, _members, _node_map_rows, _p_at, _pairs, _Players, _rebatch,
                      _replica_log_probs, _Source, _symmetrised, _whole)

__all__ = ["Shapley", "coalition_batch", "shapley", "perturbation_curve", "eval_perturbation_curve", "shapley_agreement"]


def coalition_batch(data, rep_graph, rep_thresh, key, *, rep_row=None, use: str = "edges", invert: bool = False):
    """``R`` replicas of graphs of ``data``, each restricted to a subset of its elements, as a ``cal_amd.data.Batch`` the engine
    can run.

    ``key`` is an integer tensor [K, M] (or [M]: one row) with one entry per edge column (``use="edges"``, M = E) or per node
    (``"nodes"``, M = N).  Replica r is graph ``rep_graph[r]`` (int64 [R]; an id outside the batch gives a replica with no node,
    counted in ``empty_graphs``); element e of it stays iff ``rep_row[r]`` (int64 [R]; zeros by default when ``key`` has one row)
    is outside ``[0, K)`` -- the control replica, everything stays -- or ``key[rep_row[r], e] < rep_thresh[r]``, with
    ``invert=True`` ``key[rep_row[r], e] >= rep_thresh[r]``.  A plain integer compare: ties, negative keys (elements that are
    always present) and keys that are no permutation all have a defined result, and the replicas of one key row at growing
    thresholds are nested.  ``use="edges"``: all nodes stay, the columns that stay keep their order.  ``use="nodes"``: the nodes
    that stay are renumbered densely in their order and their rows copied; a column stays iff both endpoints stay.  A source
    column that leaves its graph's node range is dropped.  A graph may appear in any number of replicas.

    The result carries ``x`` / ``feat`` as ``data`` does (row copies), ``edge_index``, ``batch``, ``ptr``, ``edge_ptr``,
    ``num_graphs = R``, ``max_nodes``, ``max_edges``, ``no_self_loops`` (inherited), no tiles, ``y = data.y[rep_graph]`` (``None``
    when ``data`` has none or a graph id is outside the batch), ``node_src`` / ``edge_src`` (int64: the source element of every
    new node / column) and the host int ``empty_graphs``.

    CUDA tensors: ``cal_coalition_count`` and ``cal_coalition_write`` on the current stream with one read-back of the totals
    between them; CPU tensors: libcalhost.  Inputs other than ``Batch`` objects get their layout derived as in ``occlude_batch``;
    edge columns that are not grouped by graph are put in stable graph order first, ``key`` is taken in the caller's column
    numbering and ``edge_src`` is mapped back to it."""
    _check_use(use)
    mode = 0 if use == "edges" else 1
    S = _Source(data)
    dev, F = S.dev, _feature_width(S, "coalition_batch")
    if rep_graph is None or rep_thresh is None:
        raise TypeError("rep_graph and rep_thresh are required")
    M = S.E if mode == 0 else S.N
    if not torch.is_tensor(key) or key.dtype.is_floating_point or key.dtype == torch.bool:
        raise TypeError("key must be an integer tensor")
    if key.dim() not in (1, 2) or int(key.size(-1)) != M:
        raise ValueError("key must be [K, M] or [M] with one entry per %s (M = %d)" % ("edge column" if mode == 0 else "node", M))
    key = key.view(1, M) if key.dim() == 1 else key
    K = int(key.size(0))
    rg, rth = _pairs(rep_graph, 0, dev, "rep_graph"), _pairs(rep_thresh, 0, dev, "rep_thresh")
    R = int(rg.numel())
    if rep_row is None:
        if K != 1:
            raise ValueError("rep_row is required when key has %d rows" % K)
        rrow = torch.zeros(R, dtype=torch.long, device=dev)
    else:
        rrow = _pairs(rep_row, 0, dev, "rep_row")
    if int(rth.numel()) != R or int(rrow.numel()) != R:
        raise ValueError("rep_graph, rep_row and rep_thresh must have one entry per replica each (got %d, %d and %d)"
                         % (R, rrow.numel(), rth.numel()))
    key = key.to(device=dev, dtype=torch.int32)
    if S.order is not None and mode == 0 and S.E:          # the caller's column numbering -> graph order
        key = key[:, S.order]
    key = key.contiguous()
    mx = _node_map_rows(S, data) if mode == 1 else 0
    inputs = S.args() + [_p(key) if K and M else None, K, _p(rg) if R else None, _p(rrow) if R else None, _p(rth) if R else None, R,
                         mode, int(bool(invert)), mx]
    built = _rebatch("cal_coalition", (S.E, R, mx, mode), inputs, R, 5, (S,), F, lambda: (rg < 0) | (rg >= S.B))
    return _built_batch(S, built, rg, S.no_self_loops, _caller_columns(S, built.edge_src, built.tot[1]))


# ---- the pieces the drivers share ---------------------------------------------------------------------------------------------
def _run_replicas(model, src, h, yhat, rg, rth, key, rrow, use, invert, chunk, out, slot):
    """The replicas ``(rg, rrow, rth)`` (one entry each per replica; ``rrow`` may be ``None``) in chunks of at most ``chunk``, one
    ``coalition_batch`` and one forward each: ``out[slot[r]] = p(ŷ)`` of replica r (``out`` 1-D).  -> the forwards it took."""
    n, forwards = int(rg.numel()), 0
    for i in range(0, n, chunk):
        g = rg[i:i + chunk]
        rb = coalition_batch(src, g, rth[i:i + chunk], key, rep_row=None if rrow is None else rrow[i:i + chunk], use=use,
                             invert=invert)
        out[slot[i:i + chunk]] = _p_at(_replica_log_probs(model, rb, h), yhat[g]).to(out.dtype)
        forwards += 1
    return forwards


def _shifted_mean(m):
    """Mean over dim 0 taken about row 0, so that equal rows give exactly that row."""
    return m[0] + (m - m[0]).mean(0)


# ---- Shapley values -----------------------------------------------------------------------------------------------------------
@dataclass
class Shapley:
    """Permutation-sampled Shapley values of a batch.  ``score`` fp64 [E] (``use="edges"``) or [N] (``"nodes"``): the mean over the
    orders of the element's marginal contribution to ``p(ŷ_g)`` at the chosen head; NaN for an element that is no player (outside
    ``elements``).  ``stderr`` fp64: the standard deviation over the orders / sqrt(S), NaN for one order.  ``p_full`` [B] and
    ``yhat`` int64 [B]: the whole graph's probability of its own argmax and that argmax; ``p_empty`` fp64 [B]: the probability
    with no player present (``1 / C`` where that graph would have no node), so that per graph the scores of the players sum to
    ``p_full - p_empty``.  ``replicas``: graphs run besides the whole batch, in ``forwards`` forwards (the whole batch's
    included).  ``twin``: the reverse-column map int32 [E] when ``undirected`` built one, else ``None``.  ``keys`` int32 [S, M]:
    every order as the builder took it -- a player's 0-based position among its graph's players, -1 for an element that is
    always present."""
    score: torch.Tensor
    stderr: torch.Tensor
    p_full: torch.Tensor
    p_empty: torch.Tensor
    yhat: torch.Tensor
    replicas: int
    forwards: int
    twin: Optional[torch.Tensor] = None
    keys: Optional[torch.Tensor] = None


def _draw_keys(P, member, S, generator):
    """``S`` random orders of the players: int32 [S, M], a player's position among its graph's players (both columns of an
    undirected edge the same), -1 elsewhere."""
    state = None if generator is not None else torch.get_rng_state()
    try:
        gdev = generator.device if generator is not None else "cpu"
        r = torch.rand(S, P.M, generator=generator, device=gdev)
    finally:
        if state is not None:
            torch.set_rng_state(state)
    r = r.to(P.dev)
    if P.twin is not None:                                               # the other column of a pair takes its representative's
        r = torch.where(P.rep, r, r[:, P.twin.clamp(min=0).long()])
    r = torch.where(member, r, torch.full_like(r, float("nan")))          # NaN ranks below every number
    minus = torch.full((P.M,), -1, dtype=torch.int32, device=P.dev)
    return torch.stack([torch.where(member, P.rank(r[s]), minus) for s in range(S)]) if S else minus.view(0, P.M)


def _shapley(model, data, lay, use, undirected, h, perms, elements, generator, chunk):
    """-> ``(Shapley, players bool [M], _Players)`` over the edge columns in ``lay``'s graph order (``score``, ``stderr``, ``twin``
    and ``keys`` index that order).  ``players`` marks one representative per player.  Called in eval mode under no_grad."""
    src = _grouped(data, lay)
    yhat, p_full, C = _whole(model, src, h)
    P = _Players(data, lay, src, use, undirected)
    dev, B, M = P.dev, P.B, P.M
    pl = torch.ones(M, dtype=torch.bool, device=dev) if P.rep is None else P.rep.clone()
    member = torch.ones(M, dtype=torch.bool, device=dev)
    if elements is not None:
        member = _members(elements, M, lay, use, P.twin)
        pl = pl & member
    if torch.is_tensor(perms):
        if perms.dim() != 2 or int(perms.size(1)) != M or int(perms.size(0)) < 1:
            raise ValueError("perms as a tensor must be int32 [S, M] with S >= 1 and M = %d elements" % M)
        if perms.dtype != torch.int32:
            raise TypeError("perms as a tensor must be int32 [S, M]")
        keys = perms.to(dev)
        if use == "edges" and lay.order is not None:
            keys = keys[:, lay.order]
        keys = keys.contiguous()
    else:
        keys = _draw_keys(P, member, int(perms), generator)
    S = int(keys.size(0))
    n = P.count(pl)                                                      # players of every graph
    t_lo = ((n == P.nodes) if use == "nodes" else torch.zeros_like(n, dtype=torch.bool)).long()     # the empty replica is not run
    cnt = (n - t_lo).clamp(min=0)
    off = torch.cumsum(n + 1, 0) - (n + 1)                                # graph g's values v(g, s, 0 .. n_g) start here
    T1, W = torch.stack([cnt.sum(), (n + 1).sum()]).tolist()             # (a read-back: the number of replicas)
    start = torch.cumsum(cnt, 0) - cnt
    rg1 = torch.repeat_interleave(torch.arange(B, device=dev), cnt, output_size=T1)
    th1 = torch.arange(T1, device=dev) - start[rg1] + t_lo[rg1]
    v = torch.full((S, W), float("nan"), dtype=torch.float64, device=dev)
    if B:
        v[:, off] = torch.where(t_lo.bool(), torch.full_like(v[0, off], 1.0 / C), v[0, off])
        v[:, off + n] = p_full.double()
    total = S * T1
    rg, rth = rg1.repeat(S), th1.repeat(S)                               # the replicas of all orders, order by order
    rrow = torch.repeat_interleave(torch.arange(S, device=dev), T1, output_size=total)
    forwards = 1 + _run_replicas(model, src, h, yhat, rg, rth, keys, rrow, use, False, chunk, v.view(-1), rrow * W + off[rg] + rth)
    score = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
    stderr = score.clone()
    if M and W:
        idx = off[P.gid].view(1, M) + keys.long()
        m = v.gather(1, (idx + 1).clamp(0, W - 1)) - v.gather(1, idx.clamp(0, W - 1))                # [S, M] marginals
        d = m - m[0]
        mean = d.mean(0)
        score = torch.where(member, m[0] + mean, score)
        if S > 1:
            stderr = torch.where(member, (((d - mean) ** 2).sum(0) / (S - 1)).sqrt() / S ** 0.5, stderr)
    p_empty = _shifted_mean(v[:, off]) if B else p_full.double()
    return Shapley(score=score, stderr=stderr, p_full=p_full, p_empty=p_empty, yhat=yhat, replicas=total, forwards=forwards,
                   twin=P.twin, keys=keys), pl, P


def _check_shapley_args(use, undirected, head, perms, chunk):
    h, chunk = _check_driver_args(use, undirected, head, chunk)
    if not torch.is_tensor(perms):
        if isinstance(perms, bool) or not isinstance(perms, int):
            raise TypeError("perms must be an int >= 1 or an int32 [S, M] tensor of keys")
        if perms < 1:
            raise ValueError("perms must be >= 1")
    return h, chunk


def _caller_order(sh, lay, use):
    """``sh``'s per-column tensors back in the caller's column order."""
    if use == "edges" and lay.order is not None:
        for name in ("score", "stderr"):
            t = torch.empty_like(getattr(sh, name))
            t[lay.order] = getattr(sh, name)
            setattr(sh, name, t)
        keys = torch.empty_like(sh.keys)
        keys[:, lay.order] = sh.keys
        sh.keys = keys
        sh.twin = None if sh.twin is None else lay.caller_twin(sh.twin)
    return sh


def shapley(model, data, *, use: str = "edges", undirected=None, head: str = "o", perms=8, elements=None, generator=None,
            chunk: int = 512) -> Shapley:
    """Permutation-sampled Shapley values of every edge column (``use="edges"``) or node (``"nodes"``) of ``data``.

    One eval forward of the whole batch (untiled, the route the replicas take) gives ŷ_g, the argmax of ``head`` (``"c"``,
    ``"o"`` or ``"co"``), and ``p_full``.  The players of graph g are its edge columns; with ``undirected`` = ``"mean"`` /
    ``"max"`` / ``"min"`` (all three the same here: the names ``explain`` takes) a pair of twin columns is one player; with
    ``use="nodes"`` its nodes.  ``elements``: a bool mask [E] / [N] of the players (an undirected edge when either of its columns
    is named); every other element is always present and scores NaN.

    ``perms = S`` draws S random orders per graph (``torch.rand(..., generator=generator)`` ranked per graph by
    ``rank_segments`` / ``rank_segment_pairs``; a given ``generator`` advances and the global RNG states are untouched, without
    one the global torch state is restored).  ``perms`` may instead be an int32 [S, M] tensor of keys -- per graph the players'
    positions 0 .. n_g - 1, both columns of an undirected edge the same, -1 for every other element -- which is trusted and not
    read back.  For order s and graph g with n_g players, replica t in [0, n_g) keeps the players with key < t
    (``coalition_batch``), ``v(g, s, t)`` is the head's probability of ŷ_g on it and ``v(g, s, n_g) = p_full[g]`` (not run).
    The marginal of the player with key p is ``v(g, s, p + 1) - v(g, s, p)``; ``score`` is its mean over the orders and
    ``stderr`` the standard deviation over the orders / sqrt(S), both formed in fp64 on the device.  Both columns of an
    undirected edge receive the score.  Per graph the scores of the players sum to ``p_full - p_empty``.

    The empty graph: with ``use="nodes"`` and every node of a graph a player, replica t = 0 would have no node; it is not run
    and its value is *defined* as ``1 / C``, the uniform prediction over the C classes.  Any other replica without a node raises
    ``ValueError`` naming the count.

    Cost: S x players replicas packed, all orders together, into chunks of at most ``chunk`` graphs (512 is the bound of the
    engine's one-launch readout), each one builder call (two launches and a read-back) and one forward -- 12 544 players, 25
    forwards per order, for the headline batch of 128 SPMotif graphs undirected.  CPU-resident models go through libcalhost
    and the operator-level ``model(data)``.  Like ``explain``, it runs in eval mode under ``no_grad`` and leaves parameters,
    optimizer state, the engine's step counter, BatchNorm statistics, the RNG states and ``model.training`` as they were."""
    h, chunk = _check_shapley_args(use, undirected, head, perms, chunk)
    with _eval_mode(model):
        lay = _Layout(data)
        sh = _caller_order(_shapley(model, data, lay, use, undirected, h, perms, elements, generator, chunk)[0], lay, use)
    return sh


# ---- deletion / insertion curves ----------------------------------------------------------------------------------------------
def _check_ratios(ratios):
    ratios = [float(r) for r in ratios]
    if not ratios:
        raise ValueError("ratios must name at least one ratio")
    for r in ratios:
        if not r >= 0.0:
            raise ValueError("ratios must be >= 0")
    return ratios


_DEFAULT_RATIOS = tuple(i / 10 for i in range(11))


def _curve(model, data, use, undirected, h, ratios, order, chunk):
    """-> ``(insertion [B, T], deletion [B, T], p_full [B], ŷ [B], replicas, forwards)`` of one batch.  Called in eval mode
    under no_grad."""
    lay = _Layout(data)
    forwards = 0
    if order is None:                                                    # the causal attention, as explain ranks it
        edge, node = _scores(model, data)
        order = (edge if use == "edges" else node).clone()
        forwards = 1
    src = _grouped(data, lay)
    yhat, p_full, C = _whole(model, src, h)
    P = _Players(data, lay, src, use, undirected)
    dev, B, M = P.dev, P.B, P.M
    if not torch.is_tensor(order) or order.dim() != 1 or int(order.numel()) != M:
        raise ValueError("order must be a score vector with one entry per %s (%d)" % ("edge column" if use == "edges" else "node", M))
    order = order.to(device=dev, dtype=torch.float32)
    if use == "edges" and lay.order is not None:
        order = order[lay.order]
    key = P.rank(order).view(1, M)
    n = P.count(torch.ones(M, dtype=torch.bool, device=dev) if P.rep is None else P.rep)
    T = len(ratios)
    rt = torch.tensor(ratios, dtype=torch.float64, device=dev)
    kk = torch.minimum(torch.ceil(rt.view(T, 1) * n.double().view(1, B)).long(), n.view(1, B))      # [T, B]: ceil(r n_g)
    gsel = torch.arange(B, device=dev).repeat(T)
    curves, replicas = [], 0
    for invert in (False, True):
        out = torch.full((T * B,), 1.0 / C, dtype=torch.float32, device=dev)
        th = kk.view(-1)
        if use == "nodes":                                               # a replica without a node is not run: 1 / C
            kept = (n.view(1, B) - kk).view(-1) if invert else th
            idx = (kept > 0).nonzero().view(-1)                          # (a read-back: the number of replicas)
        else:
            idx = torch.arange(T * B, device=dev)
        forwards += _run_replicas(model, src, h, yhat, gsel[idx], th[idx], key, None, use, invert, chunk, out, idx)
        curves.append(out.view(T, B).t().contiguous())
        replicas += int(idx.numel())
    return curves[0], curves[1], p_full, yhat, replicas, forwards + 1


def _auc(y, ratios):
    """Trapezoid of ``y`` [B, T] over ``ratios`` in fp64 -> [B]."""
    x = torch.tensor(ratios, dtype=torch.float64, device=y.device)
    y = y.double()
    return ((y[:, 1:] + y[:, :-1]) * 0.5 * (x[1:] - x[:-1])).sum(1)


def _check_curve_args(use, undirected, head, ratios, chunk):
    h, chunk = _check_driver_args(use, undirected, head, chunk)
    return h, chunk, _check_ratios(ratios)


def perturbation_curve(model, data, *, use: str = "edges", undirected=None, head: str = "o", ratios=_DEFAULT_RATIOS, order=None,
                       chunk: int = 512) -> dict:
    """Insertion and deletion curves of ``data`` under a ranking of its edges (``use="edges"``; ``undirected`` as in ``explain``:
    undirected edges) or nodes.

    ``order`` is a score vector [E] / [N] -- a ``Shapley.score``, an ``Occlusion.score``, anything; high first, NaN last, as
    ``explain`` ranks -- and by default the causal attention exactly as ``explain`` ranks it, symmetrised by ``undirected``.
    One eval forward of the whole batch gives ŷ_g (the argmax of ``head``) and ``p_full``.  Per graph with n_g elements and
    ratio r, ``k = min(n_g, ceil(r n_g))``; the insertion replica keeps the top k, the deletion replica removes them.  All
    2 T B replicas go through ``coalition_batch`` in chunks of at most ``chunk`` graphs, one forward each.  With ``use="nodes"``
    a replica without a node is not run: its value is *defined* as ``1 / C``, the uniform prediction.

    Returns ``insertion`` / ``deletion`` float32 [B, T] (``p(ŷ_g)``), ``insertion_mean`` / ``deletion_mean`` fp64 [T] (over the
    batch), ``auc_insertion`` / ``auc_deletion`` fp64 [B] (the trapezoid over ``ratios``) with ``auc_insertion_mean`` /
    ``auc_deletion_mean``, ``p_full`` [B], ``yhat`` int64 [B], ``ratios`` and the host ints ``replicas`` and ``forwards`` (the whole batch's
    included, and the scores' when ``order`` is not given).  The tensors stay on ``data``'s device.  It leaves the model as
    ``explain`` does."""
    h, chunk, ratios = _check_curve_args(use, undirected, head, ratios, chunk)
    with _eval_mode(model):
        ins, dele, p_full, yhat, replicas, forwards = _curve(model, data, use, undirected, h, ratios, order, chunk)
        ai, ad = _auc(ins, ratios), _auc(dele, ratios)
        res = {"insertion": ins, "deletion": dele, "insertion_mean": ins.double().mean(0), "deletion_mean": dele.double().mean(0),
               "auc_insertion": ai, "auc_deletion": ad, "auc_insertion_mean": ai.mean(), "auc_deletion_mean": ad.mean(),
               "p_full": p_full, "yhat": yhat, "ratios": ratios, "replicas": replicas, "forwards": forwards}
    return res


def eval_perturbation_curve(model, loader, device, *, use: str = "edges", undirected=None, head: str = "o",
                            ratios=_DEFAULT_RATIOS, chunk: int = 512) -> dict:
    """``perturbation_curve`` under the causal attention over a loader: ``insertion_mean`` / ``deletion_mean`` (lists, one entry
    per ratio), ``auc_insertion_mean`` / ``auc_deletion_mean``, ``p_full_mean``, the means taken over all graphs of the loader,
    and ``graphs``, ``ratios``, ``replicas``, ``forwards``.  The sums stay on the device until one read-back at the end (besides
    the replica builder's)."""
    h, chunk, ratios = _check_curve_args(use, undirected, head, ratios, chunk)
    T = len(ratios)
    sums = torch.zeros(2 * T + 4, dtype=torch.float64, device=device)
    replicas = forwards = 0
    with _eval_mode(model):
        for data in loader:
            ins, dele, p_full, _, r, f = _curve(model, data.to(device), use, undirected, h, ratios, None, chunk)
            tail = torch.stack([_auc(ins, ratios).sum(), _auc(dele, ratios).sum(), p_full.double().sum(),
                                torch.as_tensor(float(p_full.numel()), dtype=torch.float64, device=p_full.device)])
            sums += torch.cat([ins.double().sum(0), dele.double().sum(0), tail])
            replicas, forwards = replicas + r, forwards + f
    row = sums.tolist()
    n = row[-1]
    mean = lambda v: v / n if n else float("nan")
    return {"insertion_mean": [mean(v) for v in row[:T]], "deletion_mean": [mean(v) for v in row[T:2 * T]],
            "auc_insertion_mean": mean(row[2 * T]), "auc_deletion_mean": mean(row[2 * T + 1]), "p_full_mean": mean(row[2 * T + 2]),
            "graphs": int(n), "ratios": ratios, "replicas": replicas, "forwards": forwards}


# ---- causal attention against the Shapley scores ------------------------------------------------------------------------------
def shapley_agreement(model, data, *, use: str = "edges", undirected=None, head: str = "o", perms=8, elements=None,
                      generator=None, ratio=None, k=None, chunk: int = 512) -> dict:
    """Do ``model``'s causal scores rank the elements of ``data`` as their Shapley values do?

    The causal score (column 1 of the soft masks; for edges symmetrised by ``undirected`` exactly as ``explain`` does it) is
    compared per graph with ``shapley(model, data, ...)``'s score, cast to float32, over the players (with ``undirected`` one
    representative per undirected edge) by one ``rank_agreement`` call.  Returns ``rho``, ``tau``, ``jaccard`` (the mean Spearman
    rho, Kendall tau-b and top-k Jaccard overlap -- ``ratio`` / ``k`` as ``explain`` takes them, counted over the players -- over
    the graphs where each is defined), ``rho_undefined``, ``tau_undefined``, ``jaccard_undefined`` (the graphs where it is not),
    ``graphs``, ``elements`` (players compared), ``replicas`` and ``forwards`` (``shapley``'s plus one for the scores): the
    shape of ``faithfulness``, which is what to compare it with.  It leaves the model as ``shapley`` does."""
    _check_topk(ratio, k, "shapley_agreement")
    h, chunk = _check_shapley_args(use, undirected, head, perms, chunk)
    with _eval_mode(model):
        causal, lay = _causal_in_order(model, data, use)
        sh, pl, P = _shapley(model, data, lay, use, undirected, h, perms, elements, generator, chunk)
        if P.twin is not None:
            causal = _symmetrised(causal, lay, P.twin, undirected)
        counts, met = rank_agreement(causal, sh.score.float(), P.seg, P.max_seg, sel=pl, ratio=ratio, k=k)
        row = torch.cat([_agree_sums(met), counts[:, 0].sum().double().view(1)]).tolist()
    res = _agree_report(row, lay.B)
    res["graphs"], res["elements"], res["replicas"], res["forwards"] = lay.B, int(row[6]), sh.replicas, sh.forwards + 1
    return res
