"""Counterfactual explanations: the smallest set of edges (or nodes) whose removal changes the prediction.

CAL claims that the causal subgraph *determines* the label.  The most direct test of that claim is the counterfactual one:
removing the causal part should flip the prediction with few edges, removing trivial edges should not (CF-GNNExplainer, CF²,
RCExplainer).  ``occlude_batch`` removes exactly one element and ``coalition_batch`` keeps ``key < thresh`` -- nested subsets
only; a search over arbitrary subsets needs replicas addressed by a bitset over their own graph's elements, and a device step
that picks the next beam:

* ``subset_batch(data, rep_graph, bits, rep_row=..., rep_flip=..., use=..., twin=...)`` -> ``Batch``: replica r is graph
  ``rep_graph[r]`` of ``data`` restricted to the elements whose bit is set in row ``rep_row[r]`` of ``bits``, after the local
  index ``rep_flip[r]`` (and its twin column) has been toggled (``cal_subset_count`` / ``cal_subset_write``: two launches and
  one read-back of the totals on the GPU, libcalhost for CPU tensors).  ``pack_bits`` / ``unpack_bits`` go between masks over
  the batch's elements and one bitset row per graph.
* ``beam_step(...)``: ``cal_beam_step``, one launch and no read-back -- the counterfactual of every graph that has one among
  its candidates, else its ``beam`` best distinct children.
* ``counterfactual(model, data, use=..., undirected=..., beam=...)`` (also ``model.counterfactual``) -> ``Counterfactual``:
  the beam search; ``beam=1`` is the greedy search.
* ``ranking_flip(model, data, order=...)`` (also ``model.ranking_flip``): the smallest prefix of a ranking whose removal flips
  the prediction -- the causal attention by default.
* ``counterfactual_report(model, data, ...)`` / ``eval_counterfactual(model, loader, device, ...)``: flip rate and mean size of
  the searched set against the attention ranking and a seeded random ranking, and how much of the set lies in a ground truth.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .explain import _eval_mode, _keep8, _Layout, _scores
from .plan import _p, _stream
from .replica import (_built_batch, _caller_columns, _check_driver_args, _check_use, _feature_width, _grouped, _members, _p_at,
                      _node_map_rows, _pairs, _Players, _rebatch, _replica_log_probs, _representatives, _Source, _twin_in_order,
                      _whole)

__all__ = ["Counterfactual", "subset_batch", "pack_bits", "unpack_bits", "beam_step", "counterfactual", "ranking_flip",
           "counterfactual_report", "eval_counterfactual"]

BEAM_MAX = 16          # rules.hpp kBeamMax
BEAM_WORDS = 64        # rules.hpp kBeamWords: a state of the search covers 2048 local elements


# ---- bitsets ------------------------------------------------------------------------------------------------------------------
def _words(bits, what="bits"):
    """``bits`` as an int32 tensor of the same 32-bit patterns (the libraries read them as uint32)."""
    if not torch.is_tensor(bits) or bits.dtype not in (torch.int32, torch.uint32):
        raise TypeError("%s must be an int32 or uint32 tensor of 32-bit words" % what)
    return bits if bits.dtype == torch.int32 else bits.view(torch.int32)


def _local(seg_ptr, M: int):
    """-> (graph id, local index) int64 [M] of the elements of the segments ``seg_ptr``."""
    seg = seg_ptr.to(torch.long)
    B = int(seg.numel()) - 1
    gid = torch.repeat_interleave(torch.arange(B, device=seg.device), seg[1:] - seg[:-1], output_size=M)
    return gid, torch.arange(M, device=seg.device) - seg[gid]


def pack_bits(mask, seg_ptr, max_seg: int):
    """A bool mask [M] over the elements of the segments ``seg_ptr`` [B + 1] (edge columns grouped by graph, or nodes) as one
    bitset row per graph: int32 [B, W], ``W = max(1, ceil(max_seg / 32))``, bit ``j & 31`` of word ``j >> 5`` of row g is local
    element j of graph g -- the ``bits`` of ``subset_batch`` with ``rep_row = rep_graph``.  Plain torch, no read-back."""
    M = int(mask.numel())
    B, W = int(seg_ptr.numel()) - 1, max(1, -(-int(max_seg) // 32))
    gid, loc = _local(seg_ptr, M)
    val = mask.to(device=gid.device, dtype=torch.long) << (loc & 31)
    out = torch.zeros(B * W, dtype=torch.long, device=gid.device).index_add_(0, gid * W + (loc >> 5).clamp(max=W - 1),
                                                                            torch.where(loc < 32 * W, val, torch.zeros_like(val)))
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32).view(B, W)


def unpack_bits(bits, seg_ptr, M: int):
    """The inverse of ``pack_bits``: bool [M] from one bitset row per graph, int32 / uint32 [B, W]; a local index >= 32 W is
    absent."""
    bits = _words(bits)
    W = int(bits.size(-1))
    gid, loc = _local(seg_ptr, int(M))
    if W == 0:
        return torch.zeros(int(M), dtype=torch.bool, device=gid.device)
    word = bits.reshape(-1)[gid * W + (loc >> 5).clamp(max=W - 1)].long()
    return (((word >> (loc & 31)) & 1) == 1) & (loc < 32 * W)


# ---- the builder --------------------------------------------------------------------------------------------------------------
def subset_batch(data, rep_graph, bits, *, rep_row=None, rep_flip=None, use: str = "edges", twin=None):
    """``R`` replicas of graphs of ``data``, each restricted to an arbitrary subset of its elements, as a ``cal_amd.data.Batch``
    the engine can run.

    ``bits`` is int32 / uint32 [K, W] (or [W]: one row; or ``None``: K = 0): bit ``j & 31`` of word ``j >> 5`` of a row is LOCAL
    element j of the replica's own graph -- its j-th edge column (``use="edges"``) or node (``"nodes"``); a local index
    ``>= 32 W`` is absent.  Replica r is graph ``rep_graph[r]`` (int64 [R]; an id outside the batch gives a replica with no node,
    counted in ``empty_graphs``); its base set is row ``rep_row[r]`` (int64 [R]; a row outside ``[0, K)`` means every element is
    present: the control replica, the default when ``bits`` is ``None``; zeros by default when ``bits`` has one row).  Then
    ``rep_flip[r]`` (int64 [R], a local index; by default -1) is toggled: a set bit is cleared, a cleared one set again.  With
    ``use="edges"`` and ``twin`` (int32 [E], as ``edge_twins`` gives it) the twin column is toggled too when it lies in the same
    graph; a self loop is its own twin.  A flip outside the graph's elements toggles nothing.  ``use="edges"``: all nodes stay,
    the columns whose bit is set stay in order.  ``use="nodes"``: the nodes that stay are renumbered densely in their order and
    their rows copied; a column stays iff both endpoints stay.  A source column that leaves its graph's node range is dropped.
    A row of ``bits`` serves any number of replicas: a replica costs three int64, not a key row over the whole batch.

    The result carries what ``coalition_batch``'s does.  CUDA tensors: ``cal_subset_count`` and ``cal_subset_write`` on the
    current stream with one read-back of the totals between them; CPU tensors: libcalhost.  Inputs other than ``Batch`` objects
    get their layout derived as in ``occlude_batch``; edge columns that are not grouped by graph are put in stable graph order
    first -- which leaves a column's local index inside its graph as the caller counts it, so ``bits`` and ``rep_flip`` are
    taken in the caller's local numbering -- ``twin`` is mapped to that order and ``edge_src`` back to the caller's."""
    _check_use(use)
    mode = 0 if use == "edges" else 1
    S = _Source(data)
    dev, F = S.dev, _feature_width(S, "subset_batch")
    if rep_graph is None:
        raise TypeError("rep_graph is required")
    rg = _pairs(rep_graph, 0, dev, "rep_graph")
    R = int(rg.numel())
    K = W = 0
    if bits is not None:
        bits = _words(bits)
        if bits.dim() not in (1, 2):
            raise ValueError("bits must be [K, W] or [W]")
        bits = (bits.view(1, -1) if bits.dim() == 1 else bits).to(dev).contiguous()
        K, W = int(bits.size(0)), int(bits.size(1))
    if rep_row is None:
        if K > 1:
            raise ValueError("rep_row is required when bits has %d rows" % K)
        rrow = torch.full((R,), 0 if K == 1 else -1, dtype=torch.long, device=dev)
    else:
        rrow = _pairs(rep_row, 0, dev, "rep_row")
    rflip = torch.full((R,), -1, dtype=torch.long, device=dev) if rep_flip is None else _pairs(rep_flip, 0, dev, "rep_flip")
    if int(rrow.numel()) != R or int(rflip.numel()) != R:
        raise ValueError("rep_graph, rep_row and rep_flip must have one entry per replica each (got %d, %d and %d)"
                         % (R, rrow.numel(), rflip.numel()))
    tw = _twin_in_order(S, twin) if mode == 0 else None
    mx = _node_map_rows(S, data) if mode == 1 else 0
    inputs = S.args() + [_p(bits) if K and W else None, K, W, _p(rg) if R else None, _p(rrow) if R else None,
                         _p(rflip) if R else None, R, _p(tw) if tw is not None and S.E else None, mode, mx]
    built = _rebatch("cal_subset", (S.E, R, mx, mode), inputs, R, 5, (S,), F, lambda: (rg < 0) | (rg >= S.B))
    return _built_batch(S, built, rg, S.no_self_loops, _caller_columns(S, built.edge_src, built.tot[1]))


# ---- the beam step ------------------------------------------------------------------------------------------------------------
def lds_cap(host: bool = False) -> int:
    """``cal_explain_lds_cap()``: the candidates of one graph a beam step takes."""
    return _lib.query("cal_explain_lds_cap", host=host)


def beam_step(bits, n_state, cand_ptr, rep_row, rep_flip, p, flipped, seg_ptr, M: int, done, cf_bits, cf_p, cf_cand, *, beam: int,
              twin=None, use: str = "edges", max_cand: Optional[int] = None):
    """One ``cal_beam_step``: one launch (one workgroup per graph), no read-back.

    ``bits`` int32 / uint32 [B beam, W]: graph g's states are the rows ``g beam ...``, ``n_state`` int64 [B] of them live.  Graph
    g's candidates are ``[cand_ptr[g], cand_ptr[g + 1])`` (int64 [B + 1]) of the R entries of ``rep_row`` / ``rep_flip`` (int64,
    as ``subset_batch`` took them), ``p`` (float32: the replica's ``p(ŷ)``) and ``flipped`` (bool / uint8: its argmax is no longer
    ŷ).  ``seg_ptr`` [B + 1] / ``M``: the element segments (``edge_ptr`` / E for ``use="edges"``, ``ptr`` / N for ``"nodes"``);
    ``twin`` as in ``subset_batch``.  ``done`` uint8 [B], ``cf_bits`` int32 [B, W], ``cf_p`` float32 [B] and ``cf_cand`` int64
    [B] are read and written in place: a graph whose best candidate is flipped gets ``done = 1``, its child, its p and its
    index.  A graph that is done or has no candidate keeps ``n_state_out = 0``.  Otherwise the candidates are ordered by (flipped
    first, ``p`` ascending through ``score_key``, ``rep_row``, ``rep_flip``), equal children are one child (the earliest stands)
    and the first ``beam`` distinct children are the next states.  ``max_cand`` (by default and at most ``cal_explain_lds_cap()``)
    bounds a graph's candidates: a graph with more gets ``status = 2`` and is not worked on.

    -> ``(bits_out int32 [B beam, W], p_state_out float32 [B beam], n_state_out int64 [B], status int32 [B])``; rows and entries
    beyond ``n_state_out`` are zero."""
    _check_use(use)
    bits = _words(bits).contiguous()
    dev, host = bits.device, not bits.is_cuda
    B, W = int(n_state.numel()), int(bits.size(-1))
    beam = int(beam)
    if not 1 <= beam <= BEAM_MAX:
        raise ValueError("beam must be in [1, %d]" % BEAM_MAX)
    if bits.dim() != 2 or int(bits.size(0)) != B * beam or W > BEAM_WORDS:
        raise ValueError("bits must be [B beam, W] with W <= %d" % BEAM_WORDS)
    cap = lds_cap(host)
    max_cand = cap if max_cand is None else int(max_cand)
    if max_cand > cap:
        raise ValueError("max_cand = %d exceeds cal_explain_lds_cap() = %d" % (max_cand, cap))
    R = int(rep_row.numel())
    long = lambda t: t.to(device=dev, dtype=torch.long).contiguous()
    n_state, cand_ptr, rep_row, rep_flip, seg_ptr = long(n_state), long(cand_ptr), long(rep_row), long(rep_flip), long(seg_ptr)
    p = p.to(device=dev, dtype=torch.float32).contiguous()
    fl = flipped.to(dev).contiguous()
    fl = fl.view(torch.uint8) if fl.dtype == torch.bool else fl.to(torch.uint8)
    if done.dtype != torch.uint8 or cf_cand.dtype != torch.long or cf_p.dtype != torch.float32 or _words(cf_bits, "cf_bits").shape != (B, W):
        raise TypeError("done must be uint8 [B], cf_bits int32 [B, W], cf_p float32 [B] and cf_cand int64 [B]")
    for t in (done, cf_bits, cf_p, cf_cand):
        if not t.is_contiguous() or t.device != dev:
            raise ValueError("done, cf_bits, cf_p and cf_cand are written in place: contiguous, on the device of bits")
    tw = None
    if twin is not None and use == "edges":
        if int(twin.numel()) != int(M):
            raise ValueError("twin must have one entry per edge column")
        tw = twin.to(device=dev, dtype=torch.int32).contiguous()
    bits_out = torch.zeros_like(bits)
    p_out = torch.zeros(B * beam, dtype=torch.float32, device=dev)
    n_out = torch.zeros(B, dtype=torch.long, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.call("cal_beam_step", _p(bits) if bits.numel() else None, B, beam, W, _p(n_state) if B else None, _p(cand_ptr),
              _p(rep_row) if R else None, _p(rep_flip) if R else None, _p(p) if R else None, _p(fl) if R else None, R, _p(seg_ptr),
              int(M), _p(tw) if tw is not None and M else None, 0 if use == "edges" else 1, max_cand, _p(done) if B else None,
              _p(bits_out) if bits.numel() else None, _p(p_out) if B else None, _p(n_out) if B else None,
              _p(_words(cf_bits, "cf_bits")) if bits.numel() else None, _p(cf_p) if B else None, _p(cf_cand) if B else None,
              _p(status) if B else None, None if host else _stream(), host=host)
    return bits_out, p_out, n_out, status


# ---- the search ---------------------------------------------------------------------------------------------------------------
@dataclass
class Counterfactual:
    """The counterfactual sets of a batch.  ``removed`` bool [E] (``use="edges"``) or [N] (``"nodes"``) in the caller's numbering:
    the elements whose removal flips graph g's prediction (both columns of an undirected edge); all False for a graph without
    one.  ``size`` int64 [B]: the players removed, -1 where none was found; ``found`` bool [B].  ``p_full`` [B] and ``yhat``
    int64 [B]: the whole graph's probability of its own argmax and that argmax; ``p_cf`` float32 [B] (NaN: not found) and
    ``y_cf`` int64 [B] (-1: not found): ``p(ŷ)`` and the argmax with the set removed.  ``rounds``: rounds run; ``replicas``: graphs
    run besides the whole batch, in ``forwards`` forwards (the whole batch's included).  ``twin``: the reverse-column map int32
    [E] in the caller's numbering when ``undirected`` built one, else ``None``."""
    removed: torch.Tensor
    size: torch.Tensor
    found: torch.Tensor
    p_full: torch.Tensor
    p_cf: torch.Tensor
    yhat: torch.Tensor
    y_cf: torch.Tensor
    rounds: int
    replicas: int
    forwards: int
    twin: Optional[torch.Tensor] = None


def _limits(P, n, use, max_remove):
    """int64 [B]: the removals tried per graph of ``n`` players -- ``max_remove``, by default ``ceil(n / 2)`` capped at 16; never
    more than the players, and with ``use="nodes"`` one node always stays."""
    lim = torch.clamp((n + 1) // 2, max=16) if max_remove is None else torch.clamp(n, max=int(max_remove))
    return torch.minimum(lim, (P.nodes - 1).clamp(min=0)) if use == "nodes" else lim


def _check_cf_args(use, undirected, head, chunk, max_remove, beam=1):
    h, chunk = _check_driver_args(use, undirected, head, chunk)
    if isinstance(beam, bool) or not isinstance(beam, int) or not 1 <= beam <= BEAM_MAX:
        raise ValueError("beam must be an int in [1, %d]" % BEAM_MAX)
    if max_remove is not None and (isinstance(max_remove, bool) or not isinstance(max_remove, int) or max_remove < 0):
        raise ValueError("max_remove must be an int >= 0")
    return h, chunk


def _counterfactual(model, data, lay, use, undirected, h, beam, max_remove, elements, chunk):
    """-> ``Counterfactual`` over the edge columns in ``lay``'s graph order (``removed`` and ``twin`` index that order).  Called
    in eval mode under no_grad."""
    src = _grouped(data, lay)
    yhat, p_full, _ = _whole(model, src, h)
    P = _Players(data, lay, src, use, undirected)
    dev, B, M = P.dev, P.B, P.M
    host = dev.type != "cuda"
    pl = torch.ones(M, dtype=torch.bool, device=dev) if P.rep is None else P.rep.clone()
    if elements is not None:
        pl = pl & _members(elements, M, lay, use, P.twin)
    n = P.count(pl)
    lim = _limits(P, n, use, max_remove)
    W = max(1, -(-int(P.max_seg) // 32))
    if W > BEAM_WORDS:
        raise ValueError("a graph has %d elements: the search covers at most %d per graph" % (P.max_seg, 32 * BEAM_WORDS))
    cap = lds_cap(host)
    n_max, rounds_max = torch.stack([n.max(), lim.max()]).tolist() if B else (0, 0)      # (a read-back, once)
    if beam * n_max > cap:
        raise ValueError("beam x players = %d x %d = %d candidates of one graph exceed cal_explain_lds_cap() = %d"
                         % (beam, n_max, beam * n_max, cap))
    gid, loc = P.gid, torch.arange(M, device=dev) - P.seg[P.gid]
    word, shift = loc >> 5, (loc & 31).view(M, 1)
    full = pack_bits(torch.ones(M, dtype=torch.bool, device=dev), P.seg, P.max_seg)
    bits = torch.zeros(B, beam, W, dtype=torch.int32, device=dev)
    bits[:, 0] = full
    bits = bits.view(B * beam, W)
    n_state = (lim > 0).long()
    done = (lim <= 0).to(torch.uint8)
    cf_bits, cf_p = full.clone(), torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    cf_cand, y_cf = torch.full((B,), -1, dtype=torch.long, device=dev), torch.full((B,), -1, dtype=torch.long, device=dev)
    slots = torch.arange(beam, device=dev).view(1, beam)
    rounds = replicas = 0
    forwards = 1
    for t in range(rounds_max):
        # every live state of every graph still searched, expanded by every player still present in it
        live = (slots < n_state.view(B, 1)) & ((done == 0) & (lim > t)).view(B, 1)                       # [B, beam]
        here = (bits.view(B, beam, W).permute(0, 2, 1)[gid, word] >> shift) & 1                          # [M, beam]
        mask = pl.view(M, 1) & live[gid] & (here == 1)
        cnt = torch.zeros(B, dtype=torch.long, device=dev).index_add_(0, gid, mask.sum(1))
        total = int(cnt.sum())                               # the round's one read-back: 0 when every graph is done
        if total == 0:
            break
        idx = torch.argsort((~mask).view(-1).to(torch.uint8), stable=True)[:total]                      # (e, s) ascending: by graph
        e, s = idx // beam, idx % beam
        rg, rflip = gid[e], loc[e]
        rrow = rg * beam + s
        cand_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(cnt, 0)])
        p = torch.empty(total, dtype=torch.float32, device=dev)
        am = torch.empty(total, dtype=torch.long, device=dev)
        for i in range(0, total, chunk):
            g = rg[i:i + chunk]
            rb = subset_batch(src, g, bits, rep_row=rrow[i:i + chunk], rep_flip=rflip[i:i + chunk], use=use, twin=P.twin)
            lp = _replica_log_probs(model, rb, h)
            p[i:i + chunk] = _p_at(lp, yhat[g])
            am[i:i + chunk] = lp.argmax(-1)
            forwards += 1
        before = done.clone()
        bits, _, n_state, _ = beam_step(bits, n_state, cand_ptr, rrow, rflip, p, am != yhat[rg], P.seg, M, done, cf_bits, cf_p,
                                        cf_cand, beam=beam, twin=P.twin, use=use, max_cand=cap)
        y_cf = torch.where((done != 0) & (before == 0), am[cf_cand.clamp(0, total - 1)], y_cf)
        rounds, replicas = rounds + 1, replicas + total
    found = cf_cand >= 0
    removed = found[gid] & ~unpack_bits(cf_bits, P.seg, M) if M else torch.zeros(0, dtype=torch.bool, device=dev)
    size = torch.where(found, P.count(removed & pl), torch.full_like(cf_cand, -1))
    return Counterfactual(removed=removed, size=size, found=found, p_full=p_full, p_cf=cf_p, yhat=yhat, y_cf=y_cf, rounds=rounds,
                          replicas=replicas, forwards=forwards, twin=P.twin)


def _cf_caller_order(cf, lay, use):
    if use == "edges" and lay.order is not None:
        removed = torch.empty_like(cf.removed)
        removed[lay.order] = cf.removed
        cf.removed = removed
        cf.twin = None if cf.twin is None else lay.caller_twin(cf.twin)
    return cf


def counterfactual(model, data, *, use: str = "edges", undirected=None, head: str = "o", beam: int = 4, max_remove=None,
                   elements=None, chunk: int = 512) -> Counterfactual:
    """A small set of edges (``use="edges"``; ``undirected`` as in ``explain``: undirected edges) or nodes of every graph of
    ``data`` whose removal changes ``model``'s prediction, by beam search.

    One eval forward of the whole batch (untiled, the route the replicas take) gives ŷ_g, the argmax of ``head`` (``"c"``,
    ``"o"`` or ``"co"``), and ``p_full``.  The players are as in ``shapley``: edge columns, pairs of twin columns, or nodes;
    ``elements`` (a bool mask [E] / [N]) restricts them, every other element always stays.  A state is a subset of a graph's
    elements, one bitset row; every graph starts from its full set.  Round t expands every live state of every graph still
    searched by every player still present in it: the replicas are "state minus that player" (``subset_batch`` in chunks of at
    most ``chunk`` graphs, one forward each), and one ``cal_beam_step`` then takes, per graph, the replica whose argmax left ŷ_g
    (the one with the smallest ``p(ŷ_g)``; ties by state row and player) as the counterfactual -- or else keeps the ``beam``
    distinct children with the smallest ``p(ŷ_g)`` as the next states.  So the set found in round t has t + 1 players, and a
    graph is searched for ``max_remove`` rounds: by default ``ceil(players / 2)``, at most 16; with ``use="nodes"`` one node
    always stays.  ``beam=1`` is the greedy search.  With a beam of at least the number of subsets of the minimum size the
    result is a minimum counterfactual set.

    Besides the builder's totals there is one read-back per round (the candidates left: none once every graph is done) and one
    of the player counts up front.  A batch in which ``beam x players`` of some graph exceeds ``cal_explain_lds_cap()`` raises
    ``ValueError``.  CPU-resident models go through libcalhost and the operator-level ``model(data)``.  Like ``explain``, it runs
    in eval mode under ``no_grad`` and leaves parameters, optimizer state, the engine's step counter, BatchNorm statistics, the
    RNG states and ``model.training`` as they were."""
    h, chunk = _check_cf_args(use, undirected, head, chunk, max_remove, beam)
    with _eval_mode(model):
        lay = _Layout(data)
        cf = _cf_caller_order(_counterfactual(model, data, lay, use, undirected, h, beam, max_remove, elements, chunk), lay, use)
    return cf


# ---- the smallest flipping prefix of a ranking --------------------------------------------------------------------------------
def _ranking_flip(model, data, lay, order, use, undirected, h, max_remove, chunk):
    """-> ``(size int64 [B], p_full, ŷ, replicas, forwards)``.  Called in eval mode under no_grad."""
    from .coalition import coalition_batch
    forwards = 0
    if order is None:                                                    # the causal attention, as explain ranks it
        edge, node = _scores(model, data)
        order = (edge if use == "edges" else node).clone()
        forwards = 1
    src = _grouped(data, lay)
    yhat, p_full, _ = _whole(model, src, h)
    P = _Players(data, lay, src, use, undirected)
    dev, B, M = P.dev, P.B, P.M
    if not torch.is_tensor(order) or order.dim() != 1 or int(order.numel()) != M:
        raise ValueError("order must be a score vector with one entry per %s (%d)" % ("edge column" if use == "edges" else "node", M))
    order = order.to(device=dev, dtype=torch.float32)
    if use == "edges" and lay.order is not None:
        order = order[lay.order]
    key = P.rank(order).view(1, M)
    n = P.count(torch.ones(M, dtype=torch.bool, device=dev) if P.rep is None else P.rep)
    lim = _limits(P, n, use, max_remove)
    total = int(lim.sum()) if B else 0                                   # (a read-back: the number of replicas)
    start = torch.cumsum(lim, 0) - lim
    rg = torch.repeat_interleave(torch.arange(B, device=dev), lim, output_size=total)
    k = torch.arange(total, device=dev) - start[rg] + 1                  # replica (g, k): the top k of the ranking removed
    big = torch.iinfo(torch.long).max
    hit = torch.full((total,), big, dtype=torch.long, device=dev)
    for i in range(0, total, chunk):
        g = rg[i:i + chunk]
        rb = coalition_batch(src, g, k[i:i + chunk], key, use=use, invert=True)
        flipped = _replica_log_probs(model, rb, h).argmax(-1) != yhat[g]
        hit[i:i + chunk] = torch.where(flipped, k[i:i + chunk], hit[i:i + chunk])
        forwards += 1
    size = torch.full((B,), big, dtype=torch.long, device=dev).scatter_reduce_(0, rg, hit, "amin")
    return torch.where(size < big, size, torch.full_like(size, -1)), p_full, yhat, total, forwards + 1


def ranking_flip(model, data, order=None, *, use: str = "edges", undirected=None, head: str = "o", max_remove=None,
                 chunk: int = 512) -> dict:
    """The smallest prefix of a ranking whose removal flips the prediction: what a counterfactual set costs when the elements
    are taken in the order of a score instead of searched for.

    ``order`` is a score vector [E] / [N] -- high first, NaN last, as ``explain`` ranks; with ``undirected`` one rank per
    undirected edge -- and by default the causal attention exactly as ``explain`` ranks it.  For graph g and k = 1 ..
    ``max_remove`` (the default and the bounds of ``counterfactual``) the replica without the top k players is run; prefixes
    are nested, so the replicas are ``coalition_batch``'s with ``invert=True``, in chunks of at most ``chunk`` graphs.

    Returns ``size`` int64 [B] (the smallest flipping k; -1: none up to the bound), ``found`` bool [B], ``p_full`` [B], ``yhat``
    int64 [B] and the host ints ``replicas`` and ``forwards`` (the whole batch's included, and the scores' when ``order`` is
    not given).  It leaves the model as ``explain`` does."""
    h, chunk = _check_cf_args(use, undirected, head, chunk, max_remove)
    with _eval_mode(model):
        size, p_full, yhat, replicas, forwards = _ranking_flip(model, data, _Layout(data), order, use, undirected, h, max_remove,
                                                               chunk)
    return {"size": size, "found": size >= 0, "p_full": p_full, "yhat": yhat, "replicas": replicas, "forwards": forwards}


# ---- the report ---------------------------------------------------------------------------------------------------------------
_SUMS = ("graphs", "found", "size", "attention_found", "attention_size", "random_found", "random_size", "gt_removed_in",
         "gt_removed", "gt_inside")


def _found_size(size):
    found = size >= 0
    return [found.sum().double(), torch.where(found, size, torch.zeros_like(size)).sum().double()]


def _report_sums(model, data, use, undirected, h, beam, max_remove, chunk, gt, seed):
    """-> (fp64 [10] on the device, ``_SUMS``; replicas; forwards) of one batch.  Called in eval mode under no_grad."""
    lay = _Layout(data)
    cf = _cf_caller_order(_counterfactual(model, data, lay, use, undirected, h, beam, max_remove, None, chunk), lay, use)
    att = _ranking_flip(model, data, lay, None, use, undirected, h, max_remove, chunk)
    M = int(cf.removed.numel())
    rnd_order = torch.rand(M, generator=torch.Generator().manual_seed(int(seed))).to(cf.removed.device)
    rnd = _ranking_flip(model, data, lay, rnd_order, use, undirected, h, max_remove, chunk)
    dev, B = cf.size.device, int(cf.size.numel())
    parts = [torch.as_tensor(float(B), dtype=torch.float64, device=dev)] + _found_size(cf.size) + _found_size(att[0]) + _found_size(rnd[0])
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    if gt is None:
        parts += [zero, zero, zero]
    else:
        gt = _keep8(gt, M, dev, "edge_gt" if use == "edges" else "node_gt").view(torch.bool)
        rep = _representatives(cf.twin) if cf.twin is not None else torch.ones(M, dtype=torch.bool, device=dev)
        gid = data.batch.to(dev)[data.edge_index[0].to(dev)] if use == "edges" else data.batch.to(dev)
        taken = cf.removed & rep
        outside = torch.zeros(B, dtype=torch.long, device=dev).index_add_(0, gid, (taken & ~gt).long())
        parts += [(taken & gt).sum().double(), taken.sum().double(), (cf.found & (outside == 0)).sum().double()]
    return torch.stack(parts), cf.replicas + att[3] + rnd[3], cf.forwards + att[4] + rnd[4]


def _report(row, replicas, forwards, with_gt) -> dict:
    s = dict(zip(_SUMS, row))
    div = lambda a, b: a / b if b else float("nan")
    res = {"graphs": int(s["graphs"]), "flip_rate": div(s["found"], s["graphs"]), "size_mean": div(s["size"], s["found"]),
           "attention_flip_rate": div(s["attention_found"], s["graphs"]),
           "attention_size_mean": div(s["attention_size"], s["attention_found"]),
           "random_flip_rate": div(s["random_found"], s["graphs"]), "random_size_mean": div(s["random_size"], s["random_found"]),
           "replicas": replicas, "forwards": forwards, "sums": list(row)}
    if with_gt:
        res["removed_in_motif"] = div(s["gt_removed_in"], s["gt_removed"])
        res["inside_motif_rate"] = div(s["gt_inside"], s["found"])
    return res


def counterfactual_report(model, data, *, use: str = "edges", undirected=None, head: str = "o", beam: int = 4, max_remove=None,
                          chunk: int = 512, edge_gt=None, seed: int = 0) -> dict:
    """The counterfactual search of one batch against two rankings.

    Always reported: ``flip_rate`` (graphs with a counterfactual set up to the bound) and ``size_mean`` (its mean size over those
    graphs) of ``counterfactual``; ``attention_flip_rate`` / ``attention_size_mean``: the same for ``ranking_flip`` under the
    causal attention; ``random_flip_rate`` / ``random_size_mean``: under a random ranking drawn from ``seed`` (a CPU generator
    of its own: no RNG state moves).  With a ground truth ``edge_gt`` (a bool mask over the elements -- [E], or [N] with
    ``use="nodes"`` --, e.g. ``spmotif.ground_truth``): ``removed_in_motif``, the share of the removed players that lie inside
    it, and ``inside_motif_rate``, the share of the found sets that lie inside it entirely.  Also ``graphs``, ``replicas``,
    ``forwards`` and ``sums`` (the raw sums, which add over batches).  The sums are formed on the device and read back once."""
    h, chunk = _check_cf_args(use, undirected, head, chunk, max_remove, beam)
    with _eval_mode(model):
        sums, replicas, forwards = _report_sums(model, data, use, undirected, h, beam, max_remove, chunk, edge_gt, seed)
    return _report(sums.tolist(), replicas, forwards, edge_gt is not None)


def eval_counterfactual(model, loader, device, *, use: str = "edges", undirected=None, head: str = "o", beam: int = 4,
                        max_remove=None, chunk: int = 512, edge_gt=None, seed: int = 0) -> dict:
    """``counterfactual_report`` over a loader: the same figures from the sums over all its batches (one read-back per batch;
    batch i draws its random ranking from ``seed + i``).  ``edge_gt``: ``None``, a callable ``batch -> bool mask``, or
    ``"spmotif"`` for ``spmotif.ground_truth`` (the edge mask, the node mask with ``use="nodes"``)."""
    h, chunk = _check_cf_args(use, undirected, head, chunk, max_remove, beam)
    if edge_gt == "spmotif":
        from .spmotif import ground_truth
        edge_gt = lambda b: ground_truth(b)[1 if use == "edges" else 0]
    total, replicas, forwards = [0.0] * len(_SUMS), 0, 0
    with _eval_mode(model):
        for i, data in enumerate(loader):
            data = data.to(device)
            sums, r, f = _report_sums(model, data, use, undirected, h, beam, max_remove, chunk,
                                      None if edge_gt is None else edge_gt(data), seed + i)
            total = [a + b for a, b in zip(total, sums.tolist())]
            replicas, forwards = replicas + r, forwards + f
    return _report(total, replicas, forwards, edge_gt is not None)
