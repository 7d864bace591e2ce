"""Occlusion attributions: leave-one-out scores of single edges / nodes, and how well CAL's causal attention agrees with them.

``explain``, ``fidelity``, ``intervene`` and ``structure_intervention`` all take column 1 of the soft masks as *the* explanation.
But the backbone convolutions run on the full, unweighted ``edge_index`` before any mask exists (model.py:239-258), so an edge
with a near-zero causal score can still carry the label signal into ``xo``.  Attention cannot see that; removing the element and
running the model again can.  Leave-one-out occlusion is the model-agnostic yardstick:

* ``occlude_batch(data, rep_graph, rep_elem, use=..., twin=...)`` -> ``Batch``: replica r is graph ``rep_graph[r]`` of ``data``
  without the element ``rep_elem[r]`` (``cal_occlude_count`` / ``cal_occlude_write``: two launches and one read-back of the
  totals on the GPU, libcalhost for CPU tensors), with the layout facts that keep the engine on its per-graph route.
* ``occlusion(model, data, use=..., undirected=...)`` (also ``model.occlusion``) -> ``Occlusion``: per element
  ``p_full(ŷ_g) - p_without_element(ŷ_g)``.
* ``rank_agreement(a, b, seg_ptr, max_seg, ...)``: per segment the integer counts behind Spearman's rho, Kendall's tau-b and the
  top-k Jaccard overlap of two score vectors (``cal_rank_agreement``), and the three figures in fp64.
* ``faithfulness(model, data, ...)`` (also ``model.faithfulness``) / ``eval_faithfulness(model, loader, device, ...)``: the causal
  scores against the occlusion scores.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .explain import _eval_mode, _keep8, _Layout, rank_segment_pairs, rank_segments
from .plan import _p, _stream
from .replica import (_agree_report, _agree_sums, _built_batch, _caller_columns, _causal_in_order, _check_driver_args, _check_topk,
                      _check_use, _feature_width, _grouped, _members, _p_at, _pairs, _Players, _rebatch, _replica_log_probs,
                      _Source, _twin_in_order, _whole)

__all__ = ["Occlusion", "occlude_batch", "occlusion", "rank_agreement", "faithfulness", "eval_faithfulness"]


def occlude_batch(data, rep_graph, rep_elem, *, use: str = "edges", twin=None):
    """``R`` replicas of graphs of ``data``, each with one element removed, as a ``cal_amd.data.Batch`` the engine can run.

    Replica r is graph ``rep_graph[r]`` (int64 [R]; an id outside the batch gives a replica with no node, counted in
    ``empty_graphs``) without ``rep_elem[r]``, a global id of ``data``: with ``use="edges"`` an edge column -- all nodes stay, all
    of the graph's columns stay in order except that one and, when ``twin`` (int32 [E], as ``edge_twins`` gives it) is passed and
    ``twin[rep_elem[r]] >= 0``, its twin (a self loop is its own twin: one column goes); with ``use="nodes"`` a node -- its row is
    left out, later nodes move down by one, every column incident to it is dropped and the other endpoints are rewritten.  An
    element that is not one of the graph's (``-1``, say) removes nothing: the control replica.  A source column that leaves its
    graph's node range is dropped.  A graph may appear in any number of replicas.

    The result carries ``x`` / ``feat`` as ``data`` does (row copies), ``edge_index``, ``batch``, ``ptr``, ``edge_ptr``,
    ``num_graphs = R``, ``max_nodes``, ``max_edges``, ``no_self_loops`` (inherited), no tiles, ``y = data.y[rep_graph]`` (``None``
    when ``data`` has none or a graph id is outside the batch), ``node_src`` / ``edge_src`` (int64: the source element of every
    new node / column) and the host int ``empty_graphs``.

    CUDA tensors: ``cal_occlude_count`` and ``cal_occlude_write`` on the current stream with one read-back of the totals between
    them; CPU tensors: libcalhost.  Inputs other than ``Batch`` objects get their layout derived as in ``splice_batches``; edge
    columns that are not grouped by graph are put in stable graph order first and ``edge_src`` is mapped back to the caller's."""
    _check_use(use)
    mode = 0 if use == "edges" else 1
    S = _Source(data)
    dev, F = S.dev, _feature_width(S, "occlude_batch")
    if rep_graph is None or rep_elem is None:
        raise TypeError("rep_graph and rep_elem are required")
    rg, re = _pairs(rep_graph, 0, dev, "rep_graph"), _pairs(rep_elem, 0, dev, "rep_elem")
    R = int(rg.numel())
    if int(re.numel()) != R:
        raise ValueError("rep_graph and rep_elem must have one entry per replica each (got %d and %d)" % (R, re.numel()))
    tw = _twin_in_order(S, twin) if mode == 0 else None
    if S.order is not None and mode == 0 and S.E:          # the caller's column ids -> positions in graph order
        inv = torch.empty_like(S.order)
        inv[S.order] = torch.arange(S.E, device=dev)
        re = torch.where((re >= 0) & (re < S.E), inv[re.clamp(0, S.E - 1)], torch.full_like(re, -1))
    inputs = S.args() + [_p(rg) if R else None, _p(re) if R else None, R, mode, _p(tw) if S.E else None]
    built = _rebatch("cal_occlude", (S.E, R), inputs, R, 5, (S,), F, lambda: (rg < 0) | (rg >= S.B))
    return _built_batch(S, built, rg, S.no_self_loops, _caller_columns(S, built.edge_src, built.tot[1]))


# ---- leave-one-out scores -----------------------------------------------------------------------------------------------------
@dataclass
class Occlusion:
    """Leave-one-out scores of a batch.  ``score`` float32 [E] (``use="edges"``) or [N] (``"nodes"``):
    ``p_full_g(ŷ_g) - p_without_element(ŷ_g)`` at the chosen head; NaN for an element that was not occluded (outside
    ``elements``, or its replica would have no node).  ``p_full`` [B] and ``yhat`` int64 [B]: the whole graph's probability of
    its own argmax and that argmax.  ``replicas``: graphs run besides the whole batch, in ``forwards`` forwards (the whole
    batch's included).  ``twin``: the reverse-column map int32 [E] when ``undirected`` built one, else ``None``."""
    score: torch.Tensor
    p_full: torch.Tensor
    yhat: torch.Tensor
    replicas: int
    forwards: int
    twin: Optional[torch.Tensor] = None


def _occlusion(model, data, lay, use, undirected, h, elements, chunk):
    """-> ``(Occlusion, representatives bool [M] or None)`` over the edge columns in ``lay``'s graph order (``score`` and
    ``twin`` index that order).  Called in eval mode under no_grad."""
    src = _grouped(data, lay)
    yhat, p_full, _ = _whole(model, src, h)
    P = _Players(data, lay, src, use, undirected)
    dev, M, gid, twin, rep = P.dev, P.M, P.gid, P.twin, P.rep
    low = 0 if use == "edges" else 1                                     # edges: every node stays, a graph with one has a replica
    want = None if elements is None else _members(elements, M, lay, use, twin)
    cand = P.nodes[gid] > low if M else torch.zeros(0, dtype=torch.bool, device=dev)
    for m in (rep, want):
        if m is not None:
            cand = cand & m
    idx = cand.nonzero().view(-1)                                        # (a read-back: the number of replicas)
    score = torch.full((M,), float("nan"), dtype=torch.float32, device=dev)
    n, forwards = int(idx.numel()), 1
    graph = gid[idx]
    for i in range(0, n, chunk):
        ids, rg = idx[i:i + chunk], graph[i:i + chunk]
        rb = occlude_batch(src, rg, ids, use=use, twin=twin)
        lp = _replica_log_probs(model, rb, h)                            # [R, C]
        sc = p_full[rg] - _p_at(lp, yhat[rg])
        score[ids] = sc
        if twin is not None:
            t = twin[ids].long()
            score[torch.where(t >= 0, t, ids)] = sc                      # both columns receive the score
        forwards += 1
    return Occlusion(score=score, p_full=p_full, yhat=yhat, replicas=n, forwards=forwards, twin=twin), rep


def occlusion(model, data, *, use: str = "edges", undirected=None, head: str = "o", elements=None, chunk: int = 512) -> Occlusion:
    """Leave-one-out occlusion scores of every edge column (``use="edges"``) or node (``"nodes"``) of ``data``.

    One eval forward of the whole batch (untiled, the route the replicas take) gives ŷ_g, the argmax of ``head`` (``"c"``,
    ``"o"`` or ``"co"``), and ``p_full``.  Every element then gets a replica of its graph without it (``occlude_batch``); the
    replicas run in chunks of at most ``chunk`` graphs (512 is the bound of the engine's one-launch readout), and
    ``score[e] = p_full_g(ŷ_g) - p_without_e(ŷ_g)``.  ``undirected=None`` removes each column alone; ``"mean"`` / ``"max"`` /
    ``"min"`` (all three the same here: the names ``explain`` takes) treat one undirected edge as one element -- the lower column
    of a pair represents it, both columns are removed and both receive the score.  ``elements``: a bool mask [E] / [N] of the
    elements to occlude (an undirected edge when either of its columns is named); the others score NaN.  A replica that would
    have no node (a one-node graph's node) is not run and scores NaN.

    Cost: one forward per ``chunk`` elements besides the first -- about 12.5 k replicas, 25 forwards, for the headline batch of
    128 SPMotif graphs, and one builder call (two launches and a read-back) per forward.  Not meant for 5000-node graphs
    without ``elements``.  CPU-resident models go through libcalhost and the operator-level ``model(data)``.  Like ``explain``,
    it runs in eval mode under ``no_grad`` and leaves parameters, optimizer state, the engine's step counter, BatchNorm
    statistics, the RNG states and ``model.training`` as they were."""
    h, chunk = _check_driver_args(use, undirected, head, chunk)
    with _eval_mode(model):
        lay = _Layout(data)
        occ, _ = _occlusion(model, data, lay, use, undirected, h, elements, chunk)
        if use == "edges" and lay.order is not None:                    # back to the caller's column order
            score = torch.empty_like(occ.score)
            score[lay.order] = occ.score
            occ.score = score
            occ.twin = None if occ.twin is None else lay.caller_twin(occ.twin)
    return occ


# ---- rank agreement -----------------------------------------------------------------------------------------------------------
def _agreement_metrics(counts: torch.Tensor) -> torch.Tensor:
    """fp64 [B, 3]: Spearman's rho, Kendall's tau-b and the top-k Jaccard overlap from the integer counts; NaN where a
    denominator is zero or fewer than two elements take part."""
    n, C, D, Ta, Tb, Saa, Sbb, Sab, kg, inter = counts.unbind(1)
    ok = n >= 2
    nan = torch.full(n.shape, float("nan"), dtype=torch.float64, device=counts.device)

    def ratio(num, den):
        good = ok & (den > 0)
        return torch.where(good, num / torch.where(good, den, torch.ones_like(den)), nan)
    centre = n * (n + 1) * (n + 1)                                       # sum of the doubled mid-ranks is n (n + 1): n mean^2
    rho = ratio((Sab - centre).double(), ((Saa - centre).double() * (Sbb - centre).double()).sqrt())
    n0 = n * (n - 1) // 2
    tau = ratio((C - D).double(), ((n0 - Ta).double() * (n0 - Tb).double()).sqrt())
    jac = ratio(inter.double(), (2 * kg - inter).double())
    return torch.stack([rho, tau, jac], 1)


def rank_agreement(a: torch.Tensor, b: torch.Tensor, seg_ptr: torch.Tensor, max_seg: int, *, sel=None, ratio=None, k=None):
    """One ``cal_rank_agreement`` call over the segments ``[seg_ptr[g], seg_ptr[g+1])`` of the float32 vectors ``a`` and ``b``.

    An element takes part iff ``sel`` (bool [M] or ``None``) marks it and neither value is NaN.  Returns ``(counts int64
    [B, 10], metrics fp64 [B, 3])``.  A counts row is ``n, C, D, Ta, Tb, Saa, Sbb, Sab, k_g, inter``: the elements taking part,
    the concordant and discordant pairs, the pairs tied in ``a`` / in ``b`` (a pair tied in both counts in each), the sums of
    ``(2ra)^2``, ``(2rb)^2`` and ``(2ra)(2rb)`` over the doubled mid-ranks, ``k_g`` (``min(k, n)`` or ``ceil(ratio n)``) and the
    overlap of the two top-``k_g`` sets in ``explain``'s order (value descending, then index).  A segment longer than
    ``max_seg`` (a host int, below 2^20) gets ``n = -1``.  A metrics row is Spearman's rho (the Pearson correlation of the
    mid-ranks), Kendall's tau-b ``(C - D) / sqrt((n0 - Ta)(n0 - Tb))`` with ``n0 = n (n - 1) / 2`` and the Jaccard overlap
    ``inter / (2 k_g - inter)``; NaN where the denominator is zero or ``n < 2``.  The counts are integers, so the GPU, the host
    library and any restatement agree bit for bit."""
    kc, rt = _check_topk(ratio, k, "rank_agreement")
    if a.dim() != 1 or b.dim() != 1 or a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel():
        raise TypeError("a and b must be 1-D float32 tensors of one length")
    if a.device != b.device:
        raise ValueError("a and b must be on one device")
    dev, host = a.device, not a.is_cuda
    a, b = a.contiguous(), b.contiguous()
    M, B = int(a.numel()), int(seg_ptr.numel()) - 1
    seg_ptr = seg_ptr.to(device=dev, dtype=torch.long).contiguous()
    s8 = _keep8(sel, M, dev, "sel")
    wsb = _lib.query("cal_rank_agreement_ws", M, B, int(max_seg), host=host)
    counts = torch.empty(B, 10, dtype=torch.long, device=dev)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.long, device=dev) if wsb else None
    _lib.call("cal_rank_agreement", _p(a) if M else None, _p(b) if M else None, M, _p(seg_ptr), B, int(max_seg),
              _p(s8) if M else None, kc, rt, _p(counts), _p(ws), wsb, None if host else _stream(), host=host)
    return counts, _agreement_metrics(counts)


# ---- causal attention against occlusion ---------------------------------------------------------------------------------------
_ROW = 11          # the three figures' sums, then the graphs where each is defined (_agree_sums); graphs; sum and count of the
#                    occlusion score inside the causal top-k and outside it


def _faith_sums(model, data, use, undirected, h, ratio, k, elements, chunk):
    """One batch's sums [_ROW] fp64 on the device, the replicas and forwards it took (host ints), and the pieces the sums are
    made of ``(causal score, occlusion score, sel, seg_ptr, max_seg, top-k mask)``, all over the columns in graph order.
    Called in eval mode under no_grad."""
    causal, lay = _causal_in_order(model, data, use)
    occ, rep = _occlusion(model, data, lay, use, undirected, h, elements, chunk)
    seg, max_seg = (lay.ptr, lay.max_nodes) if use == "nodes" else (lay.edge_ptr, lay.max_edges)
    if undirected is None:
        top = rank_segments(causal, seg, max_seg, ratio=ratio, k=k)[0]
    else:                        # one symmetrised score per undirected edge, as explain; the top-k mask comes from the same call
        top, _, _, causal = rank_segment_pairs(causal, seg, max_seg, occ.twin, undirected, ratio=ratio, k=k)
    counts, met = rank_agreement(causal, occ.score, seg, max_seg, sel=rep, ratio=ratio, k=k)
    took = ~torch.isnan(occ.score)
    if rep is not None:
        took = took & rep
    sc = occ.score.double()
    zero = torch.zeros_like(sc)
    row = torch.cat([_agree_sums(met),
                     torch.stack([torch.as_tensor(float(lay.B), dtype=torch.float64, device=sc.device),
                                  torch.where(took & top, sc, zero).sum(), (took & top).sum().double(),
                                  torch.where(took & ~top, sc, zero).sum(), (took & ~top).sum().double()])])
    return row, occ.replicas, occ.forwards, (causal, occ.score, rep, seg, max_seg, top)


def _faith_report(row, replicas, forwards) -> dict:
    nan = float("nan")
    n = row[6]
    res = _agree_report(row[:6], n)
    res["occ_top"] = row[7] / row[8] if row[8] else nan
    res["occ_rest"] = row[9] / row[10] if row[10] else nan
    res["graphs"], res["elements"], res["replicas"], res["forwards"] = int(n), int(row[8] + row[10]), int(replicas), int(forwards)
    return res


def _check_faith_args(use, undirected, head, ratio, k, chunk):
    _check_topk(ratio, k, "faithfulness")
    return _check_driver_args(use, undirected, head, chunk)


def faithfulness(model, data, *, use: str = "edges", undirected=None, head: str = "o", ratio=None, k=None, elements=None,
                 chunk: int = 512) -> dict:
    """Do ``model``'s causal scores rank the elements of ``data`` as leave-one-out occlusion does?

    The causal score (column 1 of the soft masks; for edges symmetrised by ``undirected`` exactly as ``explain`` does it) is
    compared per graph with ``occlusion(model, data, use=..., undirected=..., head=..., elements=...)`` over the elements that
    were occluded (with ``undirected`` one representative per undirected edge) by one ``rank_agreement`` call:

    * ``rho``, ``tau``, ``jaccard``: the mean Spearman rho, Kendall tau-b and top-k Jaccard overlap (``ratio`` / ``k`` as
      ``explain`` takes them, counted over the elements taking part) over the graphs where each is defined;
    * ``rho_undefined``, ``tau_undefined``, ``jaccard_undefined``: the graphs where it is not (fewer than two elements, one of
      the two rankings constant, ``k_g = 0``);
    * ``occ_top`` / ``occ_rest``: the mean occlusion score of the occluded elements inside ``explain``'s top-k selection and of
      those outside it (high against low: what attention ranks first is what the prediction rests on);

    and ``graphs``, ``elements`` (occluded elements compared), ``replicas``, ``forwards``.  The cost is ``occlusion``'s plus one
    forward for the scores.  The sums stay on the device: the read-backs are the replica builder's and one at the end.  It
    leaves the model as ``occlusion`` does."""
    h, chunk = _check_faith_args(use, undirected, head, ratio, k, chunk)
    with _eval_mode(model):
        row, replicas, forwards, _ = _faith_sums(model, data, use, undirected, h, ratio, k, elements, chunk)
    return _faith_report(row.tolist(), replicas, forwards)


def eval_faithfulness(model, loader, device, *, use: str = "edges", undirected=None, head: str = "o", ratio=None, k=None,
                      chunk: int = 512) -> dict:
    """``faithfulness`` over a loader: the means taken over all graphs (and all occluded elements) of the loader.  The sums stay
    on the device until one read-back at the end (besides the replica builder's)."""
    h, chunk = _check_faith_args(use, undirected, head, ratio, k, chunk)
    sums = torch.zeros(_ROW, dtype=torch.float64, device=device)
    replicas = forwards = 0
    with _eval_mode(model):
        for data in loader:
            row, r, f, _ = _faith_sums(model, data.to(device), use, undirected, h, ratio, k, None, chunk)
            sums += row
            replicas, forwards = replicas + r, forwards + f
    return _faith_report(sums.tolist(), replicas, forwards)
