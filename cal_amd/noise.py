"""Structural noise: replicas of a batch's graphs with random edges deleted and inserted, the prediction under growing noise, and
how much of the causal explanation survives it.

CAL is meant to be robust to the trivial part of a graph, and SPMotif's own generator has a ``noise`` knob: ``int(noise |E|)``
random edges between distinct non-adjacent nodes (``spmotif.make_graph``).  Regenerating graphs on the host loses the pairing
with the clean graph that every comparison needs; here the noisy graph is built on the device from the clean one and carries
``edge_src``.

* ``noise_batch(data, rep_graph, add=..., delete=..., seed=...)`` -> ``Batch``: replica r is graph ``rep_graph[r]`` of ``data``
  with a Bernoulli subset of its edges deleted and an exact number of new edges inserted (``cal_noise_count`` /
  ``cal_noise_write``: two launches and one read-back of the totals on the GPU, libcalhost for CPU tensors), with the layout
  facts that keep the engine on its per-graph route.  ``degree_onehot(edge_index, N, F)``: SPMotif's node feature of a batch.
* ``noise_curve(model, data, add=(...))`` (also ``model.noise_curve``) / ``eval_noise_curve(model, loader, device, ...)``:
  accuracy, agreement with the clean prediction and ``p(ŷ_clean)`` at every noise level, on nested realisations.
* ``stability(model, data, add=...)`` (also ``model.stability``) / ``eval_stability(model, loader, device, ...)``: the causal
  edge ranking of the noisy replicas against the clean graph's, through ``rank_agreement``.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .explain import (_eval_forward, _eval_mode, _k_code, _Layout, _log_probs, _reduce_code, _scores, rank_segment_pairs,
                      rank_segments)
from .occlude import rank_agreement
from .plan import _p, _stream
from .replica import (_agree_report, _agree_sums, _built_batch, _caller_columns, _check_head, _check_replicas, _feature_width,
                      _grouped, _p_at, _pairs, _rebatch, _replica_log_probs, _representatives, _Source, _whole)

__all__ = ["noise_batch", "degree_onehot", "noise_curve", "eval_noise_curve", "stability", "eval_stability", "C_DEL", "C_ADD"]

#: the two stream constants of the operator (``CAL_NOISE_C_DEL`` / ``CAL_NOISE_C_ADD``)
C_DEL = 0xA0761D6478BD642F
C_ADD = 0xE7037ED1A0B428DB
_MAX63 = (1 << 63) - 1


def degree_onehot(edge_index: torch.Tensor, N: int, F: int) -> torch.Tensor:
    """float32 [N, F]: row i is zero except a 1 at ``min(d_i, F - 1)``, ``d_i`` the number of columns of ``edge_index`` that start
    at i and end elsewhere -- SPMotif's node feature (``cal_degree_onehot``: HIP for CUDA tensors, libcalhost for CPU tensors)."""
    if int(F) < 1:
        raise ValueError("degree features need F >= 1")
    ei = edge_index.to(torch.long).contiguous()
    host, E = not ei.is_cuda, int(ei.size(1))
    out = torch.empty(int(N), int(F), dtype=torch.float32, device=ei.device)
    _lib.call("cal_degree_onehot", _p(ei) if E else None, E, int(N), int(F), _p(out) if N else None, None if host else _stream(),
              host=host)
    return out


def _levels(v, R: int, dev, what: str):
    """``v`` (a float or a float tensor [R]) -> (fp64 tensor [R] or None, float or None).  A float is checked here, a tensor's
    entries by ``_check_entries``."""
    if torch.is_tensor(v):
        if v.dim() != 1 or int(v.numel()) != R or not v.dtype.is_floating_point:
            raise ValueError("%s must be a float or a float tensor with one entry per replica (%d)" % (what, R))
        return v.to(device=dev, dtype=torch.float64), None
    return None, _level(v, what)


def _level(v, what: str) -> float:
    v = float(v)
    if not (v >= 0.0 and math.isfinite(v)):
        raise ValueError("%s must be finite and >= 0" % what)
    return v


def _check_entries(named):
    """The smallest and the largest entry of every given level tensor in one read-back: all must be finite and >= 0 (a NaN
    entry makes both NaN).  -> {name: largest}."""
    named = [(what, t) for what, t in named if t is not None and t.numel()]
    if not named:
        return {}
    lims = torch.stack([torch.stack([t.min(), t.max()]) for _, t in named]).tolist()
    for (what, _), (lo, hi) in zip(named, lims):
        if not (lo >= 0.0 and math.isfinite(hi)):
            raise ValueError("%s must be finite and >= 0 in every entry" % what)
    return {what: hi for (what, _), (_, hi) in zip(named, lims)}


def _del_threshold(t, f, R: int, dev):
    """int64 [R]: ``floor(delete 2^63)`` clamped to ``[0, 2^63 - 1]``, ``delete`` the checked tensor ``t`` or the float ``f``."""
    if t is None:
        return torch.full((R,), min(int(math.floor(min(f, 1.0) * 2.0 ** 63)), _MAX63), dtype=torch.long, device=dev)
    big = 2.0 ** 63 - 1024.0                                              # the largest fp64 below 2^63
    th = (t * 2.0 ** 63).floor().clamp(max=big).long()
    return torch.where(t * 2.0 ** 63 >= 2.0 ** 63, torch.full_like(th, _MAX63), th)


def _seeds(seed, R: int, dev):
    if torch.is_tensor(seed):
        return _check_len(_pairs(seed, 0, dev, "seed"), R, "seed")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError("seed must be an int or an int64 [R] tensor")
    s = seed & ((1 << 64) - 1)
    s = s - (1 << 64) if s >= (1 << 63) else s                           # (as the operator reads it: 64 bits)
    return torch.full((R,), s, dtype=torch.long, device=dev) + torch.arange(R, device=dev)      # (int64 adds wrap)


def _check_len(t, R, what):
    if int(t.numel()) != R:
        raise ValueError("%s must have one entry per replica (%d)" % (what, R))
    return t


def _players(S, twin):
    """int64 [B]: every graph's players -- the columns that are no self loop, with ``twin`` one per undirected edge."""
    ok = S.ei[0] != S.ei[1]
    if twin is not None:
        ok = ok & _representatives(twin)
    gid = torch.repeat_interleave(torch.arange(S.B, device=S.dev), S.edge_ptr[1:] - S.edge_ptr[:-1], output_size=S.E)
    return torch.zeros(S.B, dtype=torch.long, device=S.dev).index_add_(0, gid, ok.long())


def _noise_build(S, F, twin, max_edges, rg, add, delete, seed, tries, features):
    """The operator's calls for the source ``S`` (``_Source``; ``twin`` int32 [E] over its columns or ``None``) -> ``Batch``."""
    dev, R = S.dev, int(rg.numel())
    if isinstance(tries, bool) or not isinstance(tries, int) or not 1 <= tries <= 1 << 20:
        raise ValueError("tries must be an int in [1, 2^20]")
    if features not in ("keep", "degree"):
        raise ValueError('features must be "keep" or "degree"')
    if features == "degree" and F < 1:
        raise ValueError('features="degree" needs F >= 1')
    (at, af), (dt, df) = _levels(add, R, dev, "add"), _levels(delete, R, dev, "delete")
    largest = _check_entries((("add", at), ("delete", dt)))             # (per-replica levels: one read-back)
    ok = (rg >= 0) & (rg < S.B)
    if S.B and S.E and R:
        U = _players(S, twin)[rg.clamp(0, S.B - 1)]
        lvl = at if at is not None else af
        radd = torch.where(ok, (U.double() * lvl).floor().long(), torch.zeros_like(rg))
    else:
        radd = torch.zeros(R, dtype=torch.long, device=dev)
    rdel, rseed = _del_threshold(dt, df, R, dev), _seeds(seed, R, dev)
    # the host-known bound on the candidates: a player is a column, so a <= floor(add max_edges) for every replica
    top = af if at is None else largest.get("add", 0.0)
    cand = R * tries * int(math.floor(top * max(int(max_edges), 0)))
    added = torch.zeros(max(R, 1), dtype=torch.long, device=dev)
    inputs = S.args() + [_p(twin) if twin is not None and S.E else None, _p(rg) if R else None, _p(rseed) if R else None,
                         _p(rdel) if R else None, _p(radd) if R else None, R, tries, _p(added)]
    built = _rebatch("cal_noise", (S.E, R, cand, tries), inputs, R, 7, (S,), F, lambda: ~ok)
    out = _built_batch(S, built, rg, S.no_self_loops, _caller_columns(S, built.edge_src, built.tot[1]))
    out.added, out.n_added, out.short = added[:R], int(built.tot[5]), int(built.tot[6])
    if features == "degree":
        x = degree_onehot(out.edge_index, int(built.tot[0]), F)
        out.x, out.feat = (x, None) if out.x is not None else (None, x)
    return out


def noise_batch(data, rep_graph=None, *, add=0.0, delete=0.0, seed=0, undirected: bool = True, tries: int = 8,
                features: str = "keep"):
    """``R`` noisy replicas of graphs of ``data``, as a ``cal_amd.data.Batch`` the engine can run.

    Replica r is graph ``rep_graph[r]`` (int64 [R], by default ``arange(B)``; an id outside the batch gives a replica with no
    node, counted in ``empty_graphs``).  The *players* of a graph are its edge columns that are no self loop; with
    ``undirected=True`` the twin map is built as ``occlusion`` does (``cal_edge_twin``) and a pair of twin columns is one player,
    represented by its lower column.  With ``U_g`` the players of graph g (counted on the device):

    * ``delete`` (a float, or a float tensor [R]): every player goes with that probability, independently -- the operator
      compares a 63-bit hash of (seed, the player's position in its graph) with ``floor(delete 2^63)`` clamped to
      ``[0, 2^63 - 1]``, so for one seed the deletions at a smaller ``delete`` are a subset of those at a larger one.  Both
      columns of an undirected edge go together; self loops stay.
    * ``add`` (likewise): exactly ``floor(add U_g)`` (taken in fp64) new edges between distinct nodes that are not adjacent in
      the *source* graph, drawn by bounded rejection from ``tries`` candidates per edge asked for; a replica that runs out of
      candidates (a near-complete graph) receives fewer and is counted in ``short``.  For one seed the edges inserted at a
      smaller count are a prefix of those at a larger one.  An inserted edge is one column ``(u, v)``, with ``undirected`` the two
      columns ``(u, v)``, ``(v, u)``; they follow the replica's surviving source columns, which keep their order.
    * ``seed``: an int s (replica r draws from ``s + r``) or an int64 tensor [R].  A replica depends on its own seed, graph and
      levels only, never on the others.

    ``features="keep"`` copies the source rows; ``"degree"`` overwrites them with the capped one-hot degree of the noisy graph
    (``cal_degree_onehot``), which is what SPMotif's node feature is.  The result carries what ``coalition_batch``'s does --
    ``x`` / ``feat``, ``edge_index``, ``batch``, ``ptr``, ``edge_ptr``, ``num_graphs = R``, ``max_nodes``, ``max_edges``,
    ``no_self_loops`` (inherited), no tiles, ``y = data.y[rep_graph]``, ``node_src`` / ``edge_src`` (``edge_src = -1`` for an
    inserted column), ``empty_graphs`` -- plus ``added`` (int64 [R] on the device: the insertions made) and the host ints
    ``n_added`` and ``short``.

    CUDA tensors: ``cal_noise_count`` and ``cal_noise_write`` on the current stream with one read-back of the totals between
    them (per-replica ``add`` / ``delete`` levels cost one more, of their extremes: every level must be finite and >= 0); CPU
    tensors: libcalhost.  Every integer output is uniquely determined and the same on both.  Inputs other than ``Batch`` objects get their layout derived as in ``coalition_batch``;
    edge columns that are not grouped by graph are put in stable graph order first and ``edge_src`` is mapped back."""
    S = _Source(data)
    F = _feature_width(S, "noise_batch")
    rg = _pairs(rep_graph, S.B, S.dev, "rep_graph")
    lay = _Layout(data)
    twin = lay.twins(data.edge_index)[0] if undirected else None
    return _noise_build(S, F, twin, lay.max_edges, rg, add, delete, seed, tries, features)


# ---- the pieces the drivers share ---------------------------------------------------------------------------------------------
class _Clean:
    """The clean batch as the drivers need it: the grouped source, its twin map (or ``None``), ŷ, ``p_full`` and C."""

    def __init__(self, model, data, h, undirected: bool):
        self.lay = _Layout(data)
        self.src = _grouped(data, self.lay)
        self.S = _Source(self.src)
        self.F = _feature_width(self.S, "noise_batch")
        self.twin = self.lay.twins(data.edge_index)[0] if undirected else None
        self.yhat, self.p_full, _ = _whole(model, self.src, h)
        self.B, self.dev = self.lay.B, self.S.dev

    def replicas(self, rg, add, delete, seeds, features):
        return _noise_build(self.S, self.F, self.twin, self.lay.max_edges, rg, add, delete, seeds, 8, features)


def _check_noise_args(head, trials, chunk, features):
    h = _check_head(head)
    trials, chunk = int(trials), int(chunk)
    if trials < 1 or chunk < 1:
        raise ValueError("trials and chunk must be >= 1")
    if features not in ("keep", "degree"):
        raise ValueError('features must be "keep" or "degree"')
    return h, trials, chunk


def _level_list(add, delete):
    seq = lambda v: [float(x) for x in v] if isinstance(v, (tuple, list)) else None
    a, d = seq(add), seq(delete)
    L = max(len(a) if a is not None else 1, len(d) if d is not None else 1)
    a = a if a is not None else [float(add)] * L
    d = d if d is not None else [float(delete)] * L
    if len(a) != L or len(d) != L or L == 0:
        raise ValueError("add and delete must be floats or sequences of one length")
    for v in a + d:
        _level(v, "add and delete")
    return a, d


def _curve_sums(model, data, h, adds, dels, trials, seed, features, undirected, chunk):
    """One batch's noise curve -> ``(per level [hits, agree, p] as [3, B] fp64 sums over the trials (hits NaN without labels),
    per level (replicas, forwards, added, short), _Clean)``.  Called in eval mode under no_grad."""
    cl = _Clean(model, data, h, undirected)
    B, dev = cl.B, cl.dev
    rg = torch.arange(B, device=dev).repeat(trials)
    seeds = _seeds(seed, trials * B, dev)                                # the same for every level: nested realisations
    y = None if cl.src.y is None else cl.src.y.view(-1).to(dev)
    sums, stats = [], []
    for a, d in zip(adds, dels):
        tab = torch.zeros(3, B, dtype=torch.float64, device=dev)
        forwards = added = short = 0
        for i in range(0, trials * B, chunk):
            g = rg[i:i + chunk]
            nb = cl.replicas(g, a, d, seeds[i:i + chunk], features)
            lp = _replica_log_probs(model, nb, h)                        # [R, C]
            pred = lp.argmax(-1)
            p = _p_at(lp, cl.yhat[g]).double()
            hit = (pred == y[g]).double() if y is not None else torch.full_like(p, float("nan"))
            tab.index_add_(1, g, torch.stack([hit, (pred == cl.yhat[g]).double(), p]))
            forwards, added, short = forwards + 1, added + nb.n_added, short + nb.short
        sums.append(tab)
        stats.append((trials * B, forwards, added, short))
    return sums, stats, cl


def _level_report(a, d, tab, n, stat, labels, per_graph):
    """``tab`` [3, B] sums over ``n`` replicas per graph (a tensor), or the three totals (a list) with ``per_graph`` False."""
    res = {"add": a, "delete": d}
    if per_graph:
        tot = tab.sum(1).tolist()
        B = int(tab.size(1))
        res["agree_graph"], res["p_graph"] = tab[1] / n, tab[2] / n
        if labels:
            res["acc_graph"] = tab[0] / n
        den = n * B
    else:
        tot, den = tab[:3], n
    nan = float("nan")
    if labels:
        res["acc"] = tot[0] / den if den else nan
    res["agree"], res["p"] = (tot[1] / den, tot[2] / den) if den else (nan, nan)
    res["replicas"], res["forwards"], res["added"], res["short"] = stat
    return res


def noise_curve(model, data, *, add=(0.0, 0.1, 0.2, 0.4), delete=0.0, trials: int = 4, seed: int = 0, head: str = "o",
                features: str = "keep", undirected: bool = True, chunk: int = 512) -> dict:
    """``model``'s prediction on ``data`` under growing structural noise.

    ``add`` / ``delete``: a float or a sequence of levels (a float is repeated; two sequences pair up).  One eval forward of the
    whole batch (untiled, the route the replicas take) gives ŷ_g, the argmax of ``head``, and ``p_full``.  Per level,
    ``trials`` noisy replicas of every graph (``noise_batch``: replica t B + g is graph g under seed ``seed + t B + g``) run in
    chunks of at most ``chunk`` graphs, one builder call and one forward each.  The same seeds serve every level, so the
    realisations of the curve are nested: a higher level adds edges to, and deletes edges from, the lower level's graph.

    Returns ``p_full`` [B], ``yhat`` int64 [B], ``forwards`` (all levels and the whole batch's) and ``levels``, one dict per
    level: ``add``, ``delete``, ``acc`` (against ``data.y``; absent without labels), ``agree`` (the share of replicas whose
    argmax is ŷ_g), ``p`` (the mean ``p(ŷ_g)``), the per-graph means over the trials ``acc_graph`` / ``agree_graph`` /
    ``p_graph`` (fp64 [B] on ``data``'s device), ``replicas``, ``forwards``, ``added`` (edges inserted) and ``short`` (replicas
    that received fewer than asked).  ``features`` / ``undirected`` as in ``noise_batch``.  Like ``explain``, it runs in eval mode
    under ``no_grad`` and leaves parameters, optimizer state, the engine's step counter, BatchNorm statistics, the RNG states
    and ``model.training`` as they were."""
    h, trials, chunk = _check_noise_args(head, trials, chunk, features)
    adds, dels = _level_list(add, delete)
    with _eval_mode(model):
        sums, stats, cl = _curve_sums(model, data, h, adds, dels, trials, seed, features, bool(undirected), chunk)
        labels = cl.src.y is not None
        levels = [_level_report(a, d, t, trials, s, labels, True) for a, d, t, s in zip(adds, dels, sums, stats)]
    return {"levels": levels, "p_full": cl.p_full, "yhat": cl.yhat, "forwards": 1 + sum(s[1] for s in stats)}


def eval_noise_curve(model, loader, device, *, add=(0.0, 0.1, 0.2, 0.4), delete=0.0, trials: int = 4, seed: int = 0,
                     head: str = "o", features: str = "keep", undirected: bool = True, chunk: int = 512) -> dict:
    """``noise_curve`` over a loader: ``levels`` with ``acc``, ``agree``, ``p`` taken over all replicas of the loader and the
    summed ``replicas``, ``forwards``, ``added``, ``short``; ``graphs`` and ``forwards``.  Mini-batch b draws from the seeds that
    follow mini-batch b - 1's.  The sums stay on the device until one read-back at the end (besides the replica builder's)."""
    h, trials, chunk = _check_noise_args(head, trials, chunk, features)
    adds, dels = _level_list(add, delete)
    L = len(adds)
    tot = torch.zeros(L, 3, dtype=torch.float64, device=device)
    stat = [[0, 0, 0, 0] for _ in range(L)]
    graphs = batches = 0
    with _eval_mode(model):
        for data in loader:
            batches += 1
            sums, stats, cl = _curve_sums(model, data.to(device), h, adds, dels, trials, seed + trials * graphs, features,
                                          bool(undirected), chunk)
            tot += torch.stack([t.sum(1) for t in sums])
            stat = [[u + v for u, v in zip(s, st)] for s, st in zip(stat, stats)]
            graphs += cl.B
    rows = tot.tolist()
    labels = not any(math.isnan(r[0]) for r in rows)
    levels = [_level_report(a, d, r, s[0], tuple(s), labels, False) for a, d, r, s in zip(adds, dels, rows, stat)]
    return {"levels": levels, "graphs": graphs, "forwards": batches + sum(s[1] for s in stat)}


# ---- explanation stability ----------------------------------------------------------------------------------------------------
_SROW = 17          # the three figures' sums, then the replicas where each is defined (_agree_sums); replicas; flips; sum of dp;
#                     inserted edges in the top-k and inserted edges; precision sums and counts (clean, noisy); elements compared;
#                     clean graphs


def _scores_and_log_probs(model, data):
    """One eval forward -> (edge scores [E] (a copy), log-probabilities [3, R, C])."""
    eng = _eval_forward(model, data)
    if eng is None:
        return _scores(model, data)[0].clone(), _log_probs(model, data)
    return eng.attention_scores(data)[0].clone(), torch.stack(eng.logp_copy())


def _ranked(score, seg, max_seg, twin, undirected, ratio, k, gt):
    """``explain``'s edge ranking over grouped columns -> (top-k mask, metrics or None, the score as ranked)."""
    if twin is None:
        top, _, met = rank_segments(score, seg, max_seg, ratio=ratio, k=k, gt=gt, metrics=gt is not None)
        return top, met, score
    top, _, met, sym = rank_segment_pairs(score, seg, max_seg, twin, undirected, ratio=ratio, k=k, gt=gt, metrics=gt is not None)
    return top, met, sym


def _precision(met, dev):
    """(sum of hits / k_g over the graphs with k_g > 0, their number) of a metrics tensor, zeros without one."""
    if met is None:
        return torch.zeros(2, dtype=torch.float64, device=dev)
    kg, hits = met[:, 0], met[:, 1]
    ok = kg > 0
    return torch.stack([torch.where(ok, hits / torch.where(ok, kg, torch.ones_like(kg)), torch.zeros_like(kg)).sum(), ok.sum().double()])


def _stability_sums(model, data, h, add, delete, trials, seed, ratio, k, undirected, edge_gt, features, chunk):
    """One batch's sums [_SROW] fp64 on the device and (replicas, forwards, added, short).  Called in eval mode under no_grad."""
    clean = _scores(model, data)[0].clone()
    cl = _Clean(model, data, h, undirected is not None)
    lay, dev, B = cl.lay, cl.dev, cl.B
    gt = None
    if edge_gt is not None:
        gt = edge_gt.to(device=dev, dtype=torch.bool)
        gt = gt if lay.order is None else gt[lay.order]
    if lay.order is not None:
        clean = clean[lay.order].contiguous()
    _, met0, clean = _ranked(clean, lay.edge_ptr, lay.max_edges, cl.twin, undirected, ratio, k, gt)
    rg = torch.arange(B, device=dev).repeat(trials)
    seeds = _seeds(seed, trials * B, dev)
    row = torch.zeros(_SROW, dtype=torch.float64, device=dev)
    row[11:13] = _precision(met0, dev)
    row[16] = float(B)
    forwards, added, short = 2, 0, 0
    for i in range(0, trials * B, chunk):
        g = rg[i:i + chunk]
        nb = cl.replicas(g, add, delete, seeds[i:i + chunk], features)
        _check_replicas(nb)
        noisy, lp = _scores_and_log_probs(model, nb)
        E2 = int(nb.edge_index.size(1))
        survivor = nb.edge_src >= 0
        src_col = nb.edge_src.clamp(min=0)
        twin2, rep2 = None, torch.ones(E2, dtype=torch.bool, device=dev)
        if cl.twin is not None:
            twin2 = _Layout(nb).twins(nb.edge_index)[0]
            rep2 = _representatives(twin2)
        gt2 = None if gt is None else gt[src_col] & survivor            # an inserted edge is never ground truth
        top2, met2, noisy = _ranked(noisy, nb.edge_ptr, nb.max_edges, twin2, undirected, ratio, k, gt2)
        a = clean[src_col] if cl.S.E else noisy
        _, met = rank_agreement(a, noisy, nb.edge_ptr, nb.max_edges, sel=survivor & rep2, ratio=ratio, k=k)
        ins = ~survivor & rep2
        lph = lp[h]
        pred = lph.argmax(-1)
        p = _p_at(lph, cl.yhat[g])
        row[:6] += _agree_sums(met)
        row[6:11] += torch.stack([torch.as_tensor(float(g.numel()), dtype=torch.float64, device=dev), (pred != cl.yhat[g]).sum().double(),
                                  (cl.p_full[g] - p).double().sum(), (ins & top2).sum().double(), ins.sum().double()])
        row[13:15] += _precision(met2, dev)
        row[15] += (survivor & rep2).sum().double()
        forwards, added, short = forwards + 1, added + nb.n_added, short + nb.short
    return row, (trials * B, forwards, added, short)


def _stability_report(row, stat, with_gt) -> dict:
    nan = float("nan")
    n = row[6]
    res = _agree_report(row[:6], n)
    res["flip"], res["dp"] = (row[7] / n, row[8] / n) if n else (nan, nan)
    res["noise_in_top"] = row[9] / row[10] if row[10] else 0.0
    if with_gt:
        res["precision_clean"] = row[11] / row[12] if row[12] else nan
        res["precision_noisy"] = row[13] / row[14] if row[14] else nan
    res["graphs"], res["elements"] = int(row[16]), int(row[15])
    res["replicas"], res["forwards"], res["added"], res["short"] = stat
    return res


def _check_stability_args(ratio, k, undirected, head, trials, chunk, features, add, delete):
    _k_code(ratio, k)
    if k == "gt":
        raise ValueError('stability compares two rankings at one k: k must be an int >= 0')
    _reduce_code(undirected)
    for v in (add, delete):
        _level(v, "add and delete")
    return _check_noise_args(head, trials, chunk, features)


def stability(model, data, *, add: float = 0.1, delete: float = 0.0, trials: int = 4, seed: int = 0, ratio=None, k=None,
              undirected="mean", head: str = "o", edge_gt=None, features: str = "keep", chunk: int = 512) -> dict:
    """Does ``model``'s causal explanation of ``data`` survive structural noise?

    The causal edge scores come as ``explain`` obtains them (column 1 of the soft masks, symmetrised by ``undirected`` =
    ``"mean"`` / ``"max"`` / ``"min"``; ``None``: every column on its own, and the noise is directed as well) on the clean batch
    and on ``trials`` noisy replicas of every graph (``noise_batch`` at ``add`` / ``delete``, seeds ``seed + t B + g``), in
    chunks of at most ``chunk`` graphs, one builder call and one forward each.  On a replica every surviving column e'
    (``edge_src >= 0``) carries the clean score ``a[e'] = s_clean[edge_src[e']]`` and its own ``b[e'] = s_noisy[e']``; one
    ``rank_agreement`` call per chunk over the surviving undirected edges (one representative each) gives

    * ``rho``, ``tau``, ``jaccard``: the mean Spearman rho, Kendall tau-b and top-k Jaccard overlap (``ratio`` / ``k`` as
      ``explain`` takes them, counted over the survivors) over the replicas where each is defined, and ``rho_undefined``,
      ``tau_undefined``, ``jaccard_undefined``: the replicas where it is not -- the shape of ``faithfulness``;
    * ``noise_in_top``: the share of inserted edges that ``explain``'s top-k selection on the noisy graph picks up (0 when
      nothing was inserted);
    * ``flip``: the share of replicas whose argmax at ``head`` differs from the clean graph's, ``dp``: the mean
      ``p_full(ŷ_g) - p_noisy(ŷ_g)``;
    * with ``edge_gt`` (bool [E]): ``precision_clean`` / ``precision_noisy``, precision@k against the ground truth on the clean
      batch and on the replicas, where a survivor inherits its source column's truth and an inserted edge is never true;

    and ``graphs``, ``elements`` (survivors compared), ``replicas``, ``forwards`` (the two of the clean batch included),
    ``added``, ``short``.  The sums stay on the device: the read-backs are the replica builder's and one at the end.  It leaves
    the model as ``explain`` does."""
    h, trials, chunk = _check_stability_args(ratio, k, undirected, head, trials, chunk, features, add, delete)
    with _eval_mode(model):
        row, stat = _stability_sums(model, data, h, float(add), float(delete), trials, seed, ratio, k, undirected, edge_gt,
                                    features, chunk)
    return _stability_report(row.tolist(), stat, edge_gt is not None)


def eval_stability(model, loader, device, *, add: float = 0.1, delete: float = 0.0, trials: int = 4, seed: int = 0, ratio=None,
                   k=None, undirected="mean", head: str = "o", features: str = "keep", chunk: int = 512) -> dict:
    """``stability`` over a loader of SPMotif graphs, with ``spmotif.ground_truth`` as the ground truth: the means taken over all
    replicas of the loader.  Mini-batch b draws from the seeds that follow mini-batch b - 1's.  The sums stay on the device
    until one read-back at the end (besides the replica builder's)."""
    from .spmotif import ground_truth
    h, trials, chunk = _check_stability_args(ratio, k, undirected, head, trials, chunk, features, add, delete)
    sums = torch.zeros(_SROW, dtype=torch.float64, device=device)
    stat, graphs = (0, 0, 0, 0), 0
    with _eval_mode(model):
        for data in loader:
            data = data.to(device)
            row, st = _stability_sums(model, data, h, float(add), float(delete), trials, seed + trials * graphs, ratio, k,
                                      undirected, ground_truth(data)[1], features, chunk)
            graphs += int(data.num_graphs)
            sums += row
            stat = tuple(u + v for u, v in zip(stat, st))
    return _stability_report(sums.tolist(), stat, True)
