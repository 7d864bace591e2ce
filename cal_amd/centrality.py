"""Graph centralities on the GPU, and what they are for here: the structure-only baselines of the explanations.

An SPMotif graph is a motif hung on a BA tree by one bridge, so a ranking that has never seen the model -- by degree, betweenness,
closeness or PageRank -- may already separate motif edges from base edges.  This module measures that null hypothesis:

* ``centrality(data, alpha=0.85, tol=1e-12, max_iter=1000, sources=None)`` -> ``Centrality``: hop distances (farness, reach,
  eccentricity), Brandes' node and edge betweenness, PageRank and the distinct degree of every graph of a batch
  (``cal_centrality``: one launch on the GPU, one workgroup per graph of at most 256 nodes; libcalhost, without that limit, for CPU
  tensors; the definitions are in ``include/cal_hip.h``).  ``hop_distance(data, sources)``: only the distance to a marked set.
* ``structural_scores(data, kind)``: one float32 score per edge column or node from a centrality.
* ``structural_baseline`` / ``eval_structural_baseline`` (also ``model.structural_baseline``): precision@k, recall@k and ROC-AUC
  of every structural ranking against the planted motif next to the causal attention's, the attention's rank agreement with
  each of them, and ``chance``.
* ``explanation_locality`` / ``eval_explanation_locality``: how far from the motif the edges of an explanation lie.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from .explain import _accumulate, _eval_mode, _KEYS, _keep8, _k_code, _Layout, explain, rank_segment_pairs, rank_segments
from .plan import _p, _stream
from .replica import _agree_report, _agree_sums, _causal_in_order, _check_driver_args, _representatives

__all__ = ["Centrality", "centrality", "hop_distance", "structural_scores", "structural_baseline", "eval_structural_baseline",
           "explanation_locality", "eval_explanation_locality", "KINDS", "MAX_NODES", "LDS_COLS"]

#: the largest graph the device operator takes (``CAL_MOTIF_MAX_NODES``); columns of a graph whose edge-betweenness partials fit
#: in LDS (``CAL_CENTRALITY_LDS_COLS``)
MAX_NODES = 256
LDS_COLS = 768
KINDS = ("degree", "closeness", "betweenness", "pagerank", "edge_betweenness")

_Raw = namedtuple("_Raw", "far reach ecc deg bc ebc pr pr_iters hop skipped ignored nodes edge_nodes")


class Centrality(_Raw):
    """The raw outputs of ``cal_centrality`` (``include/cal_hip.h``): ``far`` / ``reach`` / ``ecc`` / ``deg`` int64 [N], ``bc``
    fp64 [N] and ``ebc`` fp64 [E] (RAW: twice networkx's unnormalised values; ``ebc`` per edge column in the caller's order),
    ``pr`` fp64 [N], ``pr_iters`` int32 [B], ``hop`` int32 [N] or ``None``, ``skipped`` int64 [B] (graphs above 256 nodes on the
    device: -1 / NaN everywhere), ``ignored`` int64 [1] (columns that leave their graph); and ``nodes`` int64 [N] / ``edge_nodes``
    int64 [E]: the node count of the element's graph.  The methods form the published quantities in fp64 on the tensors' device,
    without a synchronisation; a skipped graph's are NaN."""
    __slots__ = ()

    def _guard(self, t, n_of):
        return torch.where(n_of < 0, torch.full_like(t, float("nan")), t)

    def closeness(self):
        """Wasserman-Faust closeness as networkx: ``((reach - 1) / far) * ((reach - 1) / (n - 1))``, 0 where ``far == 0``."""
        r = (self.reach - 1).double()
        far, n1 = self.far.double(), (self.nodes - 1).double()
        c = torch.where(self.far > 0, (r / far.clamp(min=1.0)) * (r / n1.clamp(min=1.0)), torch.zeros_like(r))
        return self._guard(c, self.far)

    def betweenness(self, normalized: bool = True):
        """``raw / ((n - 1)(n - 2))`` for n > 2 (``normalized``), otherwise ``raw / 2``: networkx's ``betweenness_centrality``."""
        n = self.nodes.double()
        if not normalized:
            return self.bc / 2.0
        return torch.where(self.nodes > 2, self.bc / ((n - 1.0) * (n - 2.0)).clamp(min=1.0), self.bc / 2.0)

    def edge_betweenness(self, normalized: bool = True):
        """``raw / (n (n - 1))`` (``normalized``), otherwise ``raw / 2``, per edge column: networkx's ``edge_betweenness_centrality``."""
        n = self.edge_nodes.double()
        if not normalized:
            return self.ebc / 2.0
        return torch.where(self.edge_nodes > 1, self.ebc / (n * (n - 1.0)).clamp(min=1.0), self.ebc / 2.0)

    def degree(self):
        """The distinct neighbours of every node, fp64 (NaN in a skipped graph)."""
        return self._guard(self.deg.double(), self.deg)

    @property
    def pagerank(self):
        return self.pr


def _run(data, alpha, tol, max_iter, sources, want_cent: bool):
    ei = data.edge_index
    dev, host = ei.device, not ei.is_cuda
    lay = _Layout(data)
    if lay.order is not None:
        ei = ei[:, lay.order]
    ei = ei.to(torch.long).contiguous()
    N, E, B = int(data.batch.numel()), int(ei.size(1)), lay.B
    ptr, eptr = lay.ptr.to(torch.long).contiguous(), lay.edge_ptr.to(torch.long).contiguous()
    alpha, tol, max_iter = float(alpha), float(tol), int(max_iter)
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha must be in [0, 1)")
    if not tol >= 0.0 or max_iter < 0:
        raise ValueError("tol and max_iter must be >= 0")
    s8 = None if sources is None else _keep8(sources, N, dev, "sources")
    hop = torch.empty(N, dtype=torch.int32, device=dev) if s8 is not None else None
    if not want_cent and hop is None:
        raise ValueError("hop_distance needs sources")
    nodes = ptr[1:] - ptr[:-1]
    ints = torch.empty(4 * N + B + 1 if want_cent else B + 1, dtype=torch.long, device=dev)
    far = reach = ecc = deg = bc = ebc = pr = iters = ws = None
    wsb = 0
    if want_cent:
        far, reach, ecc, deg, skipped, ignored = torch.split(ints, (N, N, N, N, B, 1))
        f64 = torch.empty(2 * N + E, dtype=torch.float64, device=dev)
        bc, pr, ebc = torch.split(f64, (N, N, E))
        iters = torch.empty(B, dtype=torch.int32, device=dev)
        wsb = _lib.query("cal_centrality_ws", E, host=host)
        ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev) if wsb else None
    else:
        skipped, ignored = torch.split(ints, (B, 1))
    _lib.call("cal_centrality", _p(ei) if E else None, E, N, _p(ptr), _p(eptr), B, _p(s8) if s8 is not None and N else None,
              alpha, tol, max_iter, _p(far), _p(reach), _p(ecc), _p(deg), _p(bc), _p(ebc) if E else None, _p(pr), _p(iters),
              _p(hop), _p(skipped), _p(ignored), _p(ws), wsb, None if host else _stream(), host=host)
    enodes = torch.repeat_interleave(nodes, eptr[1:] - eptr[:-1], output_size=E)
    if want_cent and lay.order is not None:                              # back to the caller's column order
        back = torch.empty_like(ebc)
        back[lay.order] = ebc
        ebc = back
        eb = torch.empty_like(enodes)
        eb[lay.order] = enodes
        enodes = eb
    nn = torch.repeat_interleave(nodes, nodes, output_size=N)
    return Centrality(far, reach, ecc, deg, bc, ebc, pr, iters, hop, skipped, ignored, nn, enodes)


def centrality(data, *, alpha: float = 0.85, tol: float = 1e-12, max_iter: int = 1000, sources=None) -> Centrality:
    """The centralities of every graph of ``data`` (``cal_centrality``; the definitions and the order of every sum are in
    ``include/cal_hip.h``).

    The graphs are read as simple undirected graphs, as ``motif_match`` reads them (a column in either direction makes its ends
    adjacent; self loops and duplicates add nothing; a column that leaves its graph is counted in ``ignored``).  PageRank uses
    ``alpha``, uniform teleport and start, dangling nodes spread uniformly, and stops when the L1 change is below ``tol`` (or
    after ``max_iter`` steps).  ``sources`` (a mask [N]) also asks for ``hop``, the distance to the nearest marked node of the
    same graph (-1: none within reach).  A batch whose columns are not grouped by graph is reordered by graph first.  CUDA
    tensors: one launch on the current stream, no read-back, graphs above 256 nodes skipped; CPU tensors: libcalhost, any size.
    Integers agree bit for bit between the two; fp64 is deterministic on each."""
    return _run(data, alpha, tol, max_iter, sources, True)


def hop_distance(data, sources) -> torch.Tensor:
    """int32 [N]: every node's hop distance to the nearest node of its graph marked in ``sources`` (a mask [N]); 0 on a marked
    node, -1 where none is within reach (and in a skipped graph).  The same launch as ``centrality``, with only ``hop`` wanted."""
    if sources is None:
        raise ValueError("hop_distance needs sources")
    return _run(data, 0.85, 0.0, 0, sources, False).hop


# ---- structure-only scores --------------------------------------------------------------------------------------------------------
def _split_kind(kind):
    if not isinstance(kind, str):
        raise TypeError("kind must be a string")
    asc = kind.startswith("-")
    name = kind[1:] if asc else kind
    if name not in KINDS:
        raise ValueError("kind must be one of %s, with an optional leading '-'" % ", ".join(KINDS))
    return name, asc


def _scores_of(c: Centrality, data, kind, use):
    name, asc = _split_kind(kind)
    if name == "edge_betweenness":
        if use != "edges":
            raise ValueError('"edge_betweenness" scores edges: use="edges"')
        s = c.edge_betweenness()
    else:
        s = {"degree": c.degree, "closeness": c.closeness, "betweenness": c.betweenness, "pagerank": lambda: c.pr}[name]()
        if use == "edges":
            N = int(s.numel())
            ei = data.edge_index.long()
            ok = (ei >= 0) & (ei < N)
            ends = s[ei.clamp(0, max(N - 1, 0))] if N else torch.zeros_like(ei, dtype=torch.float64)
            s = torch.where(ok[0] & ok[1], (ends[0] + ends[1]) * 0.5, torch.full_like(ends[0], float("nan")))
    return (-s if asc else s).float()


def structural_scores(data, kind: str, *, use: str = "edges", cent: Centrality = None) -> torch.Tensor:
    """float32 [E] (``use="edges"``) or [N] (``"nodes"``): a score that has never seen a model.  ``kind``: ``"degree"``,
    ``"closeness"``, ``"betweenness"``, ``"pagerank"`` (networkx's normalised forms, in fp64, then cast) or
    ``"edge_betweenness"`` (edges only); a leading ``"-"`` asks for the ascending orientation (the score negated).  For edges a
    node kind scores a column by the mean of its two end nodes.  ``cent``: a ``centrality(data)`` already at hand."""
    if use not in ("nodes", "edges"):
        raise ValueError('use must be "nodes" or "edges"')
    _split_kind(kind)
    return _scores_of(centrality(data) if cent is None else cent, data, kind, use)


# ---- baselines --------------------------------------------------------------------------------------------------------------------
_NK = len(_KEYS)        # precision, recall, auc


def _default_kinds(use):
    return KINDS if use == "edges" else KINDS[:4]


def _check_baseline(kinds, use, undirected, k, ratio):
    _check_driver_args(use, undirected, "o", 1)
    if ratio is not None:
        k = None
    kc, _ = _k_code(ratio, k)
    kinds = tuple(_default_kinds(use) if kinds is None else kinds)
    for kd in kinds:
        if _split_kind(kd)[0] == "edge_betweenness" and use != "edges":
            raise ValueError('"edge_betweenness" scores edges: use="edges"')
    return kinds, k, kc


def _baseline_sums(model, data, kinds, use, undirected, k, ratio, kc):
    """One batch's sums on the device, fp64 [(1 + K) * 6 + K * 6 + 3]: per ranking (the attention first) ``_accumulate``'s six,
    per kind ``_agree_sums``' six, then graphs, ground-truth elements, elements.  Called in eval mode under no_grad."""
    from .spmotif import ground_truth
    causal, lay = _causal_in_order(model, data, use)
    node_gt, edge_gt = ground_truth(data)
    cen = centrality(data)
    dev = causal.device
    sel = twin = None
    if use == "edges":
        gt = edge_gt if lay.order is None else edge_gt[lay.order]
        seg, max_seg = lay.edge_ptr, lay.max_edges
        if undirected is not None:
            twin = lay.twins(data.edge_index)[0]
            sel = _representatives(twin)
    else:
        gt, seg, max_seg = node_gt, lay.ptr, lay.max_nodes

    def ranked(score):
        """-> (the metrics [B, 4], the score the ranking used, its top-k mask)"""
        if twin is None:
            mask, _, met = rank_segments(score, seg, max_seg, ratio=ratio, k=k, gt=gt, metrics=True)
            return met, score, mask
        mask, _, met, sym = rank_segment_pairs(score, seg, max_seg, twin, undirected, ratio=ratio, k=k, gt=gt, metrics=True)
        return met, sym, mask

    from .occlude import rank_agreement
    K = len(kinds)
    sums = torch.zeros((1 + K) * 6 + K * 6 + 3, dtype=torch.float64, device=dev)
    met, causal, top = ranked(causal.contiguous())
    _accumulate(sums, met, 0)
    P, kg = met[:, 2], met[:, 0]
    gid = torch.repeat_interleave(torch.arange(lay.B, device=dev), seg[1:] - seg[:-1], output_size=int(gt.numel()))
    one = torch.ones_like(top) if sel is None else sel

    def per_graph(mask):
        return met.new_zeros(lay.B).index_add_(0, gid, mask.double())
    for i, kd in enumerate(kinds):
        s = _scores_of(cen, data, kd, use)
        if use == "edges" and lay.order is not None:
            s = s[lay.order]
        smet, s, stop = ranked(s.contiguous())
        _accumulate(sums, smet, 6 * (1 + i))
        if kc == -2:        # rank_agreement has no ground truth: rho and tau from it, the overlap from the two selections made
            agree = rank_agreement(causal, s, seg, max_seg, sel=sel, k=0)[1]
            inter = per_graph(top & stop & one)
            agree[:, 2] = torch.where(kg > 0, inter / (2.0 * kg - inter).clamp(min=1.0), torch.full_like(kg, float("nan")))
        else:
            agree = rank_agreement(causal, s, seg, max_seg, sel=sel, ratio=ratio, k=k)[1]
        sums[(1 + K) * 6 + 6 * i:(1 + K) * 6 + 6 * i + 6] = _agree_sums(agree)
    # chance: per graph P / m over the elements ranked (pairs with `undirected`), summed over the graphs that have an element
    m = per_graph(one)
    has = m > 0
    sums[-3] = has.sum()
    sums[-2] = torch.where(has, P / m.clamp(min=1.0), torch.zeros_like(P)).sum()
    sums[-1] = float(lay.B)
    return sums


def _baseline_report(row, kinds) -> dict:
    K = len(kinds)

    def prf(off):
        return {key: (row[off + 2 * i] / row[off + 2 * i + 1] if row[off + 2 * i + 1] else float("nan")) for i, key in enumerate(_KEYS)}
    B = int(row[-1])
    res = {"graphs": B, "chance": row[-2] / row[-3] if row[-3] else float("nan"), "attention": prf(0), "kinds": {}}
    for i, kd in enumerate(kinds):
        d = prf(6 * (1 + i))
        d.update(_agree_report(row[(1 + K) * 6 + 6 * i:(1 + K) * 6 + 6 * i + 6], B))
        res["kinds"][kd] = d
    return res


def structural_baseline(model, data, *, kinds=None, use: str = "edges", undirected="mean", k="gt", ratio=None) -> dict:
    """How much of the causal attention's score against the planted motif does the graph's geometry give for free?

    For every ``kind`` (``structural_scores``; by default all five for edges, the four node kinds for nodes) and for the model's
    causal attention: mean ``precision`` @k, ``recall`` @k and ROC-``auc`` against ``spmotif.ground_truth`` through the ranking
    launch ``explain`` uses (``k="gt"``: as many elements as the graph's motif has; or an int, or ``ratio``; with ``undirected``,
    the default, undirected edges are ranked under that reduction exactly as ``explain`` does).  Per kind also ``rho``, ``tau``,
    ``jaccard`` (+ ``_undefined``): the attention's rank agreement with that kind (``rank_agreement``; the overlap is that of
    the two top-k selections, under ``k="gt"`` the two selections of the motif's size).  ``chance``: the mean share of ground-truth elements, what a random
    ranking's precision@k converges to.  Returns ``{"graphs", "chance", "attention": {...}, "kinds": {kind: {...}}}``.  One
    forward, one ``cal_centrality`` launch, two ranking launches per kind; one read-back at the end.  Leaves the model as
    ``explain`` does."""
    kinds, k, kc = _check_baseline(kinds, use, undirected, k, ratio)
    with _eval_mode(model):
        row = _baseline_sums(model, data, kinds, use, undirected, k, ratio, kc).tolist()
    return _baseline_report(row, kinds)


def eval_structural_baseline(model, loader, device, *, kinds=None, use: str = "edges", undirected="mean", k="gt", ratio=None) -> dict:
    """``structural_baseline`` over a loader: the means over all graphs of the loader.  The sums stay on the device until one
    read-back at the end."""
    kinds, k, kc = _check_baseline(kinds, use, undirected, k, ratio)
    sums = None
    with _eval_mode(model):
        for data in loader:
            row = _baseline_sums(model, data.to(device), kinds, use, undirected, k, ratio, kc)
            sums = row if sums is None else sums + row
    if sums is None:
        sums = torch.zeros((1 + len(kinds)) * 6 + len(kinds) * 6 + 3, dtype=torch.float64)
    return _baseline_report(sums.tolist(), kinds)


# ---- locality ---------------------------------------------------------------------------------------------------------------------
_LROW = 8          # selected edges; in the motif; at distance 0, 1, 2, >= 3; wrong edges; the sum of their distances


def _locality_sums(model, data, ratio, k, undirected):
    from .spmotif import ground_truth
    node_gt, edge_gt = ground_truth(data)
    ex = explain(model, data, ratio=ratio, k=k, undirected=undirected, edge_gt=edge_gt, node_gt=node_gt)
    hop = hop_distance(data, node_gt).long()
    ei = data.edge_index.long()
    N = int(hop.numel())
    ok = ((ei >= 0) & (ei < N)).all(0)
    ends = hop[ei.clamp(0, max(N - 1, 0))] if N else ei
    big = torch.full_like(ends, 1 << 30)
    d = torch.where(ends < 0, big, ends).min(0).values                   # the smaller of the two ends' (-1: unreachable)
    sel = ex.edge_mask & ok
    if ex.edge_twin is not None:                                         # one column per undirected edge
        tw = ex.edge_twin.long()
        sel = sel & ~((tw >= 0) & (tw < torch.arange(tw.numel(), device=tw.device)))
    gt = edge_gt.to(sel.device)
    if ex.edge_twin is not None:
        tw = ex.edge_twin.long()
        gt = gt | (gt[tw.clamp(min=0)] & (tw >= 0))
    wrong = sel & ~gt
    fin = d < (1 << 30)
    dd = d.double()
    return torch.stack([sel.sum(), (sel & gt).sum(), (sel & (d == 0)).sum(), (sel & (d == 1)).sum(), (sel & (d == 2)).sum(),
                        (sel & (d >= 3)).sum(), (wrong & fin).sum(),
                        torch.where(wrong & fin, dd, torch.zeros_like(dd)).sum()]).double()


def _locality_report(row) -> dict:
    n = row[0]

    def share(x):
        return x / n if n else float("nan")
    return {"edges": int(n), "in_motif": share(row[1]), "hop0": share(row[2]), "hop1": share(row[3]), "hop2": share(row[4]),
            "hop3plus": share(row[5]), "wrong": int(n - row[1]), "wrong_mean_hop": row[7] / row[6] if row[6] else float("nan")}


def explanation_locality(model, data, *, ratio=None, k=None, undirected="mean") -> dict:
    """Do the explainer's mistakes hug the motif or scatter over the base?

    Takes the selected edges of ``explain(model, data, ratio / k, undirected)`` (with ``undirected`` one per undirected edge;
    ``k="gt"`` ranks against ``spmotif.ground_truth``) and every edge's hop distance to the motif: the smaller of its two ends'
    ``hop_distance`` with ``sources`` = the ground-truth nodes.  Returns ``edges`` (selected), ``in_motif`` (the share that are
    ground truth), ``hop0`` / ``hop1`` / ``hop2`` / ``hop3plus`` (the shares at that distance; an edge that cannot reach the motif
    counts as ``hop3plus``), ``wrong`` (selected edges that are not ground truth) and ``wrong_mean_hop`` (their mean distance,
    over those that reach the motif).  One ``explain``, one launch for the distances, one read-back."""
    _k_code(ratio, k)
    return _locality_report(_locality_sums(model, data, ratio, k, undirected).tolist())


def eval_explanation_locality(model, loader, device, *, ratio=None, k="gt", undirected="mean") -> dict:
    """``explanation_locality`` over a loader: the shares over all selected edges of the loader; one read-back at the end."""
    if ratio is not None:
        k = None
    _k_code(ratio, k)
    sums = torch.zeros(_LROW, dtype=torch.float64, device=device)
    for data in loader:
        sums += _locality_sums(model, data.to(device), ratio, k, undirected)
    return _locality_report(sums.tolist())
