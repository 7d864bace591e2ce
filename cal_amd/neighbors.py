"""Nearest neighbours in embedding space: example-based explanations and a non-parametric probe of CAL's split.

CAL's claim is about representations: the pooled objects row ``xo`` should carry the motif (the label), the pooled trivial row
``xc`` the base graph (the bias of the SPMotif split).  ``pooled_representations`` (intervene.py) returns both rows; this module
works on them with one operator, k-nearest-neighbour search of ``nq`` query rows in a bank of ``M`` rows (``cal_knn``: two
launches on the GPU, distances on the matrix cores and the selection fused behind them, no ``[nq, M]`` matrix; libcalhost for
CPU tensors).  The order is total -- distance first, the lower bank row on equal distances -- so every result is reproducible
bit for bit.

* ``knn(queries, bank, k, metric=, skip=, labels=, num_classes=, chunk_rows=)`` -> ``KnnResult``: the raw operator call.
* ``embedding_bank(model, loader, device, max_rows=None)`` -> ``EmbeddingBank``: ``xc``, ``xo``, ``y``, ``pred_o``, ``graph``
  (and ``context`` for SPMotif graphs) of every graph of a loader.
* ``nearest_examples(model, data, bank, k=, space=, metric=, exclude=)`` (also ``model.nearest_examples``): for every graph of
  a batch the bank graphs nearest to it in the objects (``"o"``) or trivial (``"c"``) space -- "this graph is called a house
  because, to the causal branch, it looks like these training graphs".
* ``knn_probe(bank, queries=None, k=, metric=, targets=)`` (also ``model.knn_probe``): kNN accuracy and purity of every target
  (the label, the base type) from ``xo`` and from ``xc``: a table that is diagonal-heavy for a model that has learned the split
  and flat for one that has not.
* ``eval_disentanglement(model, loader, device, test_loader=None, k=5)``: the banks of one or two loaders and their table.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib, spmotif
from .explain import _eval_mode
from .intervene import _pooled
from .plan import _p, _stream

__all__ = ["KnnResult", "EmbeddingBank", "NearestExamples", "knn", "embedding_bank", "nearest_examples", "knn_probe",
           "eval_disentanglement", "MAX_H", "MAX_K", "MAX_C"]

#: limits of the GPU path; the host library takes any sizes
MAX_H = 256
MAX_K = 64
MAX_C = 64
_METRICS = {"l2": 0, "cosine": 1}


@dataclass
class KnnResult:
    """``idx`` int32 [nq, k]: the ``k' = min(k, eligible rows)`` nearest bank rows of every query in ascending order of
    (distance, row), -1 behind them; ``dist`` float32 [nq, k]: their distances (squared Euclidean or cosine), ``+inf`` behind
    them; ``votes`` int32 [nq, C] or ``None``: how many of the neighbours carry label ``c``; ``k``."""
    idx: torch.Tensor
    dist: torch.Tensor
    votes: Optional[torch.Tensor]
    k: int


def knn(queries: torch.Tensor, bank: torch.Tensor, k: int, *, metric: str = "l2", skip: Optional[torch.Tensor] = None,
        labels: Optional[torch.Tensor] = None, num_classes: Optional[int] = None, chunk_rows: int = 0) -> KnnResult:
    """The ``k`` nearest rows of ``bank`` [M, H] for every row of ``queries`` [nq, H] (float32).  ``metric``: ``"l2"`` (squared
    Euclidean) or ``"cosine"`` (cosine distance; 1 against a zero row).  ``skip`` int64 [nq]: a bank row never returned for
    query ``q`` -- its own row when the bank holds it; a value outside [0, M) skips nothing.  ``labels`` int64 [M] with
    ``num_classes``: also ``votes``.  ``chunk_rows``: 0, or the rows of a bank chunk (a multiple of 32; the result does not
    depend on it).  CUDA tensors: ``cal_knn`` on the current stream, two launches, no synchronisation (``H <= 256``,
    ``k <= 64``, ``num_classes <= 64``); CPU tensors: libcalhost, any sizes."""
    if queries.dim() != 2 or bank.dim() != 2 or queries.dtype != torch.float32 or bank.dtype != torch.float32:
        raise ValueError("queries and bank must be 2-D float32 tensors")
    nq, H, M = int(queries.size(0)), int(queries.size(1)), int(bank.size(0))
    if int(bank.size(1)) != H:
        raise ValueError("queries [*, %d] and bank [*, %d] must have one width" % (H, int(bank.size(1))))
    if metric not in _METRICS:
        raise ValueError('metric must be "l2" or "cosine"')
    dev = queries.device
    if bank.device != dev or any(t is not None and t.device != dev for t in (skip, labels)):
        raise ValueError("queries, bank, skip and labels must be on one device")
    if M == 0:
        raise ValueError("the bank is empty (M == 0)")
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1 (got %d)" % k)
    if H < 1:
        raise ValueError("the rows are empty (H == 0)")
    if chunk_rows < 0 or chunk_rows % 32:
        raise ValueError("chunk_rows must be 0 or a positive multiple of 32")
    C = 0
    if labels is not None:
        if num_classes is None or int(num_classes) < 1:
            raise ValueError("labels need num_classes >= 1")
        C = int(num_classes)
        if labels.numel() != M:
            raise ValueError("labels must have one entry per bank row")
        labels = labels.to(torch.long).view(-1).contiguous()
    host = not queries.is_cuda
    if not host:
        if H > MAX_H:
            raise ValueError("the GPU path takes 1 <= H <= %d (got H = %d)" % (MAX_H, H))
        if k > MAX_K:
            raise ValueError("the GPU path takes 1 <= k <= %d (got k = %d)" % (MAX_K, k))
        if C > MAX_C:
            raise ValueError("the GPU path takes num_classes <= %d (got %d)" % (MAX_C, C))
    if M >= 2 ** 31:
        raise ValueError("the bank takes M < 2^31 rows")
    if skip is not None:
        if skip.numel() != nq:
            raise ValueError("skip must have one entry per query")
        skip = skip.to(torch.long).view(-1).contiguous()
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, k, dtype=torch.float32, device=dev)
    votes = torch.empty(nq, C, dtype=torch.int32, device=dev) if labels is not None else None
    if nq == 0:
        return KnnResult(idx, dist, votes, k)
    queries, bank = queries.contiguous(), bank.contiguous()
    wsb = _lib.query("cal_knn_ws", nq, M, k, int(chunk_rows), host=host)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    _lib.call("cal_knn", _p(queries), nq, _p(bank), M, H, _METRICS[metric], k, _p(skip), _p(labels), C, _p(idx), _p(dist),
              _p(votes), int(chunk_rows), _p(ws), wsb, None if host else _stream(), host=host)
    return KnnResult(idx, dist, votes, k)


@dataclass
class EmbeddingBank:
    """The pooled rows of ``M`` graphs: ``xc``, ``xo`` float32 [M, H]; ``y`` int64 [M] the labels; ``pred_o`` int64 [M] the
    objects head's argmax; ``graph`` int64 [M] the running number of the graph in its loader; ``context`` int64 [M]
    (``spmotif.context_of``: 0 tree, 1 ba) or ``None`` when it is not known for every graph."""
    xc: torch.Tensor
    xo: torch.Tensor
    y: torch.Tensor
    pred_o: torch.Tensor
    graph: torch.Tensor
    context: Optional[torch.Tensor] = None

    def rows(self, space: str) -> torch.Tensor:
        if space not in ("o", "c"):
            raise ValueError('space must be "o" (objects rows) or "c" (trivial rows)')
        return self.xo if space == "o" else self.xc

    def __len__(self) -> int:
        return int(self.y.numel())


def embedding_bank(model, loader, device, max_rows: Optional[int] = None) -> EmbeddingBank:
    """``EmbeddingBank`` of every graph of ``loader`` (eval mode, identity permutation, the pooled rows of
    ``pooled_representations``) on ``device``; at most ``max_rows`` graphs (the first ones) when given."""
    cols, n = [], 0
    with _eval_mode(model):
        for data in loader:
            data = data.to(device)
            xc, xo = _pooled(model, data)
            cols.append((xc, xo, data.y.view(-1), model.objects_readout_layer(xo).argmax(-1), spmotif.context_of(data)))
            n += int(xc.size(0))
            if max_rows is not None and n >= max_rows:
                break
    if not cols:
        raise ValueError("the loader is empty")
    xc, xo, y, pred, ctx = (torch.cat(c)[:max_rows].contiguous() for c in zip(*cols))
    return EmbeddingBank(xc, xo, y, pred, torch.arange(y.numel(), device=y.device), ctx if bool((ctx >= 0).all()) else None)


@dataclass
class NearestExamples:
    """For the ``B`` graphs of a batch their ``k`` nearest bank rows: ``idx`` int32 [B, k] (bank rows, -1 behind the last),
    ``dist`` float32 [B, k], and of those rows ``graph``, ``y``, ``pred_o`` int64 [B, k] (-1 behind the last); ``votes`` int32
    [B, C] over the neighbours' ``y``; ``space``, ``metric``."""
    idx: torch.Tensor
    dist: torch.Tensor
    graph: torch.Tensor
    y: torch.Tensor
    pred_o: torch.Tensor
    votes: torch.Tensor
    space: str
    metric: str


def nearest_examples(model, data, bank: EmbeddingBank, *, k: int = 5, space: str = "o", metric: str = "l2",
                     exclude: Optional[torch.Tensor] = None) -> NearestExamples:
    """The bank graphs nearest to every graph of ``data`` in the objects (``space="o"``) or trivial (``"c"``) space: one
    eval-mode forward with the identity permutation for the pooled rows, then ``knn`` against the bank's rows of that space.
    ``exclude`` int64 [B]: the bank row of every graph of a batch that is part of the bank (never returned for it).  Leaves
    parameters, optimizer state, BatchNorm statistics and both RNG states as they were, like ``intervene``."""
    rows = bank.rows(space)
    with _eval_mode(model):
        xc, xo = _pooled(model, data)
        C = int(model.fc2_co.weight.size(0))
        r = knn(xo if space == "o" else xc, rows, k, metric=metric, skip=exclude, labels=bank.y, num_classes=C)
    has = r.idx >= 0
    at = r.idx.clamp(min=0).long()
    take = lambda t: torch.where(has, t[at], torch.full_like(at, -1))
    return NearestExamples(r.idx, r.dist, take(bank.graph), take(bank.y), take(bank.pred_o), r.votes, space, metric)


#: classes of a probe target: its values lie in [0, 64) (others are not counted and never win a vote)
_PROBE_C = MAX_C


def _default_targets(bank: EmbeddingBank, queries: Optional[EmbeddingBank]):
    qb = bank if queries is None else queries
    t = {"y": (bank.y, qb.y)}
    if bank.context is not None and qb.context is not None:
        t["context"] = (bank.context, qb.context)
    return t


def knn_probe(bank: EmbeddingBank, *, queries: Optional[EmbeddingBank] = None, k: int = 5, metric: str = "l2",
              targets: Optional[Dict[str, object]] = None) -> dict:
    """kNN probe of the two spaces.  ``queries=None``: leave-one-out over ``bank`` (every row against the others);
    else the rows of a second ``EmbeddingBank`` against ``bank`` (train bank, test queries).  ``targets``: name -> int64 [M]
    values of the bank rows in [0, 64) (with ``queries``: a pair ``(bank values [M], query values [nq])``); default the label
    ``y``, and ``context`` when the banks carry one (``embedding_bank`` keeps it when it is known for every graph).  Returns

    * ``[space][target]["acc"]``: the share of queries whose neighbours' majority (the lowest value on ties) is their own value;
    * ``[space][target]["purity"]``: the share of all neighbours that carry their query's own value;
    * ``["chance"][target]``: the share of the most frequent value among the bank rows;
    * ``["overlap"]``: the mean Jaccard index of a query's neighbour sets in the two spaces;
    * ``k``, ``queries``, ``bank``: the sizes.

    for ``space`` in ``("o", "c")``.  Per (space, target) one ``knn`` call; integer counts on the device, read back once."""
    if targets is None:
        tg = _default_targets(bank, queries)
    else:
        tg = {}
        for name, v in targets.items():
            bv, qv = v if isinstance(v, (tuple, list)) else (v, v)
            if queries is not None and not isinstance(v, (tuple, list)):
                raise ValueError("with queries a target is a pair (bank values, query values)")
            tg[name] = (bv, qv)
    if not tg:
        raise ValueError("no target to probe")
    qb = bank if queries is None else queries
    nq, M = len(qb), len(bank)
    dev = bank.y.device
    skip = torch.arange(M, device=dev) if queries is None else None
    sums, idxs = [], {}
    for space in ("o", "c"):
        for name, (bv, qv) in tg.items():
            bv, qv = bv.to(dev).long().view(-1), qv.to(dev).long().view(-1)
            if bv.numel() != M or qv.numel() != nq:
                raise ValueError("target %r must have one value per row" % name)
            r = knn(qb.rows(space), bank.rows(space), k, metric=metric, skip=skip, labels=bv, num_classes=_PROBE_C)
            idxs[space] = r.idx
            votes = r.votes.long()
            # majority, the lowest class on ties: the keys votes * C + (C - 1 - c) are distinct (knn_majority of rules.hpp)
            major = (votes * _PROBE_C + torch.arange(_PROBE_C - 1, -1, -1, device=dev)).argmax(1)
            known = (qv >= 0) & (qv < _PROBE_C)
            own = votes.gather(1, qv.clamp(0, _PROBE_C - 1).view(-1, 1)).view(-1) * known
            sums += [((major == qv) & (r.idx[:, 0] >= 0)).sum(), own.sum(), (r.idx >= 0).sum()]
    for name, (bv, _) in tg.items():
        bv = bv.to(dev).long().view(-1)
        sums.append(torch.bincount(bv[(bv >= 0) & (bv < _PROBE_C)], minlength=_PROBE_C).max())
    io, ic = idxs["o"], idxs["c"]
    inter = ((io.unsqueeze(2) == ic.unsqueeze(1)) & (io.unsqueeze(2) >= 0)).sum((1, 2))
    union = (io >= 0).sum(1) + (ic >= 0).sum(1) - inter
    jac = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=dev))
    vals = torch.cat([torch.stack(sums).double(), jac.sum().view(1)]).tolist()
    nan = float("nan")
    out = {"k": int(k), "queries": nq, "bank": M, "chance": {}}
    it = iter(vals)
    for space in ("o", "c"):
        out[space] = {}
        for name in tg:
            hit, own, nb = next(it), next(it), next(it)
            out[space][name] = {"acc": hit / nq if nq else nan, "purity": own / nb if nb else nan}
    for name in tg:
        out["chance"][name] = next(it) / M
    out["overlap"] = next(it) / nq if nq else nan
    return out


def eval_disentanglement(model, loader, device, *, test_loader=None, k: int = 5, metric: str = "l2") -> dict:
    """``knn_probe`` of a model over a loader: leave-one-out over the loader's graphs, or -- with ``test_loader`` -- the test
    graphs against the bank of ``loader``.  The probe's table with ``graphs``, the number of queries."""
    bank = embedding_bank(model, loader, device)
    queries = embedding_bank(model, test_loader, device) if test_loader is not None else None
    out = knn_probe(bank, queries=queries, k=k, metric=metric)
    out["graphs"] = out["queries"]
    return out
