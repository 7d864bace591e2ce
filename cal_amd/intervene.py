"""All-pairs intervention readout: CAL's backdoor adjustment evaluated exactly instead of sampled.

CAL's argument is ``P(Y | do(C)) = sum_s P(Y | C, s) P(s)``: the causal part of a graph should predict the label whatever
trivial part it is paired with.  The model samples that sum: ``random_readout_layer`` (model.py:145-164) pairs every graph's
pooled objects row ``xo_g`` with ONE trivial row ``xc_perm[g]``, and ``eval_acc_causal(eval_random=True)`` reports the accuracy
of that one draw.  Here the ``co`` head runs on every pair ``(g, j)`` of a batch's objects rows and a bank of trivial rows
(``cal_intervene_pairs``: three launches on the GPU, libcalhost for CPU tensors; no ``[B, M, H]`` tensor exists):

* ``pooled_representations(model, data)`` -> ``(xc [B, H], xo [B, H])``: the pooled rows of one eval-mode forward with the
  identity permutation, as private copies (the engine's ``pooled`` buffer, which every route of the step leaves behind, or the
  operator-level ``_CausalBase._pooled``).
* ``intervention_readout(model, xo, xc_bank, ref=None, pairs=False)`` -> ``InterventionResult``: the raw operator call.
* ``intervene(model, data, bank=None, ref="y", pairs=False)`` (also ``model.intervene``): the same from a batch; ``bank=None``
  pairs every graph with the batch's own trivial rows, ``ref`` is the class each graph is judged against -- ``"y"`` (the
  label), ``"o"`` (the objects head's argmax) or a tensor.
* ``trivial_bank(model, loader, device, max_rows=None)`` -> ``[M, H]``: the trivial rows of a whole loader.
* ``eval_intervention(model, loader, device, bank="batch")`` -> ``acc_do``, ``acc_mean``, ``acc_all``, ``p_min_mean``,
  ``graphs``; the counterpart of ``eval_acc_causal`` without its noise.

``acc_mean`` is the mean over the graphs of ``hits_g / M``, the share of trivial partners under which the ``co`` head predicts
the label.  With ``bank="batch"`` the partner of a graph under a uniformly random permutation is uniform over the batch, so
``acc_mean`` is the exact expectation of the ``co`` accuracy that ``eval_acc_causal(eval_random=True)`` estimates from one
draw.  ``acc_do`` judges the adjusted prediction itself (the argmax of ``p_do``), ``acc_all`` asks for every partner at once.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .explain import _eval_forward, _eval_mode
from .plan import _p, _stream

__all__ = ["InterventionResult", "pooled_representations", "intervention_readout", "intervene", "trivial_bank",
           "eval_intervention", "MAX_H", "MAX_C"]

#: limits of the GPU path (the step engine's own); the host library takes any sizes
MAX_H = 256
MAX_C = 64


@dataclass
class InterventionResult:
    """``p_do`` float32 [B, C]: the backdoor-adjusted prediction, the mean over the bank of ``softmax(co head)``.  Against
    ``ref``: ``hits`` int32 [B] partners whose argmax (lowest class on ties) is ``ref[g]``, ``p_min`` float32 [B] the lowest
    probability of ``ref[g]`` over the bank and ``j_min`` int32 [B] the first partner attaining it; without a ``ref`` (or with
    one outside [0, C)) they are 0, NaN and -1.  ``logp_pairs`` float32 [B, M, C] only with ``pairs=True``.  ``M``: bank rows."""
    p_do: torch.Tensor
    hits: torch.Tensor
    p_min: torch.Tensor
    j_min: torch.Tensor
    logp_pairs: Optional[torch.Tensor]
    M: int


def _pooled(model, data):
    """(xc, xo) of one forward in the module's current mode; engine-backed models: private copies of the ``pooled`` buffer."""
    eng = _eval_forward(model, data)
    if eng is None:
        return model._pooled(data)
    B = int(data.num_graphs)
    pooled = eng.buffer("pooled", 2 * B * eng.H).clone().view(2, B, eng.H)
    return pooled[0], pooled[1]


def pooled_representations(model, data):
    """``(xc [B, H], xo [B, H])``: the pooled trivial and objects rows of ``data`` from one eval-mode forward with the identity
    permutation; private copies that survive later engine calls.  Leaves the model's state as ``explain`` does."""
    with _eval_mode(model):
        xc, xo = _pooled(model, data)
        return xc.clone() if xc._base is None else xc, xo.clone() if xo._base is None else xo


def _bn_args(bn):
    return [_p(bn.weight.detach().contiguous()), _p(bn.bias.detach().contiguous()), _p(bn.running_mean.contiguous()),
            _p(bn.running_var.contiguous()), float(bn.eps)]


def intervention_readout(model, xo: torch.Tensor, xc_bank: torch.Tensor, ref: Optional[torch.Tensor] = None, *,
                         pairs: bool = False) -> InterventionResult:
    """The eval-mode ``co`` head of ``model`` on every pair of an objects row ``xo`` [B, H] and a trivial row ``xc_bank``
    [M, H] (M independent of B); ``ref`` int64 [B] or ``None``.  CUDA tensors: ``cal_intervene_pairs`` on the current stream,
    three launches, no synchronisation (``1 <= H <= 256``, ``2 <= C <= 64``); CPU tensors: libcalhost, any sizes."""
    if xo.dim() != 2 or xc_bank.dim() != 2 or xo.dtype != torch.float32 or xc_bank.dtype != torch.float32:
        raise TypeError("xo and xc_bank must be 2-D float32 tensors")
    B, H = int(xo.size(0)), int(xo.size(1))
    M = int(xc_bank.size(0))
    cat = model.args.cat_or_add == "cat"
    fc1, fc2 = model.fc1_co, model.fc2_co
    C = int(fc2.weight.size(0))
    if int(xc_bank.size(1)) != H or int(fc1.weight.size(0)) != H or int(fc1.weight.size(1)) != (2 * H if cat else H):
        raise ValueError("xo / xc_bank must be [*, %d] rows, the width of the model's co head" % int(fc1.weight.size(0)))
    if M == 0:
        raise ValueError("the bank of trivial rows is empty (M == 0)")
    host = not xo.is_cuda
    dev = xo.device
    if xc_bank.device != dev or fc1.weight.device != dev:
        raise ValueError("xo, xc_bank and the model must be on one device")
    if not host:
        if not 1 <= H <= MAX_H:
            raise ValueError("the GPU path takes 1 <= H <= %d (got H = %d)" % (MAX_H, H))
        if not 2 <= C <= MAX_C:
            raise ValueError("the GPU path takes 2 <= C <= %d (got C = %d)" % (MAX_C, C))
    if ref is not None:
        if ref.numel() != B:
            raise ValueError("ref must have one entry per graph")
        ref = ref.to(device=dev, dtype=torch.long).view(-1).contiguous()
    p_do = torch.empty(B, C, dtype=torch.float32, device=dev)
    ints = torch.empty(2, B, dtype=torch.int32, device=dev)
    p_min = torch.empty(B, dtype=torch.float32, device=dev)
    lp = torch.empty(B, M, C, dtype=torch.float32, device=dev) if pairs else None
    if B == 0:
        return InterventionResult(p_do, ints[0], p_min, ints[1], lp, M)
    xo, xc_bank = xo.contiguous(), xc_bank.contiguous()
    wsb = _lib.query("cal_intervene_ws", B, M, H, C, host=host)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    keep = [fc1.weight.detach().contiguous(), fc1.bias.detach().contiguous(), fc2.weight.detach().contiguous(),
            fc2.bias.detach().contiguous()]
    _lib.call("cal_intervene_pairs", _p(xo), B, _p(xc_bank), M, H, C, int(cat), *_bn_args(model.fc1_bn_co), _p(keep[0]),
              _p(keep[1]), *_bn_args(model.fc2_bn_co), _p(keep[2]), _p(keep[3]), _p(ref), _p(p_do), _p(ints[0]), _p(p_min),
              _p(ints[1]), _p(lp), _p(ws), wsb, None if host else _stream(), host=host)
    return InterventionResult(p_do, ints[0], p_min, ints[1], lp, M)


def _ref_of(model, data, xo, ref):
    if ref is None or torch.is_tensor(ref):
        return ref
    if ref == "y":
        return data.y.view(-1)
    if ref == "o":
        return model.objects_readout_layer(xo).argmax(-1)
    raise ValueError('ref must be "y", "o", a tensor or None')


def intervene(model, data, *, bank: Optional[torch.Tensor] = None, ref="y", pairs: bool = False) -> InterventionResult:
    """``intervention_readout`` of the batch ``data``: one eval-mode forward with the identity permutation for the pooled rows,
    then the ``co`` head on every (graph, partner) pair.  ``bank=None``: the batch's own trivial rows (M = B; partner ``g`` is
    the graph's own); else a ``[M, H]`` tensor such as ``trivial_bank`` gives.  ``ref``: ``"y"`` (``data.y``), ``"o"`` (the
    objects head's argmax), an int64 [B] tensor, or ``None``.  Parameters, optimizer state, the engine's step counter, BatchNorm
    statistics and both RNG states are left as they were, and ``model.training`` is restored."""
    if not (ref is None or torch.is_tensor(ref) or ref in ("y", "o")):
        raise ValueError('ref must be "y", "o", a tensor or None')
    with _eval_mode(model):
        xc, xo = _pooled(model, data)
        return intervention_readout(model, xo, xc if bank is None else bank, _ref_of(model, data, xo, ref), pairs=pairs)


def trivial_bank(model, loader, device, max_rows: Optional[int] = None) -> torch.Tensor:
    """The pooled trivial rows ``xc`` of every graph of ``loader`` (eval mode, identity permutation), ``[M, H]`` on ``device``;
    at most ``max_rows`` rows (the first ones) when given."""
    rows, n = [], 0
    with _eval_mode(model):
        for data in loader:
            xc = _pooled(model, data.to(device))[0]
            rows.append(xc.clone() if xc._base is None else xc)
            n += int(xc.size(0))
            if max_rows is not None and n >= max_rows:
                break
    if not rows:
        raise ValueError("the loader is empty")
    bank = torch.cat(rows)
    return bank[:max_rows].contiguous() if max_rows is not None else bank


def eval_intervention(model, loader, device, *, bank="batch") -> dict:
    """The ``co`` head under every trivial partner, over a loader.  ``bank="batch"``: every graph against the trivial rows of
    its own mini-batch; or a ``[M, H]`` tensor used for every batch.  With ``ref = y``:

    * ``acc_do``: accuracy of the backdoor-adjusted prediction, the argmax of ``p_do``;
    * ``acc_mean``: the mean over the graphs of ``hits_g / M`` (``sum_g hits_g / (M n)`` for one bank size) -- with
      ``bank="batch"`` the exact expectation of the ``co`` accuracy ``eval_acc_causal(eval_random=True)`` draws once;
    * ``acc_all``: the share of graphs whose prediction is right under EVERY partner (``hits_g == M``);
    * ``p_min_mean``: the mean of the label's lowest probability over the bank;
    * ``graphs``: n.

    Per mini-batch one eval forward and one ``cal_intervene_pairs`` call; the sums stay on the device until one read-back."""
    if not (torch.is_tensor(bank) or bank == "batch"):
        raise ValueError('bank must be "batch" or a [M, H] tensor')
    sums = torch.zeros(5, dtype=torch.float64, device=device)
    with _eval_mode(model):
        for data in loader:
            data = data.to(device)
            xc, xo = _pooled(model, data)
            y = data.y.view(-1)
            r = intervention_readout(model, xo, xc if not torch.is_tensor(bank) else bank, y)
            sums += torch.stack([(r.p_do.argmax(-1) == y).sum().double(), r.hits.double().sum() / r.M,
                                 (r.hits == r.M).sum().double(), r.p_min.double().sum(),
                                 torch.as_tensor(float(y.numel()), dtype=torch.float64, device=y.device)])
    do, mean, all_, pmin, n = sums.tolist()
    nan = float("nan")
    return {"acc_do": do / n if n else nan, "acc_mean": mean / n if n else nan, "acc_all": all_ / n if n else nan,
            "p_min_mean": pmin / n if n else nan, "graphs": int(n)}
