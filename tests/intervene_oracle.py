"""The all-pairs intervention readout written out unfused in torch fp64: for every pair (g, j)
``log_softmax(fc2(bn2(relu(fc1(bn1(x))))))`` with ``x = xc_j + xo_g`` (add) or ``cat(xc_j, xo_g)`` (cat) and eval-mode
BatchNorms, then the mean of the probabilities over j, the argmax counts against ``ref`` and the minimum.  Nothing is folded,
every pair's input row is formed.  Shared by tests/test_intervene.py (host library) and tests/test_gpu_intervene.py (HIP)."""
import argparse

import torch

#: top-two logit gap below which float rounding may flip a pair's argmax
GAP = 1e-3


class Head(torch.nn.Module):
    """The four modules of the ``co`` head with the attributes ``intervention_readout`` reads, randomly initialised: non-zero
    running means, random positive running variances, random BatchNorm weight and bias, Linear weights scaled by H^-1/2."""

    def __init__(self, H, C, cat, seed, gain=1.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        K = 2 * H if cat else H
        self.args = argparse.Namespace(cat_or_add="cat" if cat else "add")
        self.fc1_bn_co, self.fc1_co = torch.nn.BatchNorm1d(K), torch.nn.Linear(K, H)
        self.fc2_bn_co, self.fc2_co = torch.nn.BatchNorm1d(H), torch.nn.Linear(H, C)
        with torch.no_grad():
            for bn in (self.fc1_bn_co, self.fc2_bn_co):
                n = bn.num_features
                bn.weight.copy_(0.5 + torch.rand(n, generator=g))
                bn.bias.copy_(0.3 * torch.randn(n, generator=g))
                bn.running_mean.copy_(0.5 * torch.randn(n, generator=g) + 0.1)
                bn.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
            self.fc2_bn_co.weight.mul_(gain)            # (wider logits: fewer near-ties among thousands of partners)
            for fc in (self.fc1_co, self.fc2_co):
                fc.weight.copy_(torch.randn(fc.weight.shape, generator=g) * H ** -0.5)
                fc.bias.copy_(0.2 * torch.randn(fc.bias.shape, generator=g))
        self.eval()


def rows(n, H, seed):
    """N(0, 1) rows [n, H] float32."""
    return torch.randn(n, H, generator=torch.Generator().manual_seed(seed))


def _bn(bn, x, dt):
    return (x - bn.running_mean.to(dt)) / torch.sqrt(bn.running_var.to(dt) + bn.eps) * bn.weight.to(dt) + bn.bias.to(dt)


def head_logits(head, xo, xc, dtype=torch.float64):
    """Raw logits [B, M, C] of every pair, unfused, in ``dtype`` (fp64: the oracle; fp32: the same statements in float)."""
    cat = head.args.cat_or_add == "cat"
    xo, xc = xo.detach().cpu().to(dtype), xc.detach().cpu().to(dtype)
    w1, b1 = head.fc1_co.weight.detach().cpu().to(dtype), head.fc1_co.bias.detach().cpu().to(dtype)
    w2, b2 = head.fc2_co.weight.detach().cpu().to(dtype), head.fc2_co.bias.detach().cpu().to(dtype)
    out = []
    for g in range(xo.size(0)):
        x = torch.cat((xc, xo[g].expand_as(xc)), dim=1) if cat else xc + xo[g]
        h = torch.relu(_bn(head.fc1_bn_co, x, dtype) @ w1.t() + b1)
        out.append(_bn(head.fc2_bn_co, h, dtype) @ w2.t() + b2)
    C = w2.size(0)
    return torch.stack(out) if out else torch.zeros(0, xc.size(0), C, dtype=dtype)


def oracle(head, xo, xc, ref=None):
    """dict: ``logits``, ``logp`` [B, M, C] fp64, ``p_do`` [B, C], and with ``ref`` [B] (valid classes): ``lo`` / ``hi`` [B] the
    bracket of the hit counts (``lo``: pairs matching ``ref`` with a top-two gap above GAP; ``hi``: those plus every pair whose
    gap is at most GAP), ``p_ref`` [B, M] the probability of ``ref`` for every pair, ``p_min`` [B]."""
    z = head_logits(head, xo, xc)
    logp = torch.log_softmax(z, dim=-1)
    res = {"logits": z, "logp": logp, "p_do": logp.exp().mean(1)}
    if ref is not None:
        ref = ref.cpu().long()
        top = z.topk(2, dim=-1).values
        close = (top[..., 0] - top[..., 1]) <= GAP
        match = z.argmax(-1) == ref[:, None]
        res["lo"] = (match & ~close).sum(1)
        res["hi"] = res["lo"] + close.sum(1)
        res["p_ref"] = logp.exp().gather(2, ref[:, None, None].expand(-1, z.size(1), 1)).squeeze(2)
        res["p_min"] = res["p_ref"].min(1).values
    return res
