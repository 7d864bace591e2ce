"""fp64 restatement of the learned-mask optimiser -- TEST INFRASTRUCTURE, independent of cal_amd.maskopt:
the one-step formula of ``cal_mask_step`` (with the seeded defects of tests/test_maskopt.py), the loss, the free-running loop
over ``softmask_oracle.masked_forward`` with torch autograd taken through the WHOLE loss (prediction term and both regularisers,
the entropy in its logarithm form), and the case tables tests/test_maskopt.py (host twin, host path) and tests/test_gpu_maskopt.py
(HIP) share.

Kernel tolerances (``KERNEL_ATOL``): 8 x the largest |fp32 host twin - fp64 formula| over every case of ``KERNEL_CASES`` (the
GPU's exp, sqrt and division are a few ulp off the host's).  Measured on the CPU:

    theta 3.80e-6 (half an ulp at |theta| = 80)   exp_avg 1.75e-9   exp_avg_sq 7.18e-12   mask 8.71e-8
    terms 2.40e-6 (double sums of up to 1000 fp32 values; the size sums reach 560)

Model tolerances (``MODEL_ATOL``): 4 x the largest |fp32 host path - this oracle| per model over every case of ``LEARN_CASES``
at 4 steps, lr 0.01, init 1.0 (three graphs, 17 nodes, 44 columns, H 32, L 2).  Measured on the CPU:

                theta      mask       p_masked   loss       smallest ReLU |pre|   smallest |dL/dtheta|
    CausalGCN   1.45e-7    6.02e-8    6.32e-8    1.61e-7    1.93e-4               5.68e-3
    CausalGAT   1.59e-7    6.09e-8    4.12e-8    1.95e-7    1.69e-4               8.14e-3
    CausalGIN   1.48e-7    5.78e-8    3.38e-8    9.84e-8    2.54e-4               1.09e-2

(theta is about 1 and moves by 0.04 in the four steps: the first row is one to two ulp of it.)

The comparison means something only while (A) every ReLU of every differentiated forward stays >= 1e-4 from its kink and (B)
every player's |dL/dtheta| stays >= 1000 x the model's ``SCORE_ATOL`` (Adam's normalisation cannot flip a sign): both are
asserted on the oracle alone by tests/test_maskopt.py for every case; the minima over the cases are the last two columns above.
CausalGAT's subset case takes a state of its own (``LEARN_SEED``): at ``MODEL_SEED`` a ReLU comes within 2.5e-6 of its kink.
"""
import math

import torch

from tests import softmask_oracle as SO


def f32(v):
    """The value the C ABI receives for a float argument, as a Python double."""
    return torch.tensor(float(v), dtype=torch.float32).double().item()


# ---- the loss and the step -------------------------------------------------------------------------------------------------------
def entropy(theta):
    """H(sigmoid(theta)) = softplus(theta) - theta sigmoid(theta), fp64, finite for any finite theta."""
    a = theta.abs()
    z = (-a).exp()
    return torch.log1p(z) + a * z / (1 + z)


DEFECTS = ("no_bias_correction", "mate_grad_dropped", "entropy_mean_over_elements", "terms_after_update", "entropy_sign_flipped",
           "mate_not_written")


def step_formula(pptr, rep, mate, grad, theta, exp_avg, exp_avg_sq, mask, M, step, lr, beta1, beta2, eps, l_size, l_ent, defect=None):
    """One ``cal_mask_step`` in fp64 -> ``(theta, exp_avg, exp_avg_sq, mask, terms [B, 2])``.  The float inputs are taken as they
    are (fp32 values in fp64), the scalars as the floats the ABI receives.  ``defect``: one of ``DEFECTS``."""
    lr, beta1, beta2, eps, l_size, l_ent = (f32(v) for v in (lr, beta1, beta2, eps, l_size, l_ent))
    B, P = pptr.numel() - 1, theta.numel()
    theta, m1, m2, mask = theta.double().clone(), exp_avg.double().clone(), exp_avg_sq.double().clone(), mask.double().clone()
    rep, mate = rep.long(), mate.long()
    r_ok, t_ok = (rep >= 0) & (rep < M), (mate >= 0) & (mate < M)
    lo = pptr.clamp(0, P)
    hi = torch.maximum(lo[1:], lo[:-1])
    lo = lo[:-1]
    gid = torch.full((P,), -1, dtype=torch.long)
    cnt = torch.zeros(P, dtype=torch.float64)
    for g in range(B):
        gid[lo[g]:hi[g]] = g
        n = float(hi[g] - lo[g])
        if defect == "entropy_mean_over_elements":
            n += float(t_ok[lo[g]:hi[g]].sum())
        cnt[lo[g]:hi[g]] = n
    live = gid >= 0

    def sums(th):
        out = torch.zeros(B, 2, dtype=torch.float64)
        out[:, 0].index_add_(0, gid[live], torch.sigmoid(th)[live])
        out[:, 1].index_add_(0, gid[live], entropy(th)[live])
        return out
    terms = sums(theta)
    if step > 0:
        grad = grad.double()
        g = torch.where(r_ok, grad[rep.clamp(0, M - 1)], torch.zeros(P, dtype=torch.float64))
        if defect != "mate_grad_dropped":
            g = g + torch.where(t_ok, grad[mate.clamp(0, M - 1)], torch.zeros(P, dtype=torch.float64))
        m = torch.sigmoid(theta)
        sign = 1.0 if defect == "entropy_sign_flipped" else -1.0
        g = (g + l_size + sign * l_ent / cnt.clamp(min=1.0) * theta) * m * (1 - m)
        n1, n2 = beta1 * m1 + (1 - beta1) * g, beta2 * m2 + (1 - beta2) * g * g
        bc1, bc2 = (1.0, 1.0) if defect == "no_bias_correction" else (1 - beta1 ** step, 1 - beta2 ** step)
        new = theta - lr / bc1 * n1 / (n2.sqrt() / math.sqrt(bc2) + eps)
        theta, m1, m2 = torch.where(live, new, theta), torch.where(live, n1, m1), torch.where(live, n2, m2)
        if defect == "terms_after_update":
            terms = sums(theta)
    val = torch.sigmoid(theta)
    mask[rep[r_ok & live]] = val[r_ok & live]
    if defect != "mate_not_written":
        mask[mate[t_ok & live]] = val[t_ok & live]
    return theta, m1, m2, mask, terms


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------
KERNEL_COUNTS = (0, 1, 63, 257, 1000)      # players per graph: the empty graph, one lane, a partial wave, the stride loop
KERNEL_STEPS = (0, 1, 2, 10000)
KERNEL_COEFFS = ((0.0, 0.0), (0.005, 0.0), (0.0, 1.0), (0.005, 1.0))       # (l_size, l_ent): both 0, each alone, the defaults
KERNEL_CASES = tuple((s, c) for s in KERNEL_STEPS for c in KERNEL_COEFFS)
ADAM = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
THETA_GRID = (-80.0, -5.0, 0.0, 1.0, 5.0, 80.0)
#: 8 x the measured maxima of the module docstring
KERNEL_ATOL = dict(theta=8 * 3.80e-6, exp_avg=8 * 1.75e-9, exp_avg_sq=8 * 7.18e-12, mask=8 * 8.71e-8, terms=8 * 2.40e-6)
_KERNEL = {}


def kernel_inputs():
    """The shared inputs (computed once, not to be changed): B = 5 graphs of ``KERNEL_COUNTS`` players, half of them pairs, their
    elements a random permutation of [0, M) with 211 non-player elements in between; player 71 has its ``rep`` and player 400 its
    ``mate`` out of range; ``grad`` is exactly 0 on both elements of every seventh player, whose moments are 0 too; ``theta`` walks
    ``THETA_GRID`` on the first 600 players and is random beyond."""
    if not _KERNEL:
        g = torch.Generator().manual_seed(11)
        P = sum(KERNEL_COUNTS)
        pptr = torch.tensor((0,) + KERNEL_COUNTS, dtype=torch.long).cumsum(0)
        pair = torch.rand(P, generator=g) < 0.5
        npair = int(pair.sum())
        M = P + npair + 211
        perm = torch.randperm(M, generator=g)
        rep = perm[:P].to(torch.int32)
        mate = torch.full((P,), -1, dtype=torch.int32)
        mate[pair] = perm[P:P + npair].to(torch.int32)
        pair[400] = True
        rep[71], mate[400] = M + 3, M                                 # (their elements become non-players)
        grad = torch.randn(M, generator=g) * 0.05
        zero = torch.arange(P) % 7 == 0
        grad[rep[zero & (rep < M)].long()] = 0.0
        grad[mate[zero & (mate >= 0) & (mate < M)].long()] = 0.0
        theta = torch.randn(P, generator=g) * 2.0
        theta[:600] = torch.tensor(THETA_GRID)[torch.arange(600) % 6]
        exp_avg = torch.randn(P, generator=g) * 0.01
        exp_avg_sq = torch.rand(P, generator=g) * 1e-4
        exp_avg[zero], exp_avg_sq[zero] = 0.0, 0.0
        mask = torch.rand(M, generator=g) + 2.0                        # prior bits no sigmoid produces
        _KERNEL.update(pptr=pptr, rep=rep, mate=mate, grad=grad, theta=theta, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, mask=mask,
                       M=M, P=P, B=len(KERNEL_COUNTS), zero=zero, pair=pair)
    return _KERNEL


def kernel_want(case, defect=None):
    step, (l_size, l_ent) = case
    k = kernel_inputs()
    key = ("want", case, defect)
    if key not in _KERNEL:
        _KERNEL[key] = step_formula(k["pptr"], k["rep"], k["mate"], k["grad"], k["theta"], k["exp_avg"], k["exp_avg_sq"], k["mask"],
                                    k["M"], step, l_size=l_size, l_ent=l_ent, defect=defect, **ADAM)
    return _KERNEL[key]


KERNEL_OUTPUTS = ("theta", "exp_avg", "exp_avg_sq", "mask", "terms")


def kernel_errors(got, want):
    """max |got - want| per output of ``KERNEL_OUTPUTS``; everything has to be finite."""
    out = {}
    for name, a, b in zip(KERNEL_OUTPUTS, got, want):
        a = a.cpu().double().view(b.shape)
        assert bool(torch.isfinite(a).all()), name
        out[name] = (a - b).abs().max().item() if b.numel() else 0.0
    return out


def within(err):
    return all(err[k] <= KERNEL_ATOL[k] for k in KERNEL_OUTPUTS)


# ---- the free-running loop -------------------------------------------------------------------------------------------------------
LEARN_STEPS = 4
#: (use, undirected, subset of the elements, head): edges, undirected pairs, nodes, a subset, the co head
LEARN_CASES = (("edges", None, False, "o"), ("edges", "mean", False, "o"), ("nodes", None, False, "o"),
               ("edges", "mean", True, "o"), ("nodes", None, False, "co"))
#: the measured |fp32 host path - oracle| per model (module docstring); the tolerance is 4 x that
MODEL_MAX = {"CausalGCN": dict(theta=1.45e-7, mask=6.02e-8, p_masked=6.32e-8, loss=1.61e-7),
             "CausalGAT": dict(theta=1.59e-7, mask=6.09e-8, p_masked=4.12e-8, loss=1.95e-7),
             "CausalGIN": dict(theta=1.48e-7, mask=5.78e-8, p_masked=3.38e-8, loss=9.84e-8)}
MODEL_ATOL = {n: {k: 4 * v for k, v in d.items()} for n, d in MODEL_MAX.items()}
RELU_MARGIN = 1e-4
#: (model, case) -> seed of ``model_state`` where ``softmask_oracle.MODEL_SEED`` does not keep both conditions (searched on the CPU,
#: on the oracle alone)
LEARN_SEED = {("CausalGAT", ("edges", "mean", True, "o")): 1}        # (seed 5: a ReLU 2.5e-6 from its kink at step 3)
_LEARN = {}


def players_of(data, use, undirected, member):
    """-> (rep [P], mate [P] or -1, gid of the players, member [M]) in graph order, elements in order inside a graph."""
    from cal_amd.explain import edge_twins
    M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
    gid = data.batch[data.edge_index[0]] if use == "edges" else data.batch
    member = torch.ones(M, dtype=torch.bool) if member is None else member.clone()
    idx = torch.arange(M)
    rep, mate = member, torch.full((M,), -1, dtype=torch.long)
    if undirected is not None:
        twin = edge_twins(data)[0]
        t = twin.clamp(min=0).long()
        paired = (twin >= 0) & (t != idx)
        member = member | (member[t] & paired)
        rep = member & ~(paired & (t < idx))
        mate = torch.where(paired, t, mate)
    players = idx[rep]
    players = players[torch.argsort(gid[players], stable=True)]
    return players, mate[players], gid[players], member


def graph_of(data, g):
    """Graph ``g`` of ``data`` alone -> (the one-graph batch, its node ids, its column ids in ``data``)."""
    nodes = (data.batch == g).nonzero().view(-1)
    cols = (data.batch[data.edge_index[0]] == g).nonzero().view(-1)
    f = SO._Foreign()
    f.x, f.feat, f.y = None, data.feat[nodes], data.y[g:g + 1]
    f.batch, f.num_graphs = torch.zeros(nodes.numel(), dtype=torch.long), 1
    f.edge_index = (data.edge_index[:, cols] - nodes[0]).contiguous()
    return f, nodes, cols


def oracle_learn(name, case, steps=LEARN_STEPS, lr=0.01, init=1.0, l_size=0.005, l_ent=1.0, beta1=0.9, beta2=0.999, eps=1e-8,
                 data=None, member=None, key=None, seed=None):
    """The optimiser in fp64 on ``softmask_oracle.model_batch()`` (or ``data``) -> dict(theta, mask, p_full, p_masked, yhat,
    loss [steps + 1, B, 3], rep, mate, min_pre, min_grad); computed once per ``(name, case, steps, key)``."""
    seed = LEARN_SEED.get((name, case)) if seed is None else seed
    ck = (name, case, steps, key, seed)
    if ck in _LEARN:
        return _LEARN[ck]
    use, undirected, subset, head = case
    lr, beta1, beta2, eps, l_size, l_ent = (f32(v) for v in (lr, beta1, beta2, eps, l_size, l_ent))
    data = SO.model_batch() if data is None else data
    feat = data.feat.size(1)
    sd64 = {k: v.double() for k, v in SO.model_state(name, feat, seed=seed).items()}
    M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
    B, h = data.num_graphs, ("c", "o", "co").index(head)
    if member is None and subset:
        member = SO.subset_of(M)
    rep, mate, pg, member = players_of(data, use, undirected, member)
    P = rep.numel()
    cnt = torch.zeros(B, dtype=torch.float64).index_add_(0, pg, torch.ones(P, dtype=torch.float64))
    track = SO.Track()
    fwd = SO.oracle_forward(name, sd64, data)(use, track)
    with torch.no_grad():
        lp = SO.oracle_forward(name, sd64, data)(use)(torch.ones(M, dtype=torch.float64))[h]
    yhat = lp.argmax(-1)
    p_full = lp.gather(-1, yhat.view(-1, 1)).view(-1).exp()

    def parts(theta, forward):
        m = torch.sigmoid(theta)
        mask = torch.ones(M, dtype=torch.float64).index_put((rep,), m)
        mask = mask.index_put((mate[mate >= 0],), m[mate >= 0])
        pred = -forward(mask)[h].gather(-1, yhat.view(-1, 1)).view(-1)
        H = -m * m.log() - (1 - m) * (1 - m).log()
        size = l_size * torch.zeros(B, dtype=torch.float64).index_add(0, pg, m)
        ent = l_ent * torch.zeros(B, dtype=torch.float64).index_add(0, pg, H) / cnt.clamp(min=1.0)
        return torch.stack([pred, size, ent], -1), mask
    theta = torch.full((P,), f32(init), dtype=torch.float64)
    m1, m2 = torch.zeros_like(theta), torch.zeros_like(theta)
    loss, min_grad = [], float("inf")
    for s in range(1, steps + 1):
        th = theta.clone().requires_grad_(True)
        row, _ = parts(th, fwd)
        (g,) = torch.autograd.grad(row.sum(), th)
        loss.append(row.detach())
        if P:
            min_grad = min(min_grad, g.abs().min().item())
        m1, m2 = beta1 * m1 + (1 - beta1) * g, beta2 * m2 + (1 - beta2) * g * g
        theta = theta - lr / (1 - beta1 ** s) * m1 / (m2.sqrt() / math.sqrt(1 - beta2 ** s) + eps)
    with torch.no_grad():
        row, mask = parts(theta, SO.oracle_forward(name, sd64, data)(use))       # the closing forward is not differentiated
    loss.append(row)
    mask = torch.where(member, mask, torch.full_like(mask, float("nan")))
    _LEARN[ck] = dict(theta=theta, mask=mask, p_full=p_full, p_masked=(-row[:, 0]).exp(), yhat=yhat, loss=torch.stack(loss), rep=rep,
                      mate=mate, gid=pg, min_pre=track.min_pre, min_grad=min_grad)
    return _LEARN[ck]
