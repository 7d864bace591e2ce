"""fp64 restatement of the parametric edge explainer -- TEST INFRASTRUCTURE, independent of
cal_amd.pgexplain: the integer draw of the concrete noise on Python ints, the forward formula of ``cal_edge_mlp_fwd`` and the
backward formula of ``cal_edge_mlp_bwd`` (with the seeded defects of tests/test_pgexplain.py), a free-running training loop over
``softmask_oracle``'s fp64 masked forward with torch autograd through a torch-composed MLP (gather, concat, two linears,
elementwise sampling, the entropy in its logarithm form) and its own fp64 Adam, and the case tables tests/test_pgexplain.py
(host twins, host path) and tests/test_gpu_pgexplain.py (HIP) share.

Kernel tolerances (``KERNEL_ATOL``): 8 x the largest |fp32 host twin - fp64 formula| per output over every case of
``KERNEL_CASES`` (the GPU's exp, log and division are a few ulp off the host's, and it sums a column's hidden units in another
order).  Measured on the CPU:

    omega 3.76e-4 (at Hd 256, where |omega| reaches 400: 256 terms summed in fp32, an ulp there is 3.1e-5)   z 3.76e-4
    mask 3.48e-7   terms 1.01e-6 (double sums of up to 150 fp32 values)   dpq 1.31e-7   dw2 2.45e-7   db2 3.09e-7

(omega's and z's figures come from the two saturated edges; an ordinary player's omega is held through ``mask``, whose bound is
three ulp of a value near 1.)

Model tolerances (``MODEL_ATOL``): 4 x the largest |fp32 host path - this oracle| per model over every case of ``TRAIN_CASES`` at
4 steps, Hd 8, lr 0.003 (three graphs, 17 nodes, 44 columns, H 32, L 2).  Measured on the CPU:

                params     omega      mask       p_masked   loss       smallest ReLU |pre|   smallest non-zero |dL/dparam|
    CausalGCN   4.92e-8    2.16e-7    8.21e-8    8.28e-8    3.54e-7    1.17e-4               2.01e-6
    CausalGAT   4.81e-8    2.17e-7    7.70e-8    4.54e-8    2.07e-7    1.12e-4               2.05e-6
    CausalGIN   2.39e-8    5.30e-7    5.00e-8    3.35e-8    1.17e-7    1.45e-4               1.71e-6

(the parameters are about 0.1 and move by 0.012 in the four steps.)

The comparison means something only while (A) every ReLU -- the model's, in the embedding pass and in every differentiated
forward, and the explainer's hidden units on every column -- stays >= ``RELU_MARGIN`` from its kink and (B) every parameter
gradient of every step is exactly 0 (a dead unit, a zero embedding) or >= ``GRAD_MARGIN`` in size (Adam's normalisation cannot
flip a sign): both are asserted on the oracle alone by tests/test_pgexplain.py for every case; the minima over the cases are the
last two columns above.  The states are ``TRAIN_SEED``'s: (model state, explainer initialisation), searched on the oracle alone.
"""
import math

import torch
import torch.nn.functional as F

from oracle import cal_oracle as O
from tests import maskopt_oracle as MO
from tests import softmask_oracle as SO

f32 = MO.f32
MASK64 = (1 << 64) - 1


# ---- the concrete noise ----------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def draw(seed, step, p):
    """The 23-bit integer of player ``p`` at ``step``: ``H(seed, step 2^32 + p) >> 41``."""
    return splitmix64((splitmix64(seed) + ((step << 32) + p)) & MASK64) >> 41


def uniform(seed, step, p):
    """``u_p = (draw + 1/2) 2^-23`` as a Python float: exact (24 significant bits), in (0, 1)."""
    return (2 * draw(seed, step, p) + 1) / float(1 << 24)


def noise(seed, step, P, keyed_by_step=True):
    """fp64 [P]: ``log u - log(1 - u)``; zeros for ``seed == 0``."""
    if seed == 0:
        return torch.zeros(P, dtype=torch.float64)
    u = torch.tensor([uniform(seed, step if keyed_by_step else 0, p) for p in range(P)], dtype=torch.float64)
    return u.log() - (1 - u).log()


# ---- the formulas ----------------------------------------------------------------------------------------------------------------
DEFECTS = ("pair_not_halved", "q_from_source_row", "entropy_sign_flipped", "noise_without_step", "mate_not_written",
           "relu_dropped")


def _tables(k):
    E, P, B = k["E"], k["P"], k["B"]
    rep, mate = k["rep"].long(), k["mate"].long()
    r_ok = (rep >= 0) & (rep < E)
    t_ok = r_ok & (mate >= 0) & (mate < E)
    lo = k["pptr"].clamp(0, P)
    hi = torch.maximum(lo[1:], lo[:-1])
    lo = lo[:-1]
    gid = torch.full((P,), -1, dtype=torch.long)
    cnt = torch.ones(P, dtype=torch.float64)
    for g in range(B):
        gid[lo[g]:hi[g]] = g
        cnt[lo[g]:hi[g]] = float(hi[g] - lo[g])
    return rep, mate, r_ok & (gid >= 0), t_ok & (gid >= 0), gid, cnt


def _hidden(k, defect=None):
    Hd = k["Hd"]
    pq = k["pq"].double()
    row, col = k["row"].long(), k["col"].long()
    return pq[row, :Hd] + pq[row if defect == "q_from_source_row" else col, Hd:]


def forward_formula(k, tau, seed, step, defect=None):
    """``cal_edge_mlp_fwd`` in fp64 on the inputs ``k`` -> ``(omega [P], z [P], mask [E], terms [B, 2])``."""
    tau = f32(tau)
    rep, mate, r_ok, t_ok, gid, _ = _tables(k)
    E, P, B = k["E"], k["P"], k["B"]
    h = _hidden(k, defect)
    act = h if defect == "relu_dropped" else h.clamp(min=0)
    om_e = k["b2"].double() + act @ k["w2"].double()
    rc, mc = rep.clamp(0, E - 1), mate.clamp(0, E - 1)
    zero = torch.zeros(P, dtype=torch.float64)
    omega = torch.where(t_ok, 0.5 * (om_e[rc] + om_e[mc]), torch.where(r_ok, om_e[rc], zero))
    z = torch.where(r_ok, (noise(seed, step, P, defect != "noise_without_step") + omega) / tau, zero)
    m = torch.sigmoid(z)
    mask = k["mask"].double().clone()
    mask[rep[r_ok]] = m[r_ok]
    if defect != "mate_not_written":
        mask[mate[t_ok]] = m[t_ok]
    terms = torch.zeros(B, 2, dtype=torch.float64)
    terms[:, 0].index_add_(0, gid[r_ok], m[r_ok])
    terms[:, 1].index_add_(0, gid[r_ok], MO.entropy(z)[r_ok])
    return omega, z, mask, terms


def backward_formula(k, z, gmask, tau, l_size, l_ent, defect=None):
    """``cal_edge_mlp_bwd`` in fp64 -> ``(dpq [N, 2 Hd], dw2 [Hd], db2 [1])``; ``z`` [P] and ``gmask`` [E] as the kernel gets them."""
    tau, l_size, l_ent = f32(tau), f32(l_size), f32(l_ent)
    rep, mate, r_ok, t_ok, gid, cnt = _tables(k)
    E, N, Hd = k["E"], k["N"], k["Hd"]
    z, g = z.double(), gmask.double()
    m = torch.sigmoid(z)
    rc, mc = rep.clamp(0, E - 1), mate.clamp(0, E - 1)
    sign = 1.0 if defect == "entropy_sign_flipped" else -1.0
    dom = (g[rc] + torch.where(t_ok, g[mc], torch.zeros_like(z)) + l_size + sign * l_ent / cnt * z) * m * (1 - m) / tau
    half = 1.0 if defect == "pair_not_halved" else 0.5
    c = torch.zeros(E, dtype=torch.float64)
    c[rep[r_ok]] = torch.where(t_ok, half * dom, dom)[r_ok]
    c[mate[t_ok]] = (half * dom)[t_ok]
    h = _hidden(k, defect)
    w2 = k["w2"].double()
    ind = torch.ones_like(h) if defect == "relu_dropped" else (h > 0).double()
    row, col = k["row"].long(), k["col"].long()
    dpq = torch.zeros(N, 2 * Hd, dtype=torch.float64)
    dpq[:, :Hd].index_add_(0, row, c[:, None] * w2 * ind)
    dpq[:, Hd:].index_add_(0, row if defect == "q_from_source_row" else col, c[:, None] * w2 * ind)
    return dpq, (c[:, None] * h * ind).sum(0), c.sum().view(1)


def composed_loss(k, pq, w2, b2, gmask, tau, seed, step, l_size, l_ent):
    """The same quantities from torch ops on fp64 leaves ``pq``, ``w2``, ``b2`` (for autograd): ``<gmask, mask> + l_size sum m +
    l_ent / P_g sum H(m)``, H = softplus(z) - z sigma(z)."""
    rep, mate, r_ok, t_ok, gid, cnt = _tables(k)
    Hd = k["Hd"]
    row, col = k["row"].long(), k["col"].long()
    om_e = b2 + F.relu(pq[row, :Hd] + pq[col, Hd:]) @ w2
    rp, tp = rep[r_ok], mate[t_ok]
    omega = om_e[rp]
    pair = t_ok[r_ok]
    omega = torch.where(pair, 0.5 * (omega + om_e[mate.clamp(0, k["E"] - 1)[r_ok]]), omega)
    z = (noise(seed, step, k["P"])[r_ok] + omega) / f32(tau)
    m = torch.sigmoid(z)
    H = F.softplus(z) - z * m                                  # (the logarithm form is 0 x inf on the saturated edges)
    g = gmask.double()
    return (g[rp] * m).sum() + (g[tp] * m[pair]).sum() + f32(l_size) * m.sum() + (f32(l_ent) / cnt[r_ok] * H).sum()


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------
KERNEL_HD = (4, 16, 64, 100, 256)
#: (tau, seed, step): every temperature, no noise and noise, the noise at two steps
KERNEL_DRAWS = ((5.0, 0, 0), (2.0, 11, 0), (1.0, 11, 5), (1.0, 0, 0))
KERNEL_CASES = tuple((hd, d) for hd in KERNEL_HD for d in KERNEL_DRAWS)
KERNEL_COEFFS = (0.05, 1.0)                                    # (l_size, l_ent): the defaults
KERNEL_OUTPUTS = ("omega", "z", "mask", "terms", "dpq", "dw2", "db2")
#: 8 x the measured maxima of the module docstring
KERNEL_ATOL = dict(omega=8 * 3.76e-4, z=8 * 3.76e-4, mask=8 * 3.48e-7, terms=8 * 1.01e-6, dpq=8 * 1.31e-7, dw2=8 * 2.45e-7,
                   db2=8 * 3.09e-7)
_KERNEL = {}


def kernel_inputs(Hd):
    """The shared inputs at hidden width ``Hd`` (computed once, not to be changed).  200 nodes in B = 5 graphs (80 + 4 x 30), about
    1000 columns in shuffled order: random undirected edges, node 0 joined to nodes 1 .. 70 both ways (in- and out-degree above
    64), the last four nodes of every graph without a column, a self-loop column (85, 85), up to 20 one-way columns.  Players: one per
    undirected edge (``rep`` the lower column, ``mate`` the other) or one-way column or self loop, grouped by graph; every seventh
    edge is no player, so non-player columns sit between players; graph 4 has columns and no player; player 3 has its ``rep`` and
    player 9 its ``mate`` out of range.  ``pq``: for 60 columns one hidden unit is exactly 0; the edges (81, 82) and (83, 84)
    have ``omega`` = b2 +- 400 (|z| = 80 at tau = 5 and far beyond at tau = 1)."""
    if Hd in _KERNEL:
        return _KERNEL[Hd]
    g = torch.Generator().manual_seed(100 + Hd)
    sizes = (80, 30, 30, 30, 30)
    N, B = sum(sizes), len(sizes)
    start = [0, 80, 110, 140, 170]
    pairs, oneway = [], []
    for b, (s, n) in enumerate(zip(start, sizes)):
        want = 90 if b else 60
        seen = set()
        while len(seen) < want:
            u, v = (int(t) for t in torch.randint(1 if b == 0 else 0, n - 4, (2,), generator=g))
            if u != v and (min(u, v), max(u, v)) not in seen and not (b == 2 and min(u, v) < 5):
                seen.add((min(u, v), max(u, v)))
        pairs += [(s + u, s + v, b) for u, v in sorted(seen)]
        for _ in range(4):
            u, v = (int(t) for t in torch.randint(0, n - 4, (2,), generator=g))
            if u != v and (min(u, v), max(u, v)) not in seen and (b != 0 or min(u, v) > 0) and not (b == 2 and min(u, v) < 5):
                oneway.append((s + u, s + v, b))
    pairs += [(0, v, 0) for v in range(1, 71)]
    pairs += [(111, 112, 2), (113, 114, 2)]                               # the two saturated edges (graph 2's nodes 1 .. 4)
    cols = [(u, v, b, i) for i, (u, v, b) in enumerate(pairs)] + [(v, u, b, i) for i, (u, v, b) in enumerate(pairs)]
    cols += [(u, v, b, len(pairs) + i) for i, (u, v, b) in enumerate(oneway)] + [(85, 85, 1, len(pairs) + len(oneway))]
    perm = torch.randperm(len(cols), generator=g).tolist()
    cols = [cols[i] for i in perm]
    E = len(cols)
    row = torch.tensor([c[0] for c in cols], dtype=torch.int32)
    col = torch.tensor([c[1] for c in cols], dtype=torch.int32)
    by_edge = {}
    for e, c in enumerate(cols):
        by_edge.setdefault((c[2], c[3]), []).append(e)
    players = []                                                          # (graph, rep, mate)
    for (b, i), es in by_edge.items():
        sat = i < len(pairs) and pairs[i][:2] in ((111, 112), (113, 114))
        if b == 4 or (i % 7 == 3 and not sat):
            continue
        players.append((b, es[0], es[1] if len(es) > 1 else -1))
    players.sort()
    P = len(players)
    pptr = torch.zeros(B + 1, dtype=torch.long)
    for b, _, _ in players:
        pptr[b + 1:] += 1
    rep = torch.tensor([p[1] for p in players], dtype=torch.int32)
    mate = torch.tensor([p[2] for p in players], dtype=torch.int32)
    assert int(mate[9]) >= 0
    rep[3], mate[9] = E + 3, E
    csr = []
    for key in (row, col):
        ptr = torch.zeros(N + 1, dtype=torch.int32)
        ptr[1:] = torch.cumsum(torch.bincount(key.long(), minlength=N), 0)
        csr += [ptr, torch.argsort(key.long(), stable=True).to(torch.int32)]
    w2 = torch.randn(Hd, generator=g)
    w2 = torch.where(w2.abs() < 0.05, torch.full_like(w2, 0.05), w2)
    b2 = torch.tensor([0.3])
    pq = torch.randn(N, 2 * Hd, generator=g) * (2.0 / math.sqrt(Hd))
    for j, (sgn, a, b) in enumerate(((1.0, 111, 112), (-1.0, 113, 114))):
        use = (w2 * sgn) > 0
        if not bool(use.any()):
            use = torch.ones(Hd, dtype=torch.bool)
        hval = torch.where(use, 400.0 * sgn / (float(use.sum()) * w2), torch.full_like(w2, -1.0))
        pq[a, :Hd] = pq[b, :Hd] = 0.5 * hval
        pq[a, Hd:] = pq[b, Hd:] = 0.5 * hval
    for e in range(0, E, E // 60):
        u, v = int(row[e]), int(col[e])
        if len({u, v} & {111, 112, 113, 114}) == 0:
            pq[v, Hd + e % Hd] = -pq[u, e % Hd]
    k = dict(Hd=Hd, N=N, E=E, B=B, P=P, row=row, col=col, pptr=pptr, rep=rep, mate=mate, pq=pq, w2=w2, b2=b2,
             rowptr_src=csr[0], eid_src=csr[1], rowptr_dst=csr[2], eid_dst=csr[3],
             mask=torch.rand(E, generator=g) + 2.0,                         # prior bits no sigmoid produces
             gmask=torch.randn(E, generator=g) * 0.05)
    _KERNEL[Hd] = k
    return k


def kernel_want(case, defect=None):
    """-> the seven outputs of ``KERNEL_OUTPUTS`` for one case; the backward is taken at the forward's z rounded to fp32 (what the
    kernel is handed) -- the formula's own z, so a defect of the forward shows in the forward's outputs."""
    Hd, (tau, seed, step) = case
    key = ("want", case, defect)
    if key not in _KERNEL:
        k = kernel_inputs(Hd)
        fwd = forward_formula(k, tau, seed, step, defect)
        z32 = kernel_z(case)
        _KERNEL[key] = fwd + backward_formula(k, z32, k["gmask"], tau, *KERNEL_COEFFS, defect=defect)
    return _KERNEL[key]


def kernel_z(case):
    """The fp32 z every backward of ``case`` is run at (the defect-free formula's, rounded)."""
    Hd, (tau, seed, step) = case
    key = ("z", case)
    if key not in _KERNEL:
        _KERNEL[key] = forward_formula(kernel_inputs(Hd), tau, seed, step)[1].float()
    return _KERNEL[key]


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


# ---- the free-running training loop ----------------------------------------------------------------------------------------------
TRAIN_STEPS = 4
TRAIN_HD = 8
TRAIN_KW = dict(lr=0.003, temp=(5.0, 2.0), size_coeff=0.05, ent_coeff=1.0, seed=1)
#: (undirected, subset of the columns, head): directed, undirected pairs, a subset, the co head
TRAIN_CASES = ((None, False, "o"), ("mean", False, "o"), ("mean", True, "o"), ("mean", False, "co"))
#: the measured |fp32 host path - oracle| per model (module docstring); the tolerance is 4 x that
MODEL_MAX = {"CausalGCN": dict(params=4.92e-8, omega=2.16e-7, mask=8.21e-8, p_masked=8.28e-8, loss=3.54e-7),
             "CausalGAT": dict(params=4.81e-8, omega=2.17e-7, mask=7.70e-8, p_masked=4.54e-8, loss=2.07e-7),
             "CausalGIN": dict(params=2.39e-8, omega=5.30e-7, mask=5.00e-8, p_masked=3.35e-8, loss=1.17e-7)}
MODEL_ATOL = {n: {k: 4 * v for k, v in d.items()} for n, d in MODEL_MAX.items()}
RELU_MARGIN = 1e-4
GRAD_MARGIN = 1e-6
#: model -> (seed of ``softmask_oracle.model_state``, seed of the explainer's initialisation) at which both conditions hold for
#: every case (searched on the CPU, on the oracle alone)
TRAIN_SEED = {"CausalGCN": (113, 0), "CausalGAT": (179, 2), "CausalGIN": (196, 1)}
_TRAIN = {}


def init_state(H, Hd, seed):
    """The explainer's initial parameters as ``torch.nn.Linear`` draws them (uniform in +- 1 / sqrt(fan_in)) from a generator
    seeded with ``seed``, in the order lin1.weight, lin1.bias, lin2.weight, lin2.bias."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, (o, i) in (("lin1", (Hd, 2 * H)), ("lin2", (1, Hd))):
        b = 1.0 / math.sqrt(i)
        out[name + ".weight"] = torch.empty(o, i).uniform_(-b, b, generator=g)
        out[name + ".bias"] = torch.empty(o).uniform_(-b, b, generator=g)
    return out


def embeddings(name, sd, x, edge_index, track, layers=2, heads=4):
    """The backbone output at ``m = 1`` (the rows ``edge_att_mlp`` reads): the first lines of ``softmask_oracle.masked_forward``."""
    m = torch.ones(edge_index.size(1), dtype=x.dtype)
    x = O._bn(x, sd, "bn_feat", False)
    x = track.relu(O.gcn_conv(x, edge_index, sd["conv_feat.weight"], sd["conv_feat.bias"], gfn=True))
    for i in range(layers):
        if name == "CausalGCN":
            x = track.relu(O.gcn_conv(O._bn(x, sd, f"bns_conv.{i}", False), edge_index, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], m))
        elif name == "CausalGAT":
            x = track.relu(SO.gat_conv_masked(O._bn(x, sd, f"bns_conv.{i}", False), edge_index, sd[f"convs.{i}.weight"],
                                              sd[f"convs.{i}.att"], sd[f"convs.{i}.bias"], heads, m))
        else:
            x = SO.gin_conv_masked(x, edge_index, sd, f"convs.{i}.", m, track)
    return x


def temperature(t, total, temp):
    return f32(temp[0] * (temp[1] / temp[0]) ** (min(t, total - 1) / max(total - 1, 1)))


def oracle_train(name, case, steps=TRAIN_STEPS, Hd=TRAIN_HD, data=None, key=None, train=True):
    """The trainer in fp64 on ``softmask_oracle.model_batch()`` (or ``data``) -> dict(params, history [steps, B, 3], omega, mask,
    yhat, p_full, p_masked, rep, mate, gid, min_pre, min_grad); computed once per ``(name, case, steps, key)``.  ``train=False``:
    the explanation of the initial parameters."""
    ck = (name, case, steps if train else 0, key)
    if ck in _TRAIN:
        return _TRAIN[ck]
    undirected, subset, head = case
    kw = TRAIN_KW
    lr, l_size, l_ent = kw["lr"], f32(kw["size_coeff"]), f32(kw["ent_coeff"])
    data = SO.model_batch() if data is None else data
    mseed, eseed = TRAIN_SEED[name]
    sd64 = {k: v.double() for k, v in SO.model_state(name, data.feat.size(1), seed=mseed).items()}
    E, B, h = data.edge_index.size(1), data.num_graphs, ("c", "o", "co").index(head)
    rep, mate, pg, member = MO.players_of(data, "edges", undirected, SO.subset_of(E) if subset else None)
    P = rep.numel()
    pair = mate >= 0
    cnt = torch.zeros(B, dtype=torch.float64).index_add_(0, pg, torch.ones(P, dtype=torch.float64))
    track = SO.Track()
    with torch.no_grad():
        x = embeddings(name, sd64, data.feat.double(), data.edge_index, track)
        lp = SO.oracle_forward(name, sd64, data)("edges")(torch.ones(E, dtype=torch.float64))[h]
    yhat = lp.argmax(-1)
    p_full = lp.gather(-1, yhat.view(-1, 1)).view(-1).exp()
    row, col = data.edge_index
    xe = torch.cat([x[row], x[col]], -1)
    params = [v.double() for v in init_state(x.size(1), Hd, eseed).values()]

    def sample(params, tau, eps):
        W1, b1, W2, b2 = params
        om_e = F.linear(track.relu(F.linear(xe, W1, b1)), W2, b2).view(-1)
        omega = torch.where(pair, 0.5 * (om_e[rep] + om_e[mate.clamp(min=0)]), om_e[rep])
        m = torch.sigmoid((eps + omega) / tau)
        mask = torch.ones(E, dtype=torch.float64).index_put((rep,), m).index_put((mate[pair],), m[pair])
        return omega, m, mask

    fwd = SO.oracle_forward(name, sd64, data)("edges", track)
    m1, m2 = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    history, min_grad = [], float("inf")
    for t in range(steps if train else 0):
        leaves = [p.clone().requires_grad_(True) for p in params]
        _, m, mask = sample(leaves, temperature(t, steps, kw["temp"]), noise(kw["seed"], t, P))
        pred = -fwd(mask)[h].gather(-1, yhat.view(-1, 1)).view(-1)
        H = -m * m.log() - (1 - m) * (1 - m).log()
        size = l_size * torch.zeros(B, dtype=torch.float64).index_add(0, pg, m)
        ent = l_ent * torch.zeros(B, dtype=torch.float64).index_add(0, pg, H) / cnt.clamp(min=1.0)
        rows = torch.stack([pred, size, ent], -1)
        grads = torch.autograd.grad(rows.sum(), leaves)
        history.append(rows.detach())
        s = t + 1
        for i, g in enumerate(grads):
            nz = g[g != 0]
            if nz.numel():
                min_grad = min(min_grad, nz.abs().min().item())
            m1[i], m2[i] = 0.9 * m1[i] + 0.1 * g, 0.999 * m2[i] + 0.001 * g * g
            params[i] = params[i] - lr / (1 - 0.9 ** s) * m1[i] / (m2[i].sqrt() / math.sqrt(1 - 0.999 ** s) + 1e-8)
    with torch.no_grad():
        omega, m, mask = sample(params, 1.0, torch.zeros(P, dtype=torch.float64))
        p_masked = SO.oracle_forward(name, sd64, data)("edges", track)(mask)[h].gather(-1, yhat.view(-1, 1)).view(-1).exp()
    nan = torch.full((E,), float("nan"), dtype=torch.float64)
    om = nan.index_put((rep,), omega).index_put((mate[pair],), omega[pair])
    _TRAIN[ck] = dict(params=params, history=torch.stack(history) if history else None, omega=om,
                      mask=torch.where(member, mask, nan), yhat=yhat, p_full=p_full, p_masked=p_masked, rep=rep, mate=mate, gid=pg,
                      min_pre=track.min_pre, min_grad=min_grad)
    return _TRAIN[ck]
