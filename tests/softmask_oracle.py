"""Plain-torch restatement of the soft-mask forward on top of ``oracle.cal_oracle``'s pieces -- TEST
INFRASTRUCTURE.  Run it in fp64.  With autograd it gives the oracle saliency and the oracle integrated gradients at a given number
of steps; every ReLU reports its smallest |pre-activation| so a test can rule out fp32 sign flips.

Semantics restated here, independently of cal_amd: a mask value ``m_e >= 0`` per edge column enters every convolution -- GCNConv as
``edge_weight`` (times the edge attention in the two head convolutions), GINConv as the weight of its sum, GATConv inside the edge
softmax (max over the loop and the columns with ``m > 0``, detached) -- the added self loop always weighs 1, and a node mask puts
``n_u n_v`` on column (u, v) and scales the node's rows before the add-pool.
"""
import torch
import torch.nn.functional as F

from oracle import cal_oracle as O


class Track:
    """Smallest |pre-activation| over every ReLU of the forwards it saw."""

    def __init__(self):
        self.min_pre = float("inf")

    def relu(self, x):
        if x.numel():
            self.min_pre = min(self.min_pre, float(x.detach().abs().min()))
        return F.relu(x)


def gat_conv_masked(x, edge_index, weight, att, bias, heads, m, negative_slope=0.2):
    n = x.size(0)
    x = torch.matmul(x, weight)
    row, col = edge_index
    keep = row != col
    ei, _ = O.add_self_loops(edge_index[:, keep], n)
    mm = torch.cat([m[keep], torch.ones(n, dtype=x.dtype)])
    row, col = ei
    d = weight.size(1) // heads
    x_i = x.index_select(0, col).view(-1, heads, d)
    x_j = x.index_select(0, row).view(-1, heads, d)
    e = F.leaky_relu((torch.cat([x_i, x_j], dim=-1) * att).sum(dim=-1), negative_slope)          # [E', heads]
    live = (mm > 0).view(-1, 1).expand_as(e)
    idx = col.view(-1, 1).expand_as(e)
    mx = torch.full((n, heads), float("-inf"), dtype=x.dtype)
    mx = mx.scatter_reduce(0, idx, torch.where(live, e, torch.full_like(e, float("-inf"))).detach(), reduce="amax", include_self=True)
    u = mm.view(-1, 1) * (e - mx.index_select(0, col)).exp()
    den = O.scatter_add(u, col, n).index_select(0, col) + 1e-16
    alpha = u / den
    out = O.scatter_add((x_j * alpha.view(-1, heads, 1)).reshape(-1, heads * d), col, n)
    return out if bias is None else out + bias


def gin_conv_masked(x, edge_index, sd, prefix, m, track, eps=0.0):
    row, col = edge_index
    keep = row != col
    out = (1 + eps) * x + O.propagate_add(edge_index[:, keep], x, m[keep])
    out = F.linear(out, sd[prefix + "nn.0.weight"], sd[prefix + "nn.0.bias"])
    out = track.relu(O._bn(out, sd, prefix + "nn.1", False))
    return track.relu(F.linear(out, sd[prefix + "nn.3.weight"], sd[prefix + "nn.3.bias"]))


def _readout(x, sd, tag, track):
    x = O._bn(x, sd, f"fc1_bn_{tag}", False)
    x = track.relu(F.linear(x, sd[f"fc1_{tag}.weight"], sd[f"fc1_{tag}.bias"]))
    x = O._bn(x, sd, f"fc2_bn_{tag}", False)
    return F.log_softmax(F.linear(x, sd[f"fc2_{tag}.weight"], sd[f"fc2_{tag}.bias"]), dim=-1)


def masked_forward(model, sd, x, edge_index, batch, num_graphs, *, edge_mask=None, node_mask=None, layers=2, heads=4,
                   cat_or_add="add", without_node_attention=False, without_edge_attention=False, track=None):
    """Eval-mode causal forward with the identity permutation under the masks -> ``(c, o, co)`` log-probs."""
    track = Track() if track is None else track
    if model != "CausalGCN":
        without_node_attention = without_edge_attention = False
    row, col = edge_index
    m = torch.ones(edge_index.size(1), dtype=x.dtype) if edge_mask is None else edge_mask
    if node_mask is not None:
        m = m * node_mask[row] * node_mask[col]
    x = O._bn(x, sd, "bn_feat", False)
    x = track.relu(O.gcn_conv(x, edge_index, sd["conv_feat.weight"], sd["conv_feat.bias"], gfn=True))
    for i in range(layers):
        if model == "CausalGCN":
            x = O._bn(x, sd, f"bns_conv.{i}", False)
            x = track.relu(O.gcn_conv(x, edge_index, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], m))
        elif model == "CausalGAT":
            x = O._bn(x, sd, f"bns_conv.{i}", False)
            x = track.relu(gat_conv_masked(x, edge_index, sd[f"convs.{i}.weight"], sd[f"convs.{i}.att"], sd[f"convs.{i}.bias"],
                                           heads, m))
        else:
            x = gin_conv_masked(x, edge_index, sd, f"convs.{i}.", m, track)
    if without_edge_attention:
        edge_att = 0.5 * torch.ones(edge_index.size(1), 2, dtype=x.dtype)
    else:
        edge_att = F.softmax(F.linear(torch.cat([x[row], x[col]], dim=-1), sd["edge_att_mlp.weight"], sd["edge_att_mlp.bias"]), dim=-1)
    if without_node_attention:
        node_att = 0.5 * torch.ones(x.shape[0], 2, dtype=x.dtype)
    else:
        node_att = F.softmax(F.linear(x, sd["node_att_mlp.weight"], sd["node_att_mlp.bias"]), dim=-1)
    xc = node_att[:, 0].view(-1, 1) * x
    xo = node_att[:, 1].view(-1, 1) * x
    xc = track.relu(O.gcn_conv(O._bn(xc, sd, "bnc", False), edge_index, sd["context_convs.weight"], sd["context_convs.bias"],
                               edge_att[:, 0] * m))
    xo = track.relu(O.gcn_conv(O._bn(xo, sd, "bno", False), edge_index, sd["objects_convs.weight"], sd["objects_convs.bias"],
                               edge_att[:, 1] * m))
    if node_mask is not None:
        xc, xo = xc * node_mask.view(-1, 1), xo * node_mask.view(-1, 1)
    xc_p = O.global_add_pool(xc, batch, num_graphs)
    xo_p = O.global_add_pool(xo, batch, num_graphs)
    xco = torch.cat((xc_p, xo_p), dim=1) if cat_or_add == "cat" else xc_p + xo_p
    return _readout(xc_p, sd, "c", track), _readout(xo_p, sd, "o", track), _readout(xco, sd, "co", track)


def remove_nodes(x, edge_index, batch, keep):
    """The batch without the nodes outside ``keep`` (bool [N]), densely renumbered; a column stays iff both endpoints stay."""
    new = torch.cumsum(keep.long(), 0) - 1
    row, col = edge_index
    ek = keep[row] & keep[col]
    return x[keep], torch.stack([new[row[ek]], new[col[ek]]]), batch[keep]


def attribution(forward, M, gid, B, *, head=1, member=None, twin=None, steps=None):
    """Oracle saliency (``steps=None``) or midpoint-rule integrated gradients of ``forward(mask fp64 [M]) -> (c, o, co)``.
    -> dict(score, p_full, p_baseline, yhat, gap)."""
    member = torch.ones(M, dtype=torch.bool) if member is None else member.clone()
    idx = torch.arange(M)
    paired = None
    if twin is not None:
        t = twin.clamp(min=0).long()
        paired = (twin >= 0) & (t != idx)
        member = member | (member[t] & paired)

    def p_at(alpha, yhat=None, grad=False):
        m = torch.where(member, torch.full((M,), float(alpha), dtype=torch.float64), torch.ones(M, dtype=torch.float64))
        m.requires_grad_(grad)
        lp = forward(m)[head]
        yhat = lp.argmax(-1) if yhat is None else yhat
        p = lp.gather(-1, yhat.view(-1, 1)).view(-1).exp()
        if not grad:
            return p.detach(), yhat, None
        (g,) = torch.autograd.grad(p.sum(), m, allow_unused=True)
        return p.detach(), yhat, torch.zeros(M, dtype=torch.float64) if g is None else g

    if steps is None:
        p_full, yhat, g = p_at(1.0, grad=True)
        p_base = None
    else:
        p_full, yhat, _ = p_at(1.0)
        p_base = p_at(0.0, yhat)[0]
        g = torch.zeros(M, dtype=torch.float64)
        for s in range(1, steps + 1):
            g += p_at((s - 0.5) / steps, yhat, grad=True)[2]
        g /= steps
    if paired is not None:
        g = torch.where(paired, g + g[t], g)
    score = torch.where(member, g, torch.full_like(g, float("nan")))
    gap = None
    if steps is not None:
        rep = member if paired is None else member & ~(paired & (t < idx))
        sums = torch.zeros(B, dtype=torch.float64).index_add_(0, gid, torch.where(rep, score, torch.zeros_like(score)))
        gap = sums - (p_full - p_base)
    return dict(score=score, p_full=p_full, p_baseline=p_base, yhat=yhat, gap=gap)


# ---- shared cases of tests/test_softmask.py (host twins) and tests/test_gpu_softmask.py (HIP) ------------------------------------
#: out / dz as tests/test_gpu_ops.py holds cal_gat_fwd / cal_gat_bwd to the oracle; dm and cal_edge_dot as the dw of its
#: test_gcn_aggregate_fwd_bwd (cal_gcn_norm_bwd)
TOL_OUT = dict(atol=5e-5, rtol=1e-4)
TOL_DZ = dict(atol=1e-4, rtol=1e-3)
TOL_DW = dict(atol=5e-5, rtol=1e-3)
EDGE_DOT_H = (1, 5, 64, 132)
GAT_SHAPES = ((1, 32), (4, 32), (4, 64), (2, 8), (3, 4))


def kernel_graph(hub_deg, n=None, seed=0):
    """-> (edge_index [2, E], N, facts).  Node 0 is a destination of in-degree ``hub_deg`` (sources 1 .. hub_deg, one of them
    twice: a duplicated column), node N - 1 is isolated, node N - 2 receives three columns (the all-masked destination of the
    GAT cases), (3, 3) is a self-loop column, the rest random."""
    g = torch.Generator().manual_seed(seed)
    n = hub_deg + 8 if n is None else n
    src = list(range(1, hub_deg)) + [1]                        # hub_deg columns into node 0, column (1, 0) twice
    dst = [0] * hub_deg
    extra = torch.randint(0, n - 2, (2, 2 * n), generator=g)
    keep = extra[0] != extra[1]
    src += extra[0][keep].tolist()
    dst += extra[1][keep].tolist()
    src += [3, 4, 5, 6]
    dst += [3, n - 2, n - 2, n - 2]
    ei = torch.tensor([src, dst], dtype=torch.long)
    perm = torch.randperm(ei.size(1), generator=g)
    ei = ei[:, perm].contiguous()
    facts = dict(hub=0, isolated=n - 1, dark=n - 2, loop=int(((ei[0] == 3) & (ei[1] == 3)).nonzero()[0]))
    return ei, n, facts


def kernel_mask(ei, facts, seed=0):
    """Masks drawn from {0, 1, uniform}, all 0 into the ``dark`` destination."""
    g = torch.Generator().manual_seed(100 + seed)
    E = ei.size(1)
    m = torch.rand(E, generator=g)
    pick = torch.randint(0, 3, (E,), generator=g)
    m = torch.where(pick == 0, torch.zeros(E), torch.where(pick == 1, torch.ones(E), m))
    m[ei[1] == facts["dark"]] = 0.0
    return m


def edge_dot_case(H, seed=0):
    """-> (ei, N, facts, a, b, want fp64 [E])."""
    ei, n, facts = kernel_graph(70, seed=seed)
    g = torch.Generator().manual_seed(200 + H)
    a, b = torch.randn(n, H, generator=g), torch.randn(n, H, generator=g)
    want = (a.double()[ei[1]] * b.double()[ei[0]]).sum(-1)
    want[ei[0] == ei[1]] = 0.0
    return ei, n, facts, a, b, want


def gin_weight_grad_oracle(x, ei, w, gout, eps=0.0):
    """d/dw and d/dx of <gout, (1 + eps) x + sum_j w_ji x_j> by autograd (fp64)."""
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    keep = ei[0] != ei[1]
    out = (1 + eps) * x + O.propagate_add(ei[:, keep], x, w[keep])
    gx, gw = torch.autograd.grad((out * gout.double()).sum(), (x, w))
    return out.detach(), gx, gw


def gat_case(K, D, relu=True, seed=0):
    """-> dict of the inputs (fp32) and the fp64 oracle's out, dz, dm for a masked GATConv on ``kernel_graph(130)``."""
    ei, n, facts = kernel_graph(131, seed=seed)
    g = torch.Generator().manual_seed(300 + 7 * K + D)
    H = K * D
    z = torch.randn(n, H, generator=g) * 0.5
    att = torch.randn(1, K, 2 * D, generator=g) * 0.3
    bias = torch.randn(H, generator=g)
    m = kernel_mask(ei, facts, seed)
    gout = torch.randn(n, H, generator=g)
    zd, md = z.double().requires_grad_(True), m.double().requires_grad_(True)
    ref = gat_conv_masked(zd, ei, torch.eye(H, dtype=torch.float64), att.double(), bias.double(), K, md)
    ref = torch.relu(ref) if relu else ref
    dz, dm = torch.autograd.grad((ref * gout.double()).sum(), (zd, md))
    return dict(ei=ei, N=n, facts=facts, z=z, att=att, bias=bias, m=m, gout=gout, relu=relu, out=ref.detach(), dz=dz, dm=dm)


# ---- model-level cases -------------------------------------------------------------------------------------------------------------
MODELS = ("CausalGCN", "CausalGAT", "CausalGIN")
#: atol of a gradient score per model: 4 x the largest |fp32 host path - fp64 oracle| over every model-level case of
#: tests/test_softmask.py (measured maxima in that module's docstring); rtol 1e-3
SCORE_ATOL = {"CausalGCN": 4 * 1.8e-8, "CausalGAT": 4 * 8.7e-9, "CausalGIN": 4 * 5.9e-8}
SCORE_RTOL = 1e-3
#: the feature layer's weight is scaled up and the heads' last layers down by as much: a ReLU network is positively homogeneous
#: up to its biases, so the logits keep their size while every pre-activation sits PRE_SCALE times further from its kink (the
#: chance that ~50 000 of them all stay 1e-4 away from 0 is otherwise below 1e-3 per seed; the fp32 error of a pre-activation
#: grows with the factor too, to ~1e-5 at activations of ~10, still a tenth of the margin); HEAD_SCALE then opens up the nearly
#: flat random-init heads
#: (CausalGIN's torch.nn.Linear layers shrink their input layer by layer, so it takes a larger factor)
PRE_SCALE = {"CausalGCN": 4.0, "CausalGAT": 4.0, "CausalGIN": 16.0}
HEAD_SCALE = 2.0


class _Foreign:
    pass


def model_batch():
    """Three small random undirected graphs (5 to 7 nodes, 10 features) with one self-loop column (0, 0) in front and one
    column without a twin behind, as a plain object (x / feat / edge_index / batch / num_graphs): the layout is derived as for
    any foreign input.  Small on purpose: every ReLU of every differentiated forward has to stay 1e-4 away from its kink, and the
    chance of that falls exponentially with the number of activations (the large shapes are the kernel-level cases')."""
    from tests.helpers import random_graph_batch
    b = random_graph_batch(3, n_lo=5, n_hi=7, p=0.4, feat=10, seed=12)
    n = int(b.batch.numel())
    last = (b.batch == b.num_graphs - 1).nonzero().view(-1)
    a, c = int(last[0]), int(last[-1])
    has = bool(((b.edge_index[0] == a) & (b.edge_index[1] == c)).any())
    extra = torch.tensor([[a], [c]]) if not has else torch.tensor([[a], [int(last[1])]])
    f = _Foreign()
    f.x, f.feat, f.batch, f.num_graphs, f.y = None, b.x, b.batch, b.num_graphs, b.y
    f.edge_index = torch.cat([torch.zeros(2, 1, dtype=torch.long), b.edge_index, extra], 1).contiguous()
    assert n == f.feat.size(0)
    return f


def to_device(f, dev):
    g = _Foreign()
    for k, v in f.__dict__.items():
        if k != "_plan":
            setattr(g, k, v.to(dev) if torch.is_tensor(v) else v)
    return g


#: seeds of ``model_state`` at which the two conditions of test_the_gradient_checks_are_not_vacuous hold (searched on the CPU,
#: on the oracle alone)
MODEL_SEED = {"CausalGCN": 7, "CausalGAT": 5, "CausalGIN": 120}


def model_state(name, feat, hidden=32, heads=4, seed=None):
    """Random-init state with random BatchNorm statistics, the feature layer scaled up by PRE_SCALE and the last layers of the
    heads scaled by HEAD_SCALE / PRE_SCALE."""
    seed = MODEL_SEED[name] if seed is None else seed
    torch.manual_seed(seed)
    sd = O.init_state(name, feat, 4, hidden=hidden, layers=2, heads=heads)
    g = torch.Generator().manual_seed(seed + 50)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.3
        if k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    sd["conv_feat.weight"] = sd["conv_feat.weight"] * PRE_SCALE[name]
    for tag in ("c", "o", "co"):
        sd[f"fc2_{tag}.weight"] = sd[f"fc2_{tag}.weight"] * (HEAD_SCALE / PRE_SCALE[name])
    return sd


def build_model(name, sd, feat, hidden=32, heads=4):
    import argparse

    from cal_amd import model as M
    args = argparse.Namespace(layers=2, hidden=hidden, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add")
    m = M.CausalGAT(feat, 4, args, head=heads) if name == "CausalGAT" else getattr(M, name)(feat, 4, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")
    return m


def oracle_forward(name, sd64, data, heads=4):
    """mask -> log-probs closures of the oracle over ``data`` (CPU tensors): ``fwd(use)(mask fp64)``."""
    x = (data.x if data.x is not None else data.feat).double()

    def fwd(use, track=None):
        key = "edge_mask" if use == "edges" else "node_mask"
        return lambda mk: masked_forward(name, sd64, x, data.edge_index, data.batch, data.num_graphs, heads=heads, track=track,
                                         **{key: mk})
    return fwd


#: the model-level cases: (use, undirected, subset of the elements, head)
SCORE_CASES = (("edges", None, False, "o"), ("edges", "mean", False, "o"), ("nodes", None, False, "o"),
               ("edges", "max", True, "o"), ("nodes", None, False, "co"))
_CACHE = {}


def subset_of(M):
    return torch.rand(M, generator=torch.Generator().manual_seed(2)) < 0.4


def oracle_scores(name, case, steps):
    """The oracle's attribution for one model-level case (computed once per process) -> (dict, smallest ReLU |pre-activation|)."""
    key = (name, case, steps)
    if key not in _CACHE:
        from cal_amd.explain import edge_twins
        use, undirected, subset, head = case
        data = model_batch()
        feat = data.feat.size(1)
        sd64 = {k: v.double() for k, v in model_state(name, feat).items()}
        track = Track()
        M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
        gid = data.batch[data.edge_index[0]] if use == "edges" else data.batch
        twin = edge_twins(data)[0] if undirected else None
        res = attribution(oracle_forward(name, sd64, data)(use, track), M, gid, data.num_graphs, head=("c", "o", "co").index(head),
                          member=subset_of(M) if subset else None, twin=twin, steps=steps)
        _CACHE[key] = (res, track.min_pre)
    return _CACHE[key]
