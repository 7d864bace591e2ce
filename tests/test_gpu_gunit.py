"""The graph-unit staging vocabulary (engine_gunit.hpp) through the engine, for the kernel families whose tile edges and
guard the suite did not reach: the per-graph GAT and GIN layers on units of 1, 2, 31, 32, 33, 63 and 64 nodes (with an
edgeless and a star graph among them), the wide GCN form on units around its 32-row tiles (129 .. 256 nodes), and the
bounds guard of the GAT and GIN kernels.  Every case asserts the launch-site names, so a fall-back to the node-level chain
cannot pass silently."""
import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests.test_gpu_engine import LOGIT_TOL, _args, _ragged_batch, _stage_names
from tests.test_gpu_store_policy import EDGE_SIZES, _state as _gcn_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGES = {"CausalGAT": ("k_ggat_fwd", "k_ggat_bwd"),
          "CausalGIN": ("k_ggin_fwd<1>", "k_ggin_fwd<2>", "k_ggin_bwd<2>", "k_ggin_bwd<1>"),
          "wide": ("k_gw_fwd", "k_gw_bwd")}


def _state(name, hidden, nfeat, ncls, layers, heads=4):
    """test_gpu_store_policy._state for any of the three models: non-trivial biases and BatchNorm weights."""
    if name == "CausalGCN":
        return _gcn_state(hidden, nfeat, ncls, layers)
    sd = O.init_state(name, nfeat, ncls, hidden=hidden, layers=layers, heads=heads)
    g = torch.Generator().manual_seed(7)
    for k in list(sd):
        if k.endswith(".bias") or ("bn" in k and k.endswith(".weight")):
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
    return sd


def _engine(name, sd, args, nfeat, ncls, heads=4):
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    m = getattr(M, name)(nfeat, ncls, args, head=heads) if name == "CausalGAT" else getattr(M, name)(nfeat, ncls, args)
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=name != "CausalGIN")      # (GINConv keeps an `eps` buffer)
    m = m.to(DEV).train()
    if name == "CausalGAT":
        for c in m.convs:
            c.dropout = 0.0
    return m, StepEngine(m, lr=1e-3)


def _step_against_oracle(name, hidden, b, bd, stages, grad_tol, heads=4, absent=()):
    layers, nfeat, ncls = 2, 10, 4
    b.y = b.y % ncls
    bd.y = bd.y % ncls
    B = int(b.y.numel())
    sd = _state(name, hidden, nfeat, ncls, layers, heads)
    m, eng = _engine(name, sd, _args(hidden=hidden, layers=layers), nfeat, ncls, heads)
    perm = torch.randperm(B)
    tr = O.CpuTrainer(name, {k: v.clone() for k, v in sd.items()}, ncls, lr=1e-3, layers=layers, heads=heads, gat_dropout=0.0)
    loss, lc, lo, lco, logits = tr.step(b.x, b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=False).cpu().numpy()
    eng.check_status()
    names = _stage_names()
    for k in stages:
        assert k in names, (k, names)
    for k in absent:
        assert k not in names, (k, names)
    lp = eng.buffer("logp", 3 * B * ncls).view(3, B, ncls).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    atol, rtol = grad_tol
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(p.grad.cpu(), gref, atol=atol, rtol=rtol), k


@pytest.mark.parametrize("name,hidden,heads", [("CausalGAT", 128, 4), ("CausalGAT", 64, 2), ("CausalGAT", 64, 4), ("CausalGIN", 128, 4)],
                         ids=["gat-h128", "gat-h64-2heads", "gat-h64-4heads-node-level", "gin-h128"])
def test_gat_and_gin_units_on_a_tile_edge_match_the_oracle(name, hidden, heads):
    """One and two row tiles, full and one-row tiles, an edgeless unit (the `ne <= 0` repair of the slot batch) and a star
    (a hub row).  Bounds: those of test_step_with_every_policy_store_on_a_tile_edge_matches_the_oracle.
    GAT at hidden 64: the per-graph kernels take heads of 32 or 64 columns (Route, engine.hip), so the reference's four heads
    (16 columns each) go through the node-level chain -- that case is held to the same oracle bounds and asserts that it did
    NOT take k_ggat_* -- and the case that puts all heads of a layer into ONE column slice of the per-graph kernels is hidden
    64 with two heads of 32."""
    torch.manual_seed(hidden + 2)
    b = _ragged_batch(hidden, 10, EDGE_SIZES)
    bd = _ragged_batch(hidden, 10, EDGE_SIZES).to(DEV)
    fused = name != "CausalGAT" or hidden // heads in (32, 64)
    _step_against_oracle(name, hidden, b, bd, STAGES[name] if fused else (), (1e-4, 3e-3), heads,
                         absent=() if fused else STAGES[name])


WIDE_SIZES = [129, 160, 161, 255, 256, 130]              # one row past a 32-row tile, on it, and the kernel's last row


def _wide_batch(seed, nfeat):
    """Graphs inside the bounds of k_gw_* (<= 256 nodes, <= 2048 stored edges): sparse random ones (~6 n directed edges), a
    hub star (index 2) and one with a node without edges (index 3)."""
    from cal_amd.data import Batch, Data
    g = torch.Generator().manual_seed(seed)
    ds = []
    for i, n in enumerate(WIDE_SIZES):
        if i == 2:
            leaves = torch.arange(1, n)
            ei = torch.cat([torch.stack([torch.zeros_like(leaves), leaves]), torch.stack([leaves, torch.zeros_like(leaves)])], 1)
        else:
            a = torch.rand(n, n, generator=g) < 3.0 / n
            a = a | a.t()
            a.fill_diagonal_(False)
            if i == 3:
                a[1, :] = False
                a[:, 1] = False
            ei = a.nonzero().t().contiguous()
        assert ei.shape[1] <= 2048
        ds.append(Data(x=torch.randn(n, nfeat, generator=g), edge_index=ei, y=torch.randint(0, 3, (1,), generator=g)))
    return Batch.from_data_list(ds)


@pytest.mark.parametrize("hidden", [64, 128])
def test_wide_units_on_a_tile_edge_match_the_oracle(hidden):
    """The wide per-graph GCN form on units of 129 .. 256 nodes.  Tolerances: test_config1_shape_takes_the_wide_per_graph_kernels."""
    torch.manual_seed(hidden + 3)
    b, bd = _wide_batch(hidden, 10), _wide_batch(hidden, 10).to(DEV)
    assert 128 < bd.max_nodes <= 256 and bd.max_edges <= 2048
    _step_against_oracle("CausalGCN", hidden, b, bd, STAGES["wide"], (2e-4, 4e-3))


@pytest.mark.parametrize("name", ["CausalGAT", "CausalGIN"])
def test_gat_and_gin_kernels_flag_bad_bounds_and_freeze_the_parameters(name):
    """The second half of test_fused_conv_matches_unfused_and_flags_bad_bounds for the other two families: a 100-node graph
    behind a claimed bound of 50 nodes / 10 edges raises status bit 8, and the Adam step that follows leaves the parameters
    alone (the contract of test_flagged_step_leaves_the_parameters_alone)."""
    torch.manual_seed(11)
    sd = _state(name, 128, 10, 4, 2)
    big = _ragged_batch(128, 10, [100, 20]).to(DEV)
    big.y = big.y % 4
    m, eng = _engine(name, sd, _args(hidden=128, layers=2), 10, 4)
    big.max_nodes, big.max_edges = 50, 10                    # claims the 64-node kernels fit
    eng.train_step(big, torch.arange(2, device=DEV), adam=False)
    assert STAGES[name][0] in _stage_names(), _stage_names()
    assert int(eng.buffer("status", 1, dtype=torch.int32).item()) & 8
    p0 = eng.flat_p.clone()
    eng.train_step(big, torch.arange(2, device=DEV), adam=True)
    assert torch.equal(eng.flat_p, p0)


@pytest.mark.parametrize("name,stage", [("CausalGCN", "k_gconv_fwd"), ("CausalGAT", "k_ggat_fwd")])
def test_edge_from_the_next_graphs_first_node_is_flagged(name, stage):
    """The in-bounds test of the slot batch at its upper edge: one edge into graph 0 whose source is the FIRST node of graph
    1 (local index == the graph's row count) is not a mini-batch edge -- the forward pass raises status bit 16."""
    torch.manual_seed(5)
    sd = _state(name, 128, 10, 4, 2)
    bad = _ragged_batch(128, 10, [33, 20]).to(DEV)
    bad.y = bad.y % 4
    assert int(bad.edge_index[1, 0]) < 33                    # edge 0 ends in graph 0
    bad.edge_index[0, 0] = 33
    m, eng = _engine(name, sd, _args(hidden=128, layers=2), 10, 4)
    eng.forward(bad, torch.arange(2, device=DEV), training=True)
    assert stage in _stage_names(), _stage_names()
    assert int(eng.buffer("status", 1, dtype=torch.int32).item()) & 16
