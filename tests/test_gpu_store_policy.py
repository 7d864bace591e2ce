"""The stores of the per-graph fused kernels that carry a store policy (engine_mma.hpp: the dW slabs and dX' partial tiles of
k_gconv_bwd, the z rows and output tiles of k_gconv_fwd), with every one of
them on a tile edge: graphs of 1, 2, 31, 32, 33, 63 and 64 nodes (one and two row tiles, full and one-row tiles), hidden 64
(one column slice) and 128 (two slices: both dX' partial planes), and a batch of more workgroups than CUs (the LEAN
instantiations).  The step is held to the CPU oracle with the tolerances of test_ragged_and_odd_shapes, whatever
policy the build chose; a deterministic engine must give the same bits twice."""
import pytest
import torch
import numpy as np

from oracle import cal_oracle as O
from tests.test_gpu_engine import LOGIT_TOL, _args, _engine, _ragged_batch, _stage_names

pytestmark = pytest.mark.gpu
DEV = "cuda"
EDGE_SIZES = [1, 2, 31, 32, 33, 63, 64, 5]                # (index 1 and 5: edgeless graphs, index 2 and 6: stars)
MANY_SMALL = [3 + i % 4 for i in range(140)]              # 140 graphs x 2 slices > the CUs of the device: LEAN backward
PER_GRAPH = ("k_gconv_fwd", "k_gconv_fwd(co)", "k_gconv_bwd", "k_att_bwd_graph")


def _state(hidden, nfeat, ncls, layers):
    sd = O.init_state("CausalGCN", nfeat, ncls, hidden=hidden, layers=layers)
    g = torch.Generator().manual_seed(7)
    for k in list(sd):
        if k.endswith(".bias") or ("bn" in k and k.endswith(".weight")):
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
    return sd


@pytest.mark.parametrize("hidden,sizes", [(64, EDGE_SIZES), (128, EDGE_SIZES), (128, MANY_SMALL)],
                         ids=["h64-edges", "h128-edges", "h128-lean"])
def test_step_with_every_policy_store_on_a_tile_edge_matches_the_oracle(hidden, sizes):
    layers, nfeat, ncls = 2, 10, 4
    torch.manual_seed(hidden + layers)
    b = _ragged_batch(hidden, nfeat, sizes)
    bd = _ragged_batch(hidden, nfeat, sizes).to(DEV)
    b.y = b.y % ncls
    bd.y = bd.y % ncls
    sd = _state(hidden, nfeat, ncls, layers)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(hidden=hidden, layers=layers), nfeat, ncls)
    B = len(sizes)
    if sizes is MANY_SMALL:      # the premise of the LEAN case (Route: lean_bb = workgroups of a one-branch launch > CUs)
        assert B * (hidden // 64) > torch.cuda.get_device_properties(0).multi_processor_count
    perm = torch.randperm(B)
    tr = O.CpuTrainer("CausalGCN", {k: v.clone() for k, v in sd.items()}, ncls, lr=1e-3, layers=layers)
    loss, lc, lo, lco, logits = tr.step(b.x, b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=False).cpu().numpy()
    eng.check_status()
    names = _stage_names()
    for k in PER_GRAPH:
        assert k in names, (k, names)                      # the per-graph kernels ran, not the node-level path
    lp = eng.buffer("logp", 3 * B * ncls).view(3, B, ncls).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(p.grad.cpu(), gref, atol=1e-4, rtol=3e-3), k


def test_deterministic_engine_gives_the_same_bits_twice_on_the_edge_shapes():
    hidden, layers, nfeat, ncls = 128, 2, 10, 4
    bd = _ragged_batch(hidden, nfeat, EDGE_SIZES).to(DEV)
    bd.y = bd.y % ncls
    B = len(EDGE_SIZES)
    sd = _state(hidden, nfeat, ncls, layers)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for _ in range(2):
        m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(hidden=hidden, layers=layers), nfeat, ncls, deterministic=True)
        stats = [eng.train_step(bd, perm, adam=True).clone() for _ in range(2)]
        eng.check_status()
        for k in PER_GRAPH:
            assert k in _stage_names(), k
        runs.append((eng.buffer("logp", 3 * B * ncls).clone(), torch.stack(stats), eng.flat_p.detach().clone()))
    for u, v in zip(runs[0], runs[1]):
        assert torch.equal(u, v)                           # bit for bit
