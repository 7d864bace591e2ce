"""GPU parity of the native step engine with a GATConv backbone (CausalGAT, model.py:315-409) against the CPU
oracle: the committed golden fixture, multi-step training WITH attention dropout (same masks fed to the oracle),
the device step counter that keys the masks inside replayed hipGraphs, and the configs 3 / 4 stand-in shapes
(SURVEY.md 8d).  Logit tolerance 1e-4 (north_star)."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests.helpers import GOLDEN, ref_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4
GOLD = 0x9E3779B97F4A7C15      # cal_amd/csrc/gat.hip step_seed()


def _args(**kw):
    d = dict(layers=3, hidden=128, with_random=True, without_node_attention=False,
             without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _engine(sd, args, nfeat=10, ncls=4, lr=1e-3, dropout=0.2, name="CausalGAT"):
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    m = getattr(M, name)(nfeat, ncls, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")          # (GINConv's eps buffers are not part of the oracle's state)
    m = m.to(DEV).train()
    if name == "CausalGAT":
        for c in m.convs:
            c.dropout = dropout
    return m, StepEngine(m, lr=lr)


def _masks(seeds, bd, b, heads, p):
    """The keep masks the kernels draw for `seeds`, in the oracle's slot order (edges without self loops, then
    one loop per node)."""
    from cal_amd import ops
    from cal_amd.plan import plan_of
    plan = plan_of(bd)
    row, col = b.edge_index
    keep_e = (row != col).nonzero().view(-1)
    out = []
    for s in seeds:
        full = ops.gat_dropout_mask(int(s), plan, heads, p).cpu()
        out.append(torch.cat([full[keep_e], full[plan.E:]], 0))
    return out


def test_gat_golden_fixture_train_step_on_engine():
    fx = np.load(os.path.join(GOLDEN, "causal_gat_batch8.npz"))
    sd = {k[3:]: torch.from_numpy(fx[k]).clone() for k in fx.files if k.startswith("sd.")}
    m, eng = _engine(sd, _args(layers=2, hidden=32), dropout=0.0)
    assert eng.heads == 4
    bd = ref_batch(list(fx["ids"])).to(DEV)
    perm = torch.from_numpy(fx["perm"]).to(DEV)
    ev = eng.forward(bd, perm, training=False)
    for n, t in zip(("c", "o", "co"), ev):
        assert np.abs(t.cpu().numpy() - fx[f"eval_logits_{n}"]).max() < LOGIT_TOL, n
    stats = eng.train_step(bd, perm, adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * 8 * 4).view(3, 8, 4).cpu().numpy()
    for i, n in enumerate(("c", "o", "co")):
        assert np.abs(lp[i] - fx[f"train_logits_{n}"]).max() < LOGIT_TOL, n
    assert np.allclose(stats[:4], fx["loss"], atol=1e-4)
    for k, p in m.named_parameters():
        g = fx[f"grad.{k}"]
        if g.size:
            assert np.allclose(p.grad.cpu().numpy(), g, atol=2e-5, rtol=1e-3), k
    post = m.state_dict()
    for k, p in m.named_parameters():
        g = fx[f"grad.{k}"]
        if g.size:
            mask = np.abs(g) > 1e-6
            assert np.allclose(post[k].cpu().numpy()[mask], fx[f"post.{k}"][mask], atol=2e-5, rtol=1e-4), k


def test_gat_steps_with_dropout_track_the_oracle():
    """Three Adam steps with p = 0.2 attention dropout; every step's masks (fixed per-layer seeds) go to the oracle."""
    ids = list(range(16))
    b, bd = ref_batch(ids), ref_batch(ids).to(DEV)
    torch.manual_seed(4)
    sd = O.init_state("CausalGAT", 10, 4, hidden=32, layers=2, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(layers=2, hidden=32), lr=1e-2)
    tr = O.CpuTrainer("CausalGAT", {k: v.clone() for k, v in sd.items()}, 4, lr=1e-2, layers=2, heads=4, gat_dropout=0.2)
    g = torch.Generator().manual_seed(0)
    for step in range(3):
        perm = torch.randperm(len(ids), generator=g)
        for i, c in enumerate(m.convs):
            c.seed = 1000 + 10 * step + i
        tr.fw["gat_masks"] = _masks([c.seed for c in m.convs], bd, b, 4, 0.2)
        loss, lc, lo, lco, logits = tr.step(b.feat, b.edge_index, b.batch, b.y, perm=perm)
        stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu()
        assert eng.gat_fixed
        if step == 0:
            lp = eng.buffer("logp", 3 * len(ids) * 4).view(3, len(ids), 4).cpu()
            for r, t in zip(logits, lp):
                assert (r.detach() - t).abs().max().item() < LOGIT_TOL
            for k, p in m.named_parameters():
                gref = tr.sd[k].grad
                if gref is not None:
                    assert torch.allclose(p.grad.cpu(), gref, atol=5e-5, rtol=2e-3), k
        assert abs(stats[0].item() - loss.item()) < 2e-3 * (step + 1), step
    assert int(eng.step_count.item()) == 3


def test_gat_step_counter_keys_the_masks_and_replays_draw_fresh_ones():
    """No fixed seeds: layer i draws from seed_i + counter * GOLD, the counter advancing once per training step.
    The same masks must be used by the forward and the backward of a step (gradients match the oracle fed with the
    masks of the effective seeds), and a replayed hipGraph must not repeat them."""
    from cal_amd import model as M
    from cal_amd.trainer import CausalTrainer
    ids = list(range(12))
    b, bd = ref_batch(ids), ref_batch(ids).to(DEV)
    torch.manual_seed(9)
    sd = O.init_state("CausalGAT", 10, 4, hidden=32, layers=2, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(layers=2, hidden=32))
    perm = torch.randperm(len(ids))
    eng.train_step(bd, perm.to(DEV), adam=False)
    assert not eng.gat_fixed
    v = int(eng.gat_ctr.item())
    assert v == 1
    eff = [(s + v * GOLD) % (1 << 64) for s in eng.gat_layer_seeds]
    tr = O.CpuTrainer("CausalGAT", {k: v_.clone() for k, v_ in sd.items()}, 4, lr=1e-3, layers=2, heads=4, gat_dropout=0.2,
                      gat_masks=_masks(eff, bd, b, 4, 0.2))
    loss, *_ = tr.step(b.feat, b.edge_index, b.batch, b.y, perm=perm)
    assert abs(eng.buffer("stats", 5)[0].item() - loss.item()) < 1e-4
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(p.grad.cpu(), gref, atol=5e-5, rtol=2e-3), k
    # eval forwards leave the counter alone
    eng.forward(bd, perm.to(DEV), training=False)
    assert int(eng.gat_ctr.item()) == 1
    # graph replay: lr = 0 keeps the weights, so any change of the loss between replays is the mask
    m2 = M.CausalGAT(10, 4, _args(layers=2, hidden=32))
    m2.load_state_dict(sd)
    m2 = m2.to(DEV)
    trn = CausalTrainer(m2, _args(layers=2, hidden=32), lr=0.0, use_graph=True)
    assert trn.engine is not None and trn.engine.heads == 4
    losses = []
    for _ in range(4):
        losses.append(float(trn.step(bd, perm=perm.to(DEV))[0].item()))
    assert len({round(x, 6) for x in losses}) == 4, losses
    c0 = int(trn.engine.gat_ctr.item())
    trn.step(bd, perm=perm.to(DEV))
    assert int(trn.engine.gat_ctr.item()) == c0 + 1
    for c in m2.convs:      # p = 0: replays are bit-identical
        c.dropout = 0.0
    trn2 = CausalTrainer(m2, _args(layers=2, hidden=32), lr=0.0, use_graph=True)
    l0 = [float(trn2.step(bd, perm=perm.to(DEV))[0].item()) for _ in range(3)]
    assert l0[0] == l0[1] == l0[2]


def test_fused_gat_layers_with_one_head_per_column_slice():
    """hidden 128 / 2 heads: head dim 64 = one head per 64-column slice of k_ggat_fwd / k_ggat_bwd (the other tests run
    two heads of 32 per slice).  One train step with dropout vs the oracle."""
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    ids = list(range(20))
    b, bd = ref_batch(ids), ref_batch(ids).to(DEV)
    torch.manual_seed(13)
    sd = O.init_state("CausalGAT", 10, 4, hidden=128, layers=2, heads=2)
    m = M.CausalGAT(10, 4, _args(layers=2), head=2)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m = m.to(DEV).train()
    for i, c in enumerate(m.convs):
        c.dropout, c.seed = 0.2, 900 + i
    eng = StepEngine(m)
    assert eng.heads == 2
    tr = O.CpuTrainer("CausalGAT", {k: v.clone() for k, v in sd.items()}, 4, lr=1e-3, layers=2, heads=2, gat_dropout=0.2,
                      gat_masks=_masks([c.seed for c in m.convs], bd, b, 2, 0.2))
    perm = torch.randperm(len(ids))
    loss, lc, lo, lco, logits = tr.step(b.feat, b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * len(ids) * 4).view(3, len(ids), 4).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    assert int(eng.buffer("status", 1, torch.int32)[0].item()) == 0
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(p.grad.cpu(), gref, atol=5e-5, rtol=2e-3), k


@pytest.mark.parametrize("self_loops,directed,seed,n_lo,n_hi,p", [(False, False, 1, 1, 24, 0.15), (True, True, 2, 1, 24, 0.15),
                                                                  (False, True, 3, 1, 24, 0.15), (False, False, 4, 64, 64, 0.055)])
def test_fused_gat_layers_on_ragged_graphs(self_loops, directed, seed, n_lo, n_hi, p):
    """Edge cases of the per-graph GAT kernels: one-node graphs, isolated nodes, asymmetric edge lists, explicit self
    loops in the input (dropped by GATConv, and they switch the engine to its generic CSR build).  One train step with
    dropout (fixed seeds, masks fed to the oracle) vs the oracle."""
    from tests.helpers import random_graph_batch
    kw = dict(num_graphs=9, n_lo=n_lo, n_hi=n_hi, p=p, feat=10, seed=seed, self_loops=self_loops, directed=directed)
    b, bd = random_graph_batch(**kw), random_graph_batch(**kw).to(DEV)
    assert bd.max_nodes <= 64 and bd.max_edges <= 512, (bd.max_nodes, bd.max_edges)     # the last case sits at the 64-node bound
    torch.manual_seed(20 + seed)
    sd = O.init_state("CausalGAT", 10, 4, hidden=128, layers=2, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(layers=2))
    for i, c in enumerate(m.convs):
        c.seed = 700 + i
    tr = O.CpuTrainer("CausalGAT", {k: v.clone() for k, v in sd.items()}, 4, lr=1e-3, layers=2, heads=4, gat_dropout=0.2,
                      gat_masks=_masks([c.seed for c in m.convs], bd, b, 4, 0.2))
    perm = torch.randperm(9)
    loss, lc, lo, lco, logits = tr.step(b.x, b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * 9 * 4).view(3, 9, 4).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    assert int(eng.buffer("status", 1, torch.int32)[0].item()) == 0
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            scale = max(1.0, gref.abs().max().item())
            assert (p.grad.cpu() - gref).abs().max().item() <= 2e-4 * scale, k


def test_dense_small_graphs_take_the_unfused_gat_layers_next_to_the_fused_head():
    """Graphs of <= 64 nodes with 512 < edges <= 1024: too many edges for k_ggat_fwd / k_ggat_bwd (512 slots each), so the GAT
    backbone runs on the gather kernels while the causal head still uses the per-graph fused GCN kernels (1024 slots).
    One train step vs the oracle."""
    from tests.helpers import random_graph_batch
    b = random_graph_batch(num_graphs=6, n_lo=36, n_hi=44, p=0.25, feat=10, seed=3)
    bd = random_graph_batch(num_graphs=6, n_lo=36, n_hi=44, p=0.25, feat=10, seed=3).to(DEV)
    assert bd.max_nodes <= 64 and 512 < bd.max_edges <= 1024, (bd.max_nodes, bd.max_edges)
    torch.manual_seed(12)
    sd = O.init_state("CausalGAT", 10, 4, hidden=128, layers=2, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(layers=2), dropout=0.0)
    perm = torch.randperm(6)
    tr = O.CpuTrainer("CausalGAT", {k: v.clone() for k, v in sd.items()}, 4, lr=1e-3, layers=2, heads=4, gat_dropout=0.0)
    loss, lc, lo, lco, logits = tr.step(b.x, b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * 6 * 4).view(3, 6, 4).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    assert int(eng.buffer("status", 1, torch.int32)[0].item()) == 0
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            scale = max(1.0, gref.abs().max().item())
            assert (p.grad.cpu() - gref).abs().max().item() <= 5e-4 * scale, k


@pytest.mark.parametrize("name,kind,nfeat,batch", [("CausalGAT", "mutag", 109, 64), ("CausalGCN", "nci1", 139, 512)])
def test_config3_config4_standin_shapes_match_oracle(name, kind, nfeat, batch):
    """SURVEY.md 8d configs 3 (CausalGAT, MUTAG-like, F = 109, B = 64) and 4 (CausalGCN, NCI1-like, F = 139,
    B = 512 per GPU) on the synthetic stand-ins of cal_amd/synth.py: one full train step against the oracle.

    The one-hot features of the NCI1-like batch put dozens of backbone pre-activations within fp32 rounding of zero (|h| down to
    1e-8 of the layer's scale in the fp64 step): which side of the ReLU such an element lands on is decided by the last bit of
    the BatchNorm sums, and one flipped decision moves conv_feat.weight's gradient by 3e-4.  So the gradients are judged against
    the oracle step taken with the ENGINE'S ReLU decisions at the node-level sites (tests/tools/fuzz_engine.py: engine_masks), after asserting that the
    engine and the unforced oracle disagree only where the oracle's pre-activation is within 1e-5 of its site's scale."""
    import sys
    from cal_amd import synth
    from cal_amd.data import Batch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import fuzz_engine
    gs = synth.tu_like(batch, kind=kind, seed=5)
    b, bd = Batch.from_data_list(gs), Batch.from_data_list(gs).to(DEV)
    torch.manual_seed(6)
    sd = O.init_state(name, nfeat, 2, hidden=128, layers=3, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(), nfeat=nfeat, ncls=2, dropout=0.0, name=name)
    perm = torch.randperm(batch)

    def oracle_step(force=None):
        shim, keep = fuzz_engine._ReluShim(force), O.F
        O.F = shim
        try:
            tr = O.CpuTrainer(name, {k: v.clone() for k, v in sd.items()}, 2, lr=1e-3, layers=3, heads=4, gat_dropout=0.0)
            return shim, tr, tr.step(b.x, b.edge_index, b.batch, b.y, perm=perm)
        finally:
            O.F = keep

    shim, _, (loss, lc, lo, lco, logits) = oracle_step()
    stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * batch * 2).view(3, batch, 2).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    # node-level sites (feature layer, three backbone layers, context / objects convolutions) from the engine's activation
    # buffers; the three readout sites stay unforced: read through engine_masks at these batch sizes they disagree with the
    # oracle everywhere, i.e. the buffer does not hold the readout's post-activations in that order here
    masks = fuzz_engine.engine_masks(eng, name, sd, 3, 128, int(bd.batch.numel()), batch)[:6] + [None] * 3
    assert len(masks) == len(shim.pre)
    for site, (mk, pre) in enumerate(zip(masks, shim.pre)):
        if mk is None:
            continue
        flip = mk != (pre > 0)
        assert (pre[flip].abs() <= 1e-5 * pre.abs().max()).all(), (site, pre[flip].abs().max().item(), pre.abs().max().item())
    _, tr, _ = oracle_step(masks)
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(p.grad.cpu(), gref, atol=1e-4, rtol=3e-3), k


@pytest.mark.parametrize("name,hidden", [("CausalGCN", 64), ("CausalGAT", 64), ("CausalGCN", 128), ("CausalGAT", 128), ("CausalGIN", 128)])
def test_big_batch_takes_the_throughput_gemm_and_matches_oracle(name, hidden):
    """A config-5-like batch (4 BA graphs of 5000 nodes: N = 20000 >= 16k rows) runs its node-level products on the
    throughput kernels: hidden 64 on the 128x128 tiles of gemm_big.hip (128-row statistic tiles, 1024-node split-K slabs),
    hidden 128 on the weight-resident kernel of gemm_wres.hip at its K = 128 instantiation (BN / row-scale prologues, the
    statistics and dot-sum epilogues as one partial row per workgroup; GINConv's two GEMMs per layer included): one train
    step vs the oracle."""
    from cal_amd import synth
    from cal_amd.data import Batch
    # (CausalGAT at hidden 128: eight graphs of 2500 nodes -- with four, the readout BatchNorms over four rows amplify the
    #  summation-order noise of this model's gradients to 10x the fp32 oracle's own distance from fp64, with the 128 x 128 tile
    #  kernels and with the weight-resident ones alike (CAL_AMD_WRES=0 / 1: 2.04e-3 / 2.00e-3 on bn_feat.weight at scale 2.5))
    ng, nn = (8, 2500) if (name, hidden) == ("CausalGAT", 128) else (4, 5000)
    gs = synth.ba_graphs(ng, n=nn, seed=3)
    b, bd = Batch.from_data_list(gs), Batch.from_data_list(gs).to(DEV)
    torch.manual_seed(8)
    sd = O.init_state(name, 10, 4, hidden=hidden, layers=2, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args(hidden=hidden, layers=2), dropout=0.0, name=name)
    perm = torch.randperm(ng)
    tr = O.CpuTrainer(name, {k: v.clone() for k, v in sd.items()}, 4, lr=1e-3, layers=2, heads=4, gat_dropout=0.0)
    loss, lc, lo, lco, logits = tr.step(b.feat, b.edge_index, b.batch, b.y, perm=perm)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    tr64 = O.CpuTrainer(name, sd64, 4, lr=1e-3, layers=2, heads=4, gat_dropout=0.0)
    tr64.step(b.feat.double(), b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * ng * 4).view(3, ng, 4).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    for k, p in m.named_parameters():
        g32, g64 = tr.sd[k].grad, tr64.sd[k].grad
        if g32 is not None:
            # sums over 20000 nodes through a readout BatchNorm over only 4 graphs amplify fp32 summation-order noise, so the
            # bound is stated against the oracle evaluated in fp64 (as tests/test_gpu_configs.py does at config-5 width): the
            # HIP path must be as close to it as the fp32 oracle is (x4), plus 1e-5 of the gradient's largest entry
            e_gpu = (p.grad.cpu().double() - g64).abs().max().item()
            e_cpu = (g32.double() - g64).abs().max().item()
            # (CausalGAT at hidden 128, eight graphs: the fp32 oracle lands within 1e-6 of fp64 there, the HIP path within
            #  4.2e-5 -- context_convs.weight, 128 x 128 tile kernels and weight-resident ones alike -- an absolute floor of 5e-5)
            floor = 5e-5 if (name, hidden) == ("CausalGAT", 128) else 1e-5
            assert e_gpu <= 4 * e_cpu + floor * max(1.0, g64.abs().max().item()), (k, e_gpu, e_cpu)


def test_fused_per_graph_gat_forward_with_dropout_matches_oracle():
    """hidden 128 / 4 heads (D = 32) on SPMotif graphs (<= 64 nodes): the backbone layers run on k_ggat_fwd (engine_ggat.hpp);
    one train step with p = 0.2 attention dropout and fixed per-layer seeds, masks fed to the oracle."""
    ids = list(range(24))
    b, bd = ref_batch(ids), ref_batch(ids).to(DEV)
    assert 0 < bd.max_nodes <= 64
    torch.manual_seed(11)
    sd = O.init_state("CausalGAT", 10, 4, hidden=128, layers=3, heads=4)
    m, eng = _engine({k: v.clone() for k, v in sd.items()}, _args())
    for i, c in enumerate(m.convs):
        c.seed = 500 + i
    tr = O.CpuTrainer("CausalGAT", {k: v.clone() for k, v in sd.items()}, 4, lr=1e-3, layers=3, heads=4, gat_dropout=0.2,
                      gat_masks=_masks([c.seed for c in m.convs], bd, b, 4, 0.2))
    perm = torch.randperm(len(ids))
    loss, lc, lo, lco, logits = tr.step(b.feat, b.edge_index, b.batch, b.y, perm=perm)
    stats = eng.train_step(bd, perm.to(DEV), adam=True).cpu().numpy()
    lp = eng.buffer("logp", 3 * len(ids) * 4).view(3, len(ids), 4).cpu()
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(stats[:4], [loss.item(), lc.item(), lo.item(), lco.item()], atol=1e-4)
    for k, p in m.named_parameters():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(p.grad.cpu(), gref, atol=5e-5, rtol=2e-3), k
    # the status word stays clean and the unfused path (no per-graph bounds) gives the same logits
    assert int(eng.buffer("status", 1, torch.int32)[0].item()) == 0
    bd2 = ref_batch(ids).to(DEV)
    m2, eng2 = _engine({k: v.clone() for k, v in sd.items()}, _args())
    eng2.fused = False
    for i, c in enumerate(m2.convs):
        c.seed = 500 + i
    eng2.train_step(bd2, perm.to(DEV), adam=False)
    lp2 = eng2.buffer("logp", 3 * len(ids) * 4).view(3, len(ids), 4).cpu()
    assert (lp - lp2).abs().max().item() < 2e-5
