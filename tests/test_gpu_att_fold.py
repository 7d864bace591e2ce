"""The per-graph attention backward folded into the last backbone layer's backward launch (k_gconv_bwd_att, gconv_bwd_att.hip:
the ATT mode of engine_gconv_bwd_body.hpp with the phases of engine_attphases.hpp; Route::att_fold, switch CAL_AMD_ATT_FOLD read at engine creation): model.py:97-113 differentiated,
then gcn_conv.py:92-104, in ONE launch -- dZ never goes to memory.  Every step here runs twice in the same process on the
same state, fold on and off (off = k_att_bwd_graph, which keeps its own text of the same phases): on is held to the CPU oracle with the tolerances of test_gpu_store_policy.py, and to the
two-launch step with the project's bound for one step on two routes (test_striped_batchnorm_sums_match_the_finishing_launches).
Unit sizes sit on the tile edges (1, 2, 31, 32, 33, 63, 64 nodes, an edgeless graph and a star among them), hidden 64 is one
column slice and 128 two, layers 1 (the folded layer feeds k_feat_bwd), 2 and 3."""
import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests.test_gpu_engine import LOGIT_TOL, _args, _ragged_batch, _stage_names
from tests.test_gpu_store_policy import EDGE_SIZES, MANY_SMALL

pytestmark = pytest.mark.gpu
DEV = "cuda"
NFEAT, NCLS = 10, 4


def _state(name, hidden, layers):
    sd = O.init_state(name, NFEAT, NCLS, hidden=hidden, layers=layers, heads=4)
    g = torch.Generator().manual_seed(7)
    for k in list(sd):
        if k.endswith(".bias") or ("bn" in k and k.endswith(".weight")):
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
    return sd


def _model(name, sd, hidden, layers, **kw):
    from cal_amd import model as M
    m = getattr(M, name)(NFEAT, NCLS, _args(hidden=hidden, layers=layers, **kw))
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=name != "CausalGIN")      # (GINConv keeps an `eps` buffer)
    m = m.to(DEV).train()
    if name == "CausalGAT":
        for c in m.convs:
            c.dropout = 0.0
    return m


def _step(monkeypatch, fold, name, sd, bd, perm, hidden, layers, **kw):
    """One train step (no Adam) of a fresh engine created with the switch set: stats, logp, gradients, launch sites"""
    from cal_amd.engine import StepEngine
    monkeypatch.setenv("CAL_AMD_ATT_FOLD", fold)
    m = _model(name, sd, hidden, layers, **kw)
    eng = StepEngine(m, lr=1e-3)
    eng.train_step(bd, perm.to(DEV), adam=False)
    eng.check_status()
    B = int(perm.numel())
    return dict(stats=eng.buffer("stats", 5).cpu().clone(), logp=eng.buffer("logp", 3 * B * NCLS).cpu().clone(),
                grads={k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None},
                names=_stage_names())


def _oracle(name, sd, b, perm, layers, **kw):
    tr = O.CpuTrainer(name, {k: v.clone() for k, v in sd.items()}, NCLS, lr=1e-3, layers=layers, heads=4, gat_dropout=0.0, **kw)
    loss, lc, lo, lco, logits = tr.step(b.x, b.edge_index, b.batch, b.y, perm=perm)
    return tr, [loss.item(), lc.item(), lo.item(), lco.item()], logits


def _check_oracle(run, tr, losses, logits, B):
    lp = run["logp"].view(3, B, NCLS)
    for r, t in zip(logits, lp):
        assert (r.detach() - t).abs().max().item() < LOGIT_TOL
    assert np.allclose(run["stats"].numpy()[:4], losses, atol=1e-4)
    for k, g in run["grads"].items():
        gref = tr.sd[k].grad
        if gref is not None:
            assert torch.allclose(g, gref, atol=1e-4, rtol=3e-3), k


def _check_on_against_off(on, off, folded):
    assert torch.equal(on["stats"], off["stats"]) and torch.equal(on["logp"], off["logp"])        # the forward is untouched
    for k, g0 in off["grads"].items():
        scale = max(1.0, g0.abs().max().item())
        assert (on["grads"][k] - g0).abs().max().item() <= 2e-5 * scale, k
    if folded:
        assert len(on["names"]) == len(off["names"]) - 1, (on["names"], off["names"])
        for names in (on["names"], off["names"]):
            assert "k_att_bwd_graph" in names and "k_gconv_bwd" in names, names
    else:
        assert on["names"] == off["names"]


def _batches(seed, sizes):
    b, bd = _ragged_batch(seed, NFEAT, sizes), _ragged_batch(seed, NFEAT, sizes).to(DEV)
    b.y = b.y % NCLS
    bd.y = bd.y % NCLS
    return b, bd


def _both(monkeypatch, name, b, bd, hidden, layers, folded, **kw):
    B = int(b.y.numel())
    torch.manual_seed(hidden + layers)
    perm = torch.randperm(B)
    sd = _state(name, hidden, layers)
    on = _step(monkeypatch, "1", name, sd, bd, perm, hidden, layers, **kw)
    off = _step(monkeypatch, "0", name, sd, bd, perm, hidden, layers, **kw)
    tr, losses, logits = _oracle(name, sd, b, perm, layers, **kw)
    _check_oracle(on, tr, losses, logits, B)
    _check_on_against_off(on, off, folded)
    return on, off


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("hidden", [64, 128])
def test_folded_step_on_the_tile_edges_matches_the_oracle_and_the_two_launches(hidden, layers, monkeypatch):
    b, bd = _batches(hidden, EDGE_SIZES)
    _both(monkeypatch, "CausalGCN", b, bd, hidden, layers, True)


@pytest.mark.parametrize("kw", [dict(without_node_attention=True), dict(without_edge_attention=True)], ids=["no-node-att", "no-edge-att"])
def test_folded_step_with_an_attention_switched_off(kw, monkeypatch):
    b, bd = _batches(128, EDGE_SIZES)
    _both(monkeypatch, "CausalGCN", b, bd, 128, 2, True, **kw)


def test_batch_of_a_single_graph_is_refused_alike(monkeypatch):
    """A training step on ONE graph does not exist on any route: the readout BatchNorms see one row and the engine raises
    torch's own error before anything is launched (model.py:127-131) -- with the fold on as with it off."""
    from cal_amd.engine import StepEngine
    _, bd1 = _batches(5, [33])
    sd = _state("CausalGCN", 128, 2)
    for fold in ("1", "0"):
        monkeypatch.setenv("CAL_AMD_ATT_FOLD", fold)
        eng = StepEngine(_model("CausalGCN", sd, 128, 2), lr=1e-3)
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            eng.train_step(bd1, torch.zeros(1, dtype=torch.long, device=DEV), adam=False)


@pytest.mark.parametrize("seed,case", [(2126, (128, 1, 1, 10, [34, 53])), (2086, (128, 4, 3, 2, [20, 12]))])
def test_folded_batches_of_two_graphs_track_the_fp64_step(seed, case, monkeypatch):
    """The smallest batch that trains, two graphs, on the folded launch (layers 1 and 4): two rows per readout BatchNorm, where the
    fp32 oracle's tolerances hold on no route -- so the reference is the fp64 step, with the cases and the bound of
    test_batches_of_two_or_three_graphs_track_the_fp64_step (tests/tools/fuzz_engine.py), and the launch sites say that the
    step folded."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import fuzz_engine
    monkeypatch.setenv("CAL_AMD_ATT_FOLD", "1")
    assert fuzz_engine.run(case, seed) == []
    # the same shape folds: one launch site fewer than with the switch off, gradients within the bound for two routes
    hidden, layers = case[0], case[1]
    _, bd = _batches(seed, [33, 2])
    sd = _state("CausalGCN", hidden, layers)
    perm = torch.tensor([1, 0])
    on = _step(monkeypatch, "1", "CausalGCN", sd, bd, perm, hidden, layers)
    off = _step(monkeypatch, "0", "CausalGCN", sd, bd, perm, hidden, layers)
    _check_on_against_off(on, off, True)


def test_folded_step_with_a_duplicated_edge(monkeypatch):
    from cal_amd.data import Batch, Data
    def build():
        ds = []
        for n in (9, 40, 17):
            a = torch.rand(n, n, generator=torch.Generator().manual_seed(n)) < 0.25
            a = a | a.t()
            a.fill_diagonal_(False)
            ei = a.nonzero().t().contiguous()
            if n == 40:                                    # the first edge and its reverse, once more each
                e0 = ei[:, :1]
                ei = torch.cat([ei, e0, e0.flip(0)], 1)
            ds.append(Data(x=torch.randn(n, NFEAT, generator=torch.Generator().manual_seed(100 + n)), edge_index=ei,
                           y=torch.randint(0, NCLS, (1,), generator=torch.Generator().manual_seed(200 + n))))
        return Batch.from_data_list(ds)

    b, bd = build(), build().to(DEV)
    assert b.edge_index.shape[1] > torch.unique(b.edge_index, dim=1).shape[1]
    _both(monkeypatch, "CausalGCN", b, bd, 128, 2, True)


def test_lean_batches_keep_the_two_launches(monkeypatch):
    """140 graphs x 2 slices are more workgroups than CUs: the LEAN k_gconv_bwd has no ATT form (Route: !lean_bb)"""
    b, bd = _batches(128, MANY_SMALL)
    assert len(MANY_SMALL) * (128 // 64) > torch.cuda.get_device_properties(0).multi_processor_count
    _both(monkeypatch, "CausalGCN", b, bd, 128, 2, False)


@pytest.mark.parametrize("name", ["CausalGAT", "CausalGIN"])
def test_other_backbones_keep_the_two_launches(name, monkeypatch):
    b, bd = _batches(64, [20, 33, 7, 64, 12])
    _both(monkeypatch, name, b, bd, 64, 2, False)


def test_deterministic_engine_gives_the_same_bits_twice_with_the_fold(monkeypatch):
    from cal_amd.engine import StepEngine
    monkeypatch.setenv("CAL_AMD_ATT_FOLD", "1")
    hidden, layers = 128, 2
    _, bd = _batches(hidden, EDGE_SIZES)
    B = len(EDGE_SIZES)
    sd = _state("CausalGCN", hidden, layers)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for _ in range(2):
        eng = StepEngine(_model("CausalGCN", sd, hidden, layers), lr=1e-3, deterministic=True)
        stats = [eng.train_step(bd, perm, adam=True).clone() for _ in range(2)]
        eng.check_status()
        runs.append((eng.buffer("logp", 3 * B * NCLS).clone(), torch.stack(stats), eng.flat_p.detach().clone()))
    for u, v in zip(runs[0], runs[1]):
        assert torch.equal(u, v)                           # bit for bit
