"""Graph centralities on the MI355X: cal_centrality (csrc/centrality.hip) through the case table of tests/centrality_oracle.py.
Integers are bit-equal to the host twin and to the plain-int restatement; bc / ebc / pr are held to the same bounds against the
EXACT values as the host twin is (tests/test_centrality.py); a second run gives the same bits; one launch per call.

Why each shape is in the table -- the smallest at which this kernel can still go wrong:
  n = 0 .. 3 and a graph without columns (the normalisations, the empty graph, PageRank of dangling nodes only); path, star, cycle,
  house, K4 (levels, one and several shortest paths); two components and an isolated node (the unreached marker, Wasserman-Faust,
  dangling PageRank); n = 63, 64, 65, 127, 128, 129 (word and wave boundaries of rows and ballots -- what one lane writes to LDS and
  another reads shows only above 64 nodes --, sources that do not divide by the four waves); a path of 256 (255 levels), a star
  of 256 (the hub's bc = (n - 1)(n - 2) exactly), K64 (full rows, all bc 0, 4032 columns: the workspace path of ebc, beside
  graphs on the LDS path in the same launch), a 16 x 16 grid and Q6 (many shortest paths, sigma up to 1.6e8), a graph of 257
  nodes (skipped, its neighbours unharmed), one-way / duplicated / self-loop / leaving columns, sources empty, everywhere, and in
  another component only; everything in one launch, and a batch of more graphs than the device has CUs."""
import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.centrality import centrality, eval_structural_baseline, hop_distance, structural_baseline
from cal_amd.data import Batch, DataLoader
from tests import centrality_oracle as O
from tests.test_centrality import (ALPHA, BY_NAME, CASES, GENERAL, MAX_ITER, SMALL, TOL, batch_of, run, same_bits)
from tests.test_gpu_wl import _args, _gpu_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTS = ("far", "reach", "ecc", "deg", "hop", "pr_iters", "skipped")


@pytest.mark.parametrize("case", GENERAL, ids=lambda c: c.__name__[5:])
def test_hip_meets_the_contract(case):
    case(DEV)


def test_integers_equal_the_host_twin_and_a_second_run_gives_the_same_bits():
    b, src = batch_of(CASES, DEV)
    n0 = _lib.query("cal_launch_count")
    c1 = centrality(b, sources=src)
    c2 = centrality(b, sources=src)
    assert _lib.query("cal_launch_count") - n0 == 2                          # one launch per call
    same_bits(c1[:11], c2[:11])
    host = run(CASES, "cpu")[1]
    for k in INTS + ("ignored",):
        assert torch.equal(getattr(c1, k).cpu(), getattr(host, k)), k
    for k in ("bc", "ebc", "pr"):                                            # (not promised bit for bit: both meet the bounds)
        a, h = getattr(c1, k).cpu(), getattr(host, k)
        print(k, "device vs host: max abs difference %.3e" % float((a - h).abs().max()))


def test_a_257_node_graph_is_skipped_and_its_neighbours_are_unharmed():
    big = O._case("path257", 257, O.path(257) + [(0, 300)], O._mask(257, {0}))
    cs = [BY_NAME["house"], big, BY_NAME["ba65"]]
    got, c = run(cs, DEV)
    assert got["skipped"].tolist() == [0, 1, 0] and got["ignored"] == 1 and got["pr_iters"][1] == -1
    lo, hi, elo, ehi = 5, 5 + 257, 12, 12 + 513
    for k in ("far", "reach", "ecc", "deg", "hop"):
        assert (got[k][lo:hi] == -1).all(), k
    for k in ("bc", "pr", "closeness"):
        assert np.isnan(got[k][lo:hi]).all(), k
    assert np.isnan(got["ebc"][elo:ehi]).all() and torch.isnan(c.betweenness()[lo:hi]).all() and torch.isnan(c.degree()[lo:hi]).all()
    rest = {k: (np.concatenate([v[:lo], v[hi:]]) if k not in ("ebc", "pr_iters", "skipped", "ignored") else v) for k, v in got.items()}
    rest["ebc"] = np.concatenate([got["ebc"][:elo], got["ebc"][ehi:]])
    rest["pr_iters"], rest["skipped"], rest["ignored"] = got["pr_iters"][[0, 2]], got["skipped"][[0, 2]], 0
    assert O.judge([cs[0], cs[2]], rest, ALPHA, TOL, MAX_ITER) == []


def test_more_graphs_than_the_device_has_cus():
    cs = (SMALL + [BY_NAME["ba63"], BY_NAME["q6"]]) * 24                     # 360 graphs
    assert len(cs) > torch.cuda.get_device_properties(0).multi_processor_count
    got, _ = run(cs, DEV)
    assert O.judge(cs, got, ALPHA, TOL, MAX_ITER) == []


def test_lds_path_and_workspace_path_side_by_side():
    """K64 has 4032 columns (> CAL_CENTRALITY_LDS_COLS): its per-wave partials of ebc go through the workspace, its neighbours'
    through LDS, in one launch; alone in a batch of few columns nothing needs a workspace."""
    assert _lib.query("cal_centrality_ws", O.LDS_COLS) == 0 and _lib.query("cal_centrality_ws", O.LDS_COLS + 1) == 32 * (O.LDS_COLS + 1)
    cs = [BY_NAME["grid16"], BY_NAME["k64"], BY_NAME["ba129"], BY_NAME["k64"]]
    got, _ = run(cs, DEV)
    assert O.judge(cs, got, ALPHA, TOL, MAX_ITER) == []


# ---- the drivers once on the device, against their CPU result ---------------------------------------------------------------------
def _close(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _close(a[k], b[k])
    elif isinstance(a, float):
        assert (a != a and b != b) or abs(a - b) <= 1e-9, (a, b)
    else:
        assert a == b, (a, b)


def test_drivers_on_the_device_equal_their_cpu_result():
    m = _gpu_model("CausalGCN", _args())
    gs = spmotif.train_mix(12, node_num=7, seed=5)
    b, hb = Batch.from_data_list(gs).to(DEV), Batch.from_data_list(gs)      # (``to`` moves a batch in place: two batches)
    # the structural scores never see the model: the device's figures for them equal the host's; the attention's own figures
    # follow the model's forward, which is compared elsewhere
    dev = structural_baseline(m, b)
    cpu = structural_baseline(_gpu_model("CausalGCN", _args()).to("cpu"), hb)
    assert dev["chance"] == pytest.approx(cpu["chance"], abs=1e-12) and dev["graphs"] == cpu["graphs"] == 12
    for kd in dev["kinds"]:
        for key in ("precision", "recall", "auc"):
            _close(dev["kinds"][kd][key], cpu["kinds"][kd][key])
    loader = DataLoader(gs, 5, shuffle=False)
    ev = eval_structural_baseline(m, loader, DEV)
    for kd in dev["kinds"]:
        for key in ("precision", "recall", "auc"):
            _close(ev["kinds"][kd][key], cpu["kinds"][kd][key])
    loc = m.explanation_locality(b, k="gt")
    hop = hop_distance(b, spmotif.ground_truth(b)[0])
    assert hop.is_cuda and torch.equal(hop.cpu(), hop_distance(hb, spmotif.ground_truth(hb)[0]))
    assert loc["edges"] > 0 and abs(loc["hop0"] + loc["hop1"] + loc["hop2"] + loc["hop3plus"] - 1.0) < 1e-12
