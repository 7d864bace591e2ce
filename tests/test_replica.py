"""The pieces cal_amd/replica.py and explain._eval_mode hand to every replica-based driver, pinned on hand-written CPU tensors:
the representative of an undirected edge, the elements-to-players mask, edge_src back in the caller's numbering, the rho / tau /
jaccard report, the eval scope and the k="gt" refusal."""
import math
from types import SimpleNamespace

import pytest
import torch

from cal_amd.data import Data
from cal_amd.explain import _eval_mode, _Layout
from cal_amd.replica import (AGREE, _agree_report, _agree_sums, _caller_columns, _check_topk, _members, _representatives)

# columns 0 and 3 are a pair, 1 has no reverse, 2 is a self loop (its own twin), 4 and 5 are a pair
TWIN = torch.tensor([3, -1, 2, 0, 5, 4], dtype=torch.int32)


def test_representatives_keep_the_lower_column_the_unpaired_column_and_the_self_loop():
    assert _representatives(TWIN).tolist() == [True, True, True, False, True, False]
    assert _representatives(torch.zeros(0, dtype=torch.int32)).tolist() == []


def _two_graphs(order):
    """Two graphs of three nodes; graph order of the columns: (0,1) (1,0) (2,2) | (3,4) (4,3) (4,5); ``order`` shuffles them."""
    ei = torch.tensor([[0, 1, 2, 3, 4, 4], [1, 0, 2, 4, 3, 5]])
    d = Data(x=torch.zeros(6, 2), edge_index=ei if order is None else ei[:, order])
    d.batch, d.num_graphs = torch.tensor([0, 0, 0, 1, 1, 1]), 2
    return d


@pytest.mark.parametrize("shuffled", [False, True])
def test_members_naming_either_column_of_a_pair_selects_both(shuffled):
    twin = torch.tensor([1, 0, 2, 4, 3, -1], dtype=torch.int32)              # over the columns in graph order
    perm = torch.tensor([3, 0, 4, 1, 2, 5]) if shuffled else None           # caller column c is graph-order column perm[c]
    lay = _Layout(_two_graphs(perm))
    assert (lay.order is not None) == shuffled
    graph_pos = torch.arange(6) if perm is None else perm
    for named, want in ((0, [0, 1]), (1, [0, 1]), (2, [2]), (4, [3, 4]), (5, [5])):
        elements = graph_pos == named                                       # the caller names graph-order column ``named``
        got = _members(elements, 6, lay, "edges", twin)
        assert got.dtype == torch.bool and got.nonzero().view(-1).tolist() == want
        assert _members(elements, 6, lay, "edges", None).nonzero().view(-1).tolist() == [named]
    nodes = torch.tensor([True, False, False, False, True, False])
    assert torch.equal(_members(nodes, 6, lay, "nodes", None), nodes)        # nodes are never reordered
    with pytest.raises(ValueError):
        _members(torch.ones(5, dtype=torch.bool), 6, lay, "edges", twin)


def test_caller_columns_leaves_minus_one_alone_and_is_the_identity_without_an_order():
    esrc = torch.tensor([2, -1, 0, 1, -1])
    assert _caller_columns(SimpleNamespace(order=None), esrc, 5) is esrc
    S = SimpleNamespace(order=torch.tensor([7, 5, 9]))
    assert _caller_columns(S, esrc, 5).tolist() == [9, -1, 7, 5, -1]
    none = torch.zeros(0, dtype=torch.long)
    assert _caller_columns(S, none, 0) is none


def test_agree_report_means_over_the_defined_rows_and_counts_the_rest():
    nan = float("nan")
    met = torch.tensor([[0.5, nan, 1.0], [nan, 0.25, 0.5], [-0.25, 0.75, nan], [0.75, -0.5, 0.0]], dtype=torch.float64)
    sums = _agree_sums(met)
    assert sums.dtype == torch.float64 and sums.tolist() == [1.0, 0.5, 1.5, 3.0, 3.0, 3.0]
    res = _agree_report(sums.tolist(), 4)
    assert list(res) == ["rho", "rho_undefined", "tau", "tau_undefined", "jaccard", "jaccard_undefined"]
    assert res == {"rho": 1.0 / 3.0, "rho_undefined": 1, "tau": 0.5 / 3.0, "tau_undefined": 1, "jaccard": 0.5, "jaccard_undefined": 1}
    assert AGREE == ("rho", "tau", "jaccard")
    empty = _agree_report(_agree_sums(torch.full((2, 3), nan, dtype=torch.float64)).tolist(), 2)
    assert all(math.isnan(empty[key]) and empty[key + "_undefined"] == 2 for key in AGREE)


def test_eval_mode_turns_grad_off_and_restores_training_after_an_exception():
    model = torch.nn.Linear(2, 2).train()
    with pytest.raises(RuntimeError, match="inside"):
        with _eval_mode(model):
            assert not model.training and not torch.is_grad_enabled()
            raise RuntimeError("inside")
    assert model.training and torch.is_grad_enabled()
    model.eval()
    with _eval_mode(model):
        assert not model.training
    assert not model.training


@pytest.mark.parametrize("who", ["structure_intervention", "faithfulness", "shapley_agreement", "gradient_agreement", "mask_agreement"])
def test_check_topk_refuses_the_ground_truth_count_in_the_callers_name(who):
    with pytest.raises(ValueError) as e:
        _check_topk(None, "gt", who)
    assert str(e.value) == "%s has no ground truth: k must be an int >= 0" % who
    assert _check_topk(0.25, None, who) == (-1, 0.25) and _check_topk(None, 3, who) == (3, 0.0)
    with pytest.raises(ValueError, match="exactly one of ratio / k"):
        _check_topk(None, None, who)
