"""tests/gemm_contract_ref.py against torch itself, in float64 on the CPU: the reference of the GPU contract tests must mean
what torch means by BatchNorm, its running statistics and its backward sums, not what the project's kernels compute."""
import pytest
import torch

from tests import gemm_contract_ref as ref

ROWS, W = 37, 11


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(ROWS, W, generator=g) * (0.5 + torch.rand(W, generator=g)) + torch.randn(W, generator=g)).double()
    return {
        "x": x, "s": x.sum(0), "q": (x * x).sum(0),
        "gamma": (0.5 + torch.rand(W, generator=g)).double(), "beta": torch.randn(W, generator=g).double(),
        "rm": torch.randn(W, generator=g).double(), "rv": (0.5 + torch.rand(W, generator=g)).double(),
        "rs": (0.05 + 0.95 * torch.rand(ROWS, generator=g)).double(),
        "c": torch.randn(ROWS, W, generator=g).double(),
    }


def test_transform_is_batch_norm_in_training_mode(data):
    d = data
    _, _, sc, sh = ref.bn_constants(d["s"], d["q"], ROWS, d["gamma"], d["beta"])
    want = torch.nn.functional.batch_norm(d["x"], None, None, d["gamma"], d["beta"], training=True, eps=ref.EPS)
    torch.testing.assert_close(ref.transform(d["x"], None, sc, sh), want, rtol=1e-12, atol=1e-12)


def test_transform_is_batch_norm_in_eval_mode(data):
    d = data
    _, _, sc, sh = ref.bn_constants(d["s"], d["q"], ROWS, d["gamma"], d["beta"], run_mean=d["rm"], run_var=d["rv"],
                                    use_running=True)
    want = torch.nn.functional.batch_norm(d["x"], d["rm"].clone(), d["rv"].clone(), d["gamma"], d["beta"], training=False,
                                          eps=ref.EPS)
    torch.testing.assert_close(ref.transform(d["x"], None, sc, sh), want, rtol=1e-12, atol=1e-12)


def test_row_scale_comes_before_the_batch_norm(data):
    d = data
    _, _, sc, sh = ref.bn_constants(d["s"], d["q"], ROWS, d["gamma"], d["beta"], run_mean=d["rm"], run_var=d["rv"],
                                    use_running=True)
    want = torch.nn.functional.batch_norm(d["rs"][:, None] * d["x"], d["rm"].clone(), d["rv"].clone(), d["gamma"], d["beta"],
                                          training=False, eps=ref.EPS)
    torch.testing.assert_close(ref.transform(d["x"], d["rs"], sc, sh), want, rtol=1e-12, atol=1e-12)


def test_running_statistics_are_those_of_batchnorm1d_after_one_forward(data):
    d = data
    bn = torch.nn.BatchNorm1d(W, eps=ref.EPS, momentum=ref.MOMENTUM).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(d["rm"]); bn.running_var.copy_(d["rv"]); bn.num_batches_tracked.fill_(5)
    bn(d["x"])
    rm, rv, nbt = ref.running_update(d["rm"], d["rv"], 5, d["s"], d["q"], ROWS)
    torch.testing.assert_close(rm, bn.running_mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rv, bn.running_var, rtol=1e-12, atol=1e-12)
    assert nbt == int(bn.num_batches_tracked) == 6


@pytest.mark.parametrize("with_rs", [False, True])
def test_dot_sums_are_the_bias_and_weight_gradients_of_batchnorm1d(data, with_rs):
    d = data
    x_in = d["rs"][:, None] * d["x"] if with_rs else d["x"]
    bn = torch.nn.BatchNorm1d(W, eps=ref.EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"])
    bn(x_in).backward(d["c"])
    mean, rstd, _, _ = ref.bn_constants(x_in.sum(0), (x_in * x_in).sum(0), ROWS, d["gamma"], d["beta"])
    ds, dp = ref.dot_sums(d["c"], d["x"], d["rs"] if with_rs else None, mean, rstd)
    torch.testing.assert_close(ds, bn.bias.grad, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(dp, bn.weight.grad, rtol=1e-11, atol=1e-11)


def test_product_epilogue_and_column_sums(data):
    d = data
    b = d["c"].t().contiguous()                   # [W, ROWS]
    bias = d["rs"]
    c = ref.product(d["x"], b, bias, relu=True)
    torch.testing.assert_close(c, torch.relu(torch.nn.functional.linear(d["x"], b.t(), bias)), rtol=1e-12, atol=1e-12)
    s, q = ref.column_sums(c)
    torch.testing.assert_close(s, c.sum(0)); torch.testing.assert_close(q, c.pow(2).sum(0))
