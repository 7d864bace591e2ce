"""A plain torch float64 restatement of the GEMM contract of cal_amd/csrc/engine.hpp (GemmArgs / GemmProb / Xform / BNRef),
for tests/test_gpu_gemm_contract.py.  tests/test_gemm_contract_ref.py ties every function here to torch itself
(batch_norm, BatchNorm1d and autograd), so the GPU tests compare the kernels with torch's meaning of the operations and
not with a second copy of the project's arithmetic.

Everything is in STORAGE coordinates, as the contract is: a transformed operand X is the matrix as it lies in memory,
row = node / sample, column = feature; the BatchNorm acts on the columns and the row scale on the rows.
"""
import torch

EPS = 1e-5
MOMENTUM = 0.1


def _d(t):
    return None if t is None else t.detach().double().cpu()


def bn_constants(s, q, n, gamma, beta, eps=EPS, run_mean=None, run_var=None, use_running=False):
    """mean, rstd, scale, shift of one BatchNorm from its arena sums (sum and sum of squares per column over n rows), or
    from the running statistics in eval mode."""
    if use_running:
        mean, var = _d(run_mean), _d(run_var)
    else:
        mean = _d(s) / n
        var = (_d(q) / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = _d(gamma) * rstd
    shift = _d(beta) - mean * scale
    return mean, rstd, scale, shift


def transform(x, rs, scale, shift):
    """op(X) = (rs[row] * X) * scale[col] + shift[col]; rs may be None."""
    x = _d(x)
    if rs is not None:
        x = _d(rs)[:, None] * x
    return x * scale[None, :] + shift[None, :]


def product(op_a, op_b, bias=None, relu=False):
    """C = op(A) op(B) (+ bias) (ReLU) for the LOGICAL operands [M, K] and [K, N]."""
    c = _d(op_a) @ _d(op_b)
    if bias is not None:
        c = c + _d(bias)[None, :]
    return torch.relu(c) if relu else c


def column_sums(c):
    c = _d(c)
    return c.sum(0), (c * c).sum(0)


def aux_normalised(aux, aux_rs, mean, rstd):
    a = _d(aux)
    if aux_rs is not None:
        a = _d(aux_rs)[:, None] * a
    return (a - mean[None, :]) * rstd[None, :]


def dot_sums(c, aux, aux_rs, mean, rstd):
    """The BatchNorm-backward column sums: sum C and sum C * aux_n."""
    c = _d(c)
    return c.sum(0), (c * aux_normalised(aux, aux_rs, mean, rstd)).sum(0)


def running_update(run_mean, run_var, nbt, s, q, n, momentum=MOMENTUM):
    """One training-mode update of the running statistics: unbiased variance, num_batches_tracked + 1."""
    mean = _d(s) / n
    var = (_d(q) / n - mean * mean).clamp_min(0.0)
    unbias = n / (n - 1.0) if n > 1 else 1.0
    return ((1.0 - momentum) * _d(run_mean) + momentum * mean,
            (1.0 - momentum) * _d(run_var) + momentum * var * unbias,
            int(nbt) + 1)
