"""Rotated 1-bit updates on the host: the numpy path of rotated.py against a written-out answer and the
plain restatement, the binding, and the error the format exists for."""

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import AlgorithmRepository, _native, rotated
from distributed_learning_simulation_lib_amd.sign import _sign_compress_torch

from tests import rsign_reference as ref

SEED = 0x1234_5678_9ABC_DEF0


@pytest.mark.parametrize("mode", ["unbiased", "mse"])
def test_known_answer_one_block(mode):
    """x = (3, 1, 0, ...) in one block of 64: y_j = 3 D_0 +- D_1, so |y| is 4 and 2 half of the time each,
    l1 = 192, l2 = 640, every sign is D_0's, and H of a constant vector is 64 times it at index 0."""
    x = torch.zeros(64)
    x[0], x[1] = 3.0, 1.0
    d, res = rotated._rotated_sign_compress_numpy(x, seed=SEED, draw=3, tensor_id=5, mode=mode)
    D0 = ref.diagonal(SEED, 3, 5, 64)[0]
    assert d.bits.tolist() == [0xFF if D0 else 0] * 8
    sigma = np.float64(640) / 192 if mode == "unbiased" else np.float64(3)
    scale = np.float32(sigma / 64)
    assert d.scales.dtype == torch.float32 and d.scales.tolist() == [float(scale)]
    want = np.zeros(64, dtype=np.float32)
    want[0], want[1] = np.float32(3) - scale * np.float32(64), 1.0
    assert res.numpy().tobytes() == want.tobytes()
    if mode == "mse":
        assert float(scale) == 0.046875 and want[0] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("n", [100, 4096 + 37])
def test_numpy_path_is_the_restatement(dtype, n):
    g = torch.Generator().manual_seed(n)
    delta, error = (torch.randn(n, generator=g, dtype=torch.float64).to(dtype) for _ in range(2))
    d, res = rotated._rotated_sign_compress_numpy(delta, error, seed=SEED, draw=1, tensor_id=2, mode="mse")
    total = (delta + error).to(torch.float64).numpy()
    bits, scales, residual = ref.encode(total, dtype, SEED, 1, 2, "mse")
    assert d.bits.numpy().tobytes() == bits.tobytes()
    assert d.scales.to(torch.float64).numpy().tobytes() == scales.tobytes()
    assert res.to(torch.float64).numpy().tobytes() == residual.tobytes()
    # to_dense() is D H (-+scale), rounded once: total - residual up to that rounding
    B, _, n_pad = ref.geometry(n)
    neg = np.unpackbits(bits, bitorder="little").astype(bool)
    z = ref.fwht(np.where(neg, -np.repeat(scales, B), np.repeat(scales, B)), B)
    sent = ref.narrow(np.where(ref.diagonal(SEED, 1, 2, n_pad), -z, z)[:n], dtype)
    assert d.to_dense().to(torch.float64).numpy().tobytes() == sent.tobytes()


def test_binding_constants_and_registry():
    lib = _native.load()
    assert hasattr(lib, "fedavg_rsign_compress") and hasattr(lib, "fedavg_rsign_aggregate_delta")
    assert _native.kernel_constant("rsign_tile") == rotated.MAX_BLOCK == 4096
    assert _native.kernel_constant("rsign_min_block") == rotated.MIN_BLOCK == 64
    assert _native.kernel_constant("rsign_threads") * 16 == 4096
    assert 1 <= _native.kernel_constant("rsign_batch") <= _native.kernel_constant("rsign_max_clients") == 1024
    assert AlgorithmRepository.has_algorithm("fed_avg_rsign") and AlgorithmRepository.has_algorithm("fed_avg_rsign_ef")


def _nmse(x, sent):
    return float(((x - sent) ** 2).sum() / (x ** 2).sum())


def test_error_does_not_depend_on_the_shape_of_the_data():
    """3 * 4096 + 100 elements, fixed seeds. Gaussian input: the mse rule's normalised squared error is
    1 - 2 / pi = 0.3634 within 0.02 and the unbiased rule's pi / 2 - 1 = 0.5708 within 0.03 (the margins are
    over the sampling deviations of these sizes, 0.0015 and 0.008). Student-t(2) input: the mse rule's
    error is below half of the plain scaled sign's on the same data. Obtained with these seeds: 0.3653
    (mse), 0.5758 (unbiased), and 0.249 against 0.893 (Student-t)."""
    n = 3 * 4096 + 100
    rng = np.random.default_rng(7)
    gauss = torch.from_numpy(rng.standard_normal(n))
    heavy = torch.from_numpy(rng.standard_t(2, n))
    err = {}
    for mode in ("mse", "unbiased"):
        d, _ = rotated._rotated_sign_compress_numpy(gauss, seed=SEED, draw=0, mode=mode)
        err[mode] = _nmse(gauss, d.to_dense())
    assert abs(err["mse"] - (1 - 2 / np.pi)) < 0.02, err
    assert abs(err["unbiased"] - (np.pi / 2 - 1)) < 0.03, err
    d, _ = rotated._rotated_sign_compress_numpy(heavy, seed=SEED, draw=0, mode="mse")
    plain, _ = _sign_compress_torch(heavy)
    rot, sign = _nmse(heavy, d.to_dense()), _nmse(heavy, plain.to_dense())
    assert rot < 0.5 * sign, (rot, sign)
