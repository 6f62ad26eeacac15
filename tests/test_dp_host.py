"""The differential-privacy layer without a GPU (dp.py): the CPU path against the
reference's own recorded outputs (tests/golden/dp_golden.npz) and against the numpy restatement
(tests/dp_reference.py) bytes for bytes, the accuracy and the moments of the defined normal stream,
the endpoints and the refusals."""

from __future__ import annotations

import logging
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    DeltaParameterMessage,
    DifferentialPrivacyEmbeddingEndpoint,
    DifferentialPrivacyParameterEndpoint,
    FeatureMessage,
    Message,
    ParameterMessage,
    dp,
)
from tests import dp_cases as cases
from tests import dp_reference as ref

GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "dp_golden.npz")

# The largest relative error of z against the 50-digit value over accuracy_inputs(), measured with
# this test (it prints the figure): 4.362e-16 = 2^-51.03. Pinned at twice that; the ceiling the layer needs is 2^-40.
MEASURED_REL_ERROR = 4.362e-16
assert 2 * MEASURED_REL_ERROR < 2.0**-40


# -- golden vectors from the reference's own code ------------------------------------------------
def test_compute_dp_sigma_matches_the_reference():
    for (eps, delta), want in zip(GOLDEN["sigma/in"], GOLDEN["sigma/out"]):
        assert dp.compute_dp_sigma(epsilon=float(eps), delta=float(delta)) == want
    assert dp.compute_dp_sigma() == GOLDEN["sigma/out"][0]
    for bad in (dict(epsilon=0.0), dict(delta=0.0), dict(delta=1.0)):
        with pytest.raises(AssertionError):
            dp.compute_dp_sigma(**bad)


def test_parameter_golden_bit_for_bit():
    n = sum(1 for k in GOLDEN.files if k.endswith("/names"))
    assert n >= 6
    for i in range(n):
        C, sigma, seed, draw = GOLDEN[f"p{i}/meta"]
        names = [str(k) for k in GOLDEN[f"p{i}/names"]]
        parameter = {k: torch.from_numpy(GOLDEN[f"p{i}/in/{k}"]) for k in names}
        got = dp.add_dp_noise_to_parameter(parameter, C=float(C), sigma=float(sigma), seed=int(seed), draw=int(draw))
        assert list(got) == names
        for k in names:
            want = GOLDEN[f"p{i}/out/{k}"]
            assert got[k].dtype == torch.float64 and tuple(got[k].shape) == want.shape
            assert got[k].numpy().tobytes() == want.tobytes(), (i, k)


def test_tensor_golden_bit_for_bit():
    n = sum(1 for k in GOLDEN.files if k.startswith("t") and k.endswith("/in"))
    assert n >= 6
    for i in range(n):
        C, sigma, seed, draw, tid = GOLDEN[f"t{i}/meta"]
        x, want = torch.from_numpy(GOLDEN[f"t{i}/in"]), GOLDEN[f"t{i}/out"]
        got = dp.add_dp_noise(x, C=float(C), sigma=float(sigma), seed=int(seed), draw=int(draw), tensor_id=int(tid))
        assert got.shape == x.shape and got.numpy().tobytes() == want.tobytes(), i


# -- the CPU path against the restatement --------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("name", list(cases.list_cases()))
def test_cpu_list_cases_equal_the_restatement(name, dtype):
    xs, c, want = cases.list_case(name, dtype)
    got = dp.add_dp_noise_to_parameter({str(i): x for i, x in enumerate(xs)}, C=c, sigma=cases.SIGMA,
                                       seed=cases.SEED, draw=cases.DRAW)
    for i, (x, w) in enumerate(zip(xs, want)):
        assert got[str(i)].dtype == x.dtype and got[str(i)].shape == x.shape
        assert cases.raw(got[str(i)]) == w, (name, dtype, i)


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("rows,length", cases.row_cases())
def test_cpu_row_cases_equal_the_restatement(rows, length, dtype):
    x, want = cases.row_case(rows, length, dtype)
    got = dp.add_dp_noise(x.reshape(rows, length), C=cases.C, sigma=cases.SIGMA, seed=cases.SEED, draw=cases.DRAW,
                          tensor_id=5)
    assert got.shape == (rows, length) and got.dtype == x.dtype
    assert cases.raw(got) == want


def test_mixed_dtypes_follow_each_tensors_group():
    tl = ref.tile()
    xs = {"a": cases.values(tl + 9, "f32", 1), "b": cases.values(37, "bf16", 2), "c": cases.values(3, "f64", 3)}
    got = dp.add_dp_noise_to_parameter(xs, C=cases.C, sigma=cases.SIGMA, seed=cases.SEED, draw=1)
    # the one sum: every tensor's pieces in the order of its own dtype's group
    parts = []
    lanes = ref.kernel_constant("dp_threads")
    for x, d in zip(xs.values(), ("f32", "bf16", "f64")):
        q = cases.widen(x) ** 2
        parts += [ref._tree(ref._lane_sums(q[s : s + tl], ref.group(d), lanes)) for s in range(0, q.size, tl)]
    s = ref.scale_of(np.float64(ref._tree(ref._lane_sums(np.array(parts), 1, lanes))), cases.C)
    for t, (k, d) in enumerate(zip(xs, ("f32", "bf16", "f64"))):
        x = cases.widen(xs[k])
        o = x / s + ref.normals(cases.SEED, 1, t, x.size) * np.float64(cases.SIGMA * cases.C)
        assert cases.raw(got[k]) == ref.narrow_bytes(o, d), k


def test_noise_scale_zero_below_the_norm_returns_the_input():
    """s = 1 and n = z * 0: every element comes back as it is; a zero comes back as a zero, -0.0 only
    where the input is -0.0 and z < 0 (-0.0 + -0.0), +0.0 otherwise."""
    x = cases.values(300, "f32", 9) * 2.0**-6
    x[5], x[6], x[7], x[8] = -0.0, -0.0, 0.0, 0.0
    got = dp.add_dp_noise(x, C=100.0, sigma=0.0, seed=cases.SEED, draw=0)
    z = dp.normal_stream(cases.SEED, 0, 0, 300)
    assert torch.equal(got, x)  # by value: -0.0 == +0.0
    nonzero = (x != 0).numpy()
    assert np.array_equal(got.numpy().view(np.uint32)[nonzero], x.numpy().view(np.uint32)[nonzero])
    for i in (5, 6, 7, 8):
        assert math.copysign(1.0, got[i].item()) == (-1.0 if (i in (5, 6) and z[i] < 0) else 1.0)


# -- the normal stream -----------------------------------------------------------------------------
def test_stream_equals_the_restatement_and_is_indexed_by_its_arguments():
    z = dp.normal_stream(cases.SEED, 2, 7, 4097)
    assert z.tobytes() == ref.normals(cases.SEED, 2, 7, 4097).tobytes()
    assert dp.normal_stream(cases.SEED, 2, 7, 11).tobytes() == z[:11].tobytes()  # a prefix, odd lengths too
    for other in ((cases.SEED + 1, 2, 7), (cases.SEED, 3, 7), (cases.SEED, 2, 8), (cases.SEED ^ (1 << 40), 2, 7)):
        assert not np.array_equal(dp.normal_stream(*other, 64), z[:64])
    assert dp.normal_stream(1, 0, 0, 0).size == 0


def accuracy_inputs() -> tuple[np.ndarray, np.ndarray]:
    """(a, b): u1 at 2^-53, 1, 1 - 2^-53 and the powers of two (and their neighbours) against every
    octant boundary of u2 (and its neighbours), then the integers of 10^5 draws of the stream."""
    a_edge = [0, 2**53 - 1, 2**53 - 2] + [2**k - 1 for k in range(1, 53)] + [2**k for k in range(53)]
    b_edge = sorted(v for v in {k * 2**50 + d for k in range(9) for d in (-2, -1, 0, 1, 2)} if 0 <= v < 2**53)
    a = np.array([x for x in a_edge for _ in b_edge], dtype=np.uint64)
    b = np.array([y for _ in a_edge for y in b_edge], dtype=np.uint64)
    sa, sb = ref.stream_integers(cases.SEED, 0, 0, 50_000)
    return np.concatenate([a, sa]), np.concatenate([b, sb])


def test_normal_pair_accuracy_against_50_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    a, b = accuracy_inputs()
    z0, z1 = dp.box_muller(a, b)
    worst = mp.mpf(0)
    for ai, bi, g0, g1 in zip(a.tolist(), b.tolist(), z0.tolist(), z1.tolist()):
        u2 = mp.mpf(bi) / 2**53
        r = mp.sqrt(-2 * mp.log(mp.mpf(ai + 1) / 2**53))
        for got, want in ((g0, r * mp.cospi(2 * u2)), (g1, r * mp.sinpi(2 * u2))):
            if want == 0:
                assert got == 0, (ai, bi)
            else:
                worst = max(worst, abs((mp.mpf(got) - want) / want))
    print(f"largest relative error of z over {2 * a.size} deviates: {float(worst):.3e} = 2^{float(mp.log(worst, 2)):.2f}")
    assert worst <= 2 * MEASURED_REL_ERROR


def test_moments_of_2_to_20_draws():
    """The bounds are derived, not measured: the mean of n standard normal draws has standard
    deviation 1 / sqrt(n) and their variance sqrt(2 / n), and five of those are asserted; the
    correlation of the (even, odd) pairs is held to the same 5 / sqrt(n). The seed is fixed."""
    n = 1 << 20
    z = dp.normal_stream(12345, 0, 0, n)
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) <= 5 / math.sqrt(n)


# -- the endpoints ---------------------------------------------------------------------------------
class Sink:
    def __init__(self):
        self.sent = []
        self.worker_id = 3

    def send(self, data):
        self.sent.append(data)


def test_parameter_endpoint_transforms_parameters_and_deltas(caplog):
    sink = Sink()
    ep = DifferentialPrivacyParameterEndpoint(sink, C=0.25, epsilon=2.0, delta=1e-4, seed=11)
    assert ep.sigma == dp.compute_dp_sigma(2.0, 1e-4) and ep.worker_id == 3 and ep.draw == 0
    p = {"w": cases.values(40, "f32", 1).reshape(5, 8), "b": cases.values(3, "f64", 2)}
    keep = {k: v.clone() for k, v in p.items()}
    small = {k: v * 0.01 for k, v in p.items()}
    with caplog.at_level(logging.INFO, logger="distributed_learning_simulation_lib_amd.dp"):
        ep.send(ParameterMessage(parameter=p, aggregation_weight=2.0))
        ep.send(DeltaParameterMessage(delta_parameter=dict(small)))
        ep.send(Message(end_training=True))
    assert ep.draw == 2 and len(sink.sent) == 3
    first, second, third = sink.sent
    want0 = dp.add_dp_noise_to_parameter(keep, C=0.25, sigma=ep.sigma, seed=11, draw=0)
    want1 = dp.add_dp_noise_to_parameter(small, C=0.25, sigma=ep.sigma, seed=11, draw=1)
    for k in keep:
        assert torch.equal(first.parameter[k], want0[k]) and first.parameter[k].dtype == keep[k].dtype
        assert torch.equal(second.delta_parameter[k], want1[k])
        assert not torch.equal(want0[k], want1[k])
        assert torch.equal(p[k], keep[k])  # the caller's tensors are not written
    assert first.aggregation_weight == 2.0 and third.end_training
    text = caplog.text
    assert "pre_noise_norm" in text and "expected_noise_norm" in text and "(delta)" in text
    assert text.count("noise dominates signal") == 1  # the small delta: its norm is below sigma * C * sqrt(43)


def test_embedding_endpoint_transforms_features_only():
    sink = Sink()
    ep = DifferentialPrivacyEmbeddingEndpoint(sink, C=1.0, seed=5)
    f = cases.values(6 * 16, "f32", 3).reshape(6, 16)
    p = {"w": cases.values(4, "f32", 4)}
    ep.send(FeatureMessage(feature=f.clone()))
    ep.send(FeatureMessage(feature=None))
    ep.send(ParameterMessage(parameter=p))
    ep.send(FeatureMessage(feature=f.clone()))
    assert ep.draw == 2
    assert torch.equal(sink.sent[0].feature, dp.add_dp_noise(f, C=1.0, sigma=ep.sigma, seed=5, draw=0))
    assert sink.sent[1].feature is None and sink.sent[2].parameter is p
    assert torch.equal(sink.sent[3].feature, dp.add_dp_noise(f, C=1.0, sigma=ep.sigma, seed=5, draw=1))
    rows = torch.linalg.vector_norm(dp.add_dp_noise(f, C=1.0, sigma=0.0, seed=5), dim=1)
    assert (rows <= 1.0 + 1e-6).all()  # every row is clipped on its own


def test_endpoints_draw_a_seed_and_check_their_arguments():
    a, b = DifferentialPrivacyParameterEndpoint(Sink()), DifferentialPrivacyParameterEndpoint(Sink())
    assert a.seed != b.seed and a.C == 1.0 and a.sigma == dp.compute_dp_sigma()
    with pytest.raises(TypeError):
        DifferentialPrivacyParameterEndpoint(Sink(), topology=None)
    with pytest.raises(TypeError):
        DifferentialPrivacyParameterEndpoint(object())
    with pytest.raises(ValueError):
        DifferentialPrivacyParameterEndpoint(Sink(), C=0.0)
    entry = AlgorithmRepository.config["fed_avg_dp"]
    assert entry["client_endpoint_cls"] is DifferentialPrivacyParameterEndpoint
    assert entry["server_cls"] is AlgorithmRepository.config["fed_avg"]["server_cls"]
    assert entry["algorithm_cls"] is AlgorithmRepository.config["fed_avg"]["algorithm_cls"]


# -- the refusals ----------------------------------------------------------------------------------
def test_refusals():
    x = cases.values(8, "f32", 1)
    for bad_c in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            dp.add_dp_noise(x, C=bad_c, sigma=1.0, seed=1)
        with pytest.raises(ValueError):
            dp.add_dp_noise_to_parameter({"x": x}, C=bad_c, sigma=1.0, seed=1)
    for bad_sigma in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            dp.add_dp_noise(x, C=1.0, sigma=bad_sigma, seed=1)
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1, draw=-1), dict(seed=1, draw=1 << 32)):
        with pytest.raises(ValueError):
            dp.add_dp_noise(x, C=1.0, sigma=1.0, **kw)
    with pytest.raises(TypeError):
        dp.add_dp_noise(torch.arange(4), C=1.0, sigma=1.0, seed=1)
    with pytest.raises(TypeError):
        dp.add_dp_noise_to_parameter({"x": x, "n": torch.arange(4)}, C=1.0, sigma=1.0, seed=1)
    for bad in (math.inf, -math.inf, math.nan):
        y = x.clone()
        y[3] = bad
        with pytest.raises(ValueError):
            dp.add_dp_noise(y, C=1.0, sigma=1.0, seed=1)
        with pytest.raises(ValueError):
            dp.add_dp_noise_to_parameter({"x": x, "y": y.to(torch.float16)}, C=1.0, sigma=1.0, seed=1)
    with pytest.raises(ValueError):
        dp.normal_stream(1, 0, 1 << 32, 4)
    assert dp.add_dp_noise_to_parameter({}, C=1.0, sigma=1.0, seed=1) == {}
    e = dp.add_dp_noise(torch.zeros(0, 4), C=1.0, sigma=1.0, seed=1)
    assert e.shape == (0, 4)
    fresh = dp.add_dp_noise(x, C=1.0, sigma=1.0, seed=None)
    assert not torch.equal(fresh, dp.add_dp_noise(x, C=1.0, sigma=1.0, seed=None))
