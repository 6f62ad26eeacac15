"""The geometric median (RFA) without a GPU: ``GeometricMedianFedAVGAlgorithm`` on the CPU device
and ``fedavg.geometric_median_step`` against the independent numpy restatement
(tests/geomed_reference.py), bit for bit; the finite screen; the stopping rule; that
``sqdist_to_point_cpu`` follows the pinned summation order on data that can tell orders apart; and
the rule's robustness and Weiszfeld's monotone objective. Not a reference algorithm: the
restatement is what parity means."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    ClientTable,
    DeltaParameterMessage,
    GeometricMedianFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from distributed_learning_simulation_lib_amd.algorithm.geometric_median_algorithm import (
    POINT_DEFAULTS,
    point_constants,
    sqdist_to_point_cpu,
)
from distributed_learning_simulation_lib_amd.fedavg import geometric_median_step
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor
from tests import foreign_messages as fm
from tests import geomed_reference as ref

INF = float("inf")
CPU = torch.device("cpu")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def constants() -> dict:
    return ref.native_constants(_native.kernel_constant)


def f64(*xs):
    return torch.tensor(xs, dtype=torch.float64)


def bits(t) -> list[int]:
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).reshape(-1).tolist()


def fbits(xs) -> list[int]:
    return np.asarray(xs, dtype=np.float64).reshape(-1).view(np.int64).tolist()


def run_algo(clients, device=CPU, weights=None, msg_cls=ParameterMessage, **kw):
    algo = GeometricMedianFedAVGAlgorithm(device=device, **kw)
    for wid, c in enumerate(clients):
        w = wid + 1 if weights is None else weights[wid]
        algo.process_worker_data(10 + wid, None if c is None else msg_cls(parameter=dict(c), aggregation_weight=w))
    return algo, algo.aggregate_worker_data()


def check_against_restatement(algo, msg, clients, weights, dtype, out_dtype, **kw):
    """The class's record and result equal the restatement's, bit for bit."""
    counted = [c for c in clients if c is not None]
    ids = [10 + i for i, c in enumerate(clients) if c is not None]
    alpha = [weights[i] for i, c in enumerate(clients) if c is not None]
    want = ref.geometric_median([list(c.values()) for c in counted], alpha, constants(), dtype,
                                out_dtype=np.float32 if out_dtype == torch.float32 else np.float64, **kw)
    it = algo.last_iterations
    assert it.worker_ids == ids and it.dropped == [ids[r] for r in want["dropped"]]
    assert it.iterations == want["iterations"] and len(it.objectives) == len(want["objectives"])
    assert fbits(it.distances) == fbits(want["distances"])
    assert fbits(it.betas) == fbits(want["betas"])
    assert fbits(it.objectives) == fbits(want["objectives"])
    assert list(msg.parameter) == list(counted[0])
    for (name, got), w in zip(msg.parameter.items(), want["result"]):
        assert got.dtype == out_dtype and got.shape == counted[0][name].shape, name
        assert bits(got) == bits(torch.from_numpy(w)), name
    return want


# ---- constructor, messages, registration ------------------------------------------------------
def test_constructor_validation():
    for kw in ({"max_iterations": 0}, {"max_iterations": -1}, {"max_iterations": 1.5}, {"smoothing": 0.0},
               {"smoothing": -1e-6}, {"smoothing": float("nan")}, {"tolerance": -0.1}, {"tolerance": float("nan")}):
        with pytest.raises(ValueError):
            GeometricMedianFedAVGAlgorithm(device=CPU, **kw)
    with pytest.raises(TypeError):
        GeometricMedianFedAVGAlgorithm(device=CPU, out_dtype=torch.float16)
    algo = GeometricMedianFedAVGAlgorithm(device=CPU)
    assert (algo.max_iterations, algo.smoothing, algo.tolerance, algo.weighted) == (3, 1e-6, 0.0, False)
    assert algo.out_dtype == torch.float64 and algo.last_iterations is None


def test_delta_and_quantised_payloads_are_refused():
    algo = GeometricMedianFedAVGAlgorithm(device=CPU)
    assert not algo.accepts_delta_messages and not algo.accepts_quantized_messages
    with pytest.raises(NotImplementedError, match="[Dd]elta"):
        algo.process_worker_data(0, DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1))
    with pytest.raises(NotImplementedError):
        algo.process_worker_data(0, fm.DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1))
    q = QuantizedTensor.__new__(QuantizedTensor)
    with pytest.raises(NotImplementedError, match="dequantise"):
        algo.process_worker_data(0, ParameterMessage(parameter={"a": q}, aggregation_weight=1))


def test_missing_key_and_shape_are_refused():
    clients = [{"a": f64(float(x), 0.5), "b": f64(2.0)} for x in range(4)]
    del clients[3]["b"]
    with pytest.raises(ValueError, match="client 13 lacks tensor b"):
        run_algo(clients)
    clients = [{"a": f64(float(x), 0.5)} for x in range(4)]
    clients[2]["a"] = f64(1.0, 2.0, 3.0)
    with pytest.raises(ValueError, match="shape"):
        run_algo(clients)


def test_registered_with_the_robust_rules_classes():
    assert AlgorithmRepository.has_algorithm("fed_geometric_median")
    entry = AlgorithmRepository.config["fed_geometric_median"]
    assert entry["server_cls"] is AlgorithmRepository.config["fed_trimmed_mean"]["server_cls"]
    assert entry.get("client_cls") is AlgorithmRepository.config["fed_trimmed_mean"].get("client_cls")
    assert isinstance(entry["algorithm_cls"](), GeometricMedianFedAVGAlgorithm)


def test_message_fields_follow_fedavg():
    algo = GeometricMedianFedAVGAlgorithm(device=CPU)
    algo.aggregate_loss = True
    for wid in range(4):
        algo.process_worker_data(wid, ParameterMessage(
            parameter={"a": f64(float(wid), 1.0)}, aggregation_weight=1 + wid, end_training=True, in_round=True,
            other_data={"training_loss": float(wid), "tag": "x"}))
    msg = algo.aggregate_worker_data()
    assert isinstance(msg, ParameterMessage) and msg.end_training and msg.in_round
    assert msg.other_data["tag"] == "x"
    assert math.isclose(msg.other_data["training_loss"], sum((1 + w) * float(w) for w in range(4)) / 10)
    _, msg = run_algo([{"a": f64(1.0)}, {"a": f64(2.0)}], msg_cls=fm.ParameterMessage)
    assert type(msg) is fm.ParameterMessage


# ---- the Weiszfeld step -------------------------------------------------------------------------
def test_step_against_the_restatement():
    D = [4.0, 0.0, 1e-16, 2.0, 9.0, INF]
    alpha = [1.0, 2.0, 3.0, 0.0, 0.5, 1.0]
    beta, G = geometric_median_step(D[:5], alpha[:5], 1e-6)
    want_beta, want_G = ref.step(D[:5], alpha[:5], 1e-6)
    assert fbits(beta) == fbits(want_beta) and fbits([G]) == fbits([want_G])
    # the clamp: distances 0 and 1e-8 < nu both weigh alpha / nu
    assert beta[1] == 2.0 / 1e-6 and beta[2] == 3.0 / 1e-6 and beta[0] == 0.5
    assert beta[3] == 0.0                                     # alpha = 0 pulls nothing
    assert geometric_median_step(D, alpha, 1e-6)[0][5] == 0.0   # an infinite distance weighs nothing
    # the objective is added in arrival order: (1e16 + 1) + 1 is not 1 + 1 + 1e16
    _, G = geometric_median_step([1e32, 1.0, 1.0], [1.0, 1.0, 1.0], 1e-6)
    assert G == (1e16 + 1.0) + 1.0 != (1.0 + 1.0) + 1e16
    assert geometric_median_step(torch.tensor([4.0], dtype=torch.float64), [3.0], 1.0) == ([1.5], 6.0)
    with pytest.raises(ValueError):
        geometric_median_step([1.0], [1.0, 2.0], 1e-6)
    with pytest.raises(ValueError):
        geometric_median_step([1.0], [1.0], 0.0)


def test_set_weights_keeps_the_pointer_array():
    table = ClientTable(2)
    a, b = f64(1.0, 2.0), f64(3.0)
    table.add_client([a, b], [1.0, 1.0])
    table.add_client([a, None], [2.0, 2.0])
    p, w = table.arrays()
    table.set_weights([0.25, 7.0])
    p2, w2 = table.arrays()
    assert p2 is p and w2 is w and w.tolist() == [0.25, 0.25, 7.0, 0.0]   # the absent entry keeps 0.0
    with pytest.raises(ValueError):
        table.set_weights([1.0])


# ---- the class on the CPU device ----------------------------------------------------------------
def planted(dtype, gen_seed=11, n=8, with_empty=True):
    gen = torch.Generator().manual_seed(gen_seed)
    shapes = {"w": (5, 7), "b": (3,), "s": ()}
    if with_empty:
        shapes["e"] = (0, 4)
    base = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(n):
        far = 30.0 if c in (2, 5) else 0.0
        clients.append({k: (base[k] + 0.05 * torch.randn(s, generator=gen, dtype=torch.float64) + far).to(dtype)
                        for k, s in shapes.items()})
    return clients


@pytest.mark.parametrize("code", list(DTYPES))
def test_cpu_class_matches_restatement(code):
    dtype = DTYPES[code]
    clients = planted(dtype)
    clients[4] = None    # a skipped worker
    for weighted in (False, True):
        for out_dtype in (torch.float64, torch.float32):
            algo, msg = run_algo(clients, weighted=weighted, out_dtype=out_dtype)
            assert algo.skipped_workers == {14}
            ws = [float(i + 1) if weighted else 1.0 for i in range(len(clients))]
            want = check_against_restatement(algo, msg, clients, ws, dtype, out_dtype)
            assert want["iterations"] == 3 and want["dropped"] == []
            assert msg.parameter["e"].shape == (0, 4)


def test_result_is_fedavg_with_the_last_beta():
    clients = planted(torch.float32, with_empty=False)
    for out_dtype in (torch.float64, torch.float32):
        algo, msg = run_algo(clients, out_dtype=out_dtype, max_iterations=2)
        it = algo.last_iterations
        assert it.iterations == 2 and len(it.betas) == 2
        want = ref.fold([list(c.values()) for c in clients], it.betas[-1],
                        np.float32 if out_dtype == torch.float32 else np.float64)
        for got, w in zip(msg.parameter.values(), want):
            assert bits(got) == bits(torch.from_numpy(w))


def test_zero_alpha_is_legal_and_all_zero_is_not():
    clients = [{"a": f64(0.0, 1.0)}, {"a": f64(1.0, 1.0)}, {"a": f64(100.0, -50.0)}, {"a": f64(0.5, 1.0)}]
    ws = [1.0, 2.0, 0.0, 1.0]
    algo, msg = run_algo(clients, weights=ws, weighted=True)
    check_against_restatement(algo, msg, clients, ws, torch.float64, torch.float64)
    assert all(b[2] == 0.0 for b in algo.last_iterations.betas)
    assert 0.0 <= msg.parameter["a"][0].item() <= 1.0       # the weightless outlier pulls nothing
    with pytest.raises(ValueError, match="weight 0"):
        run_algo(clients, weights=[0.0] * 4, weighted=True)


def test_one_client_returns_its_update():
    x = {"a": torch.tensor([1.5, -2.25, 3.0], dtype=torch.float32), "s": torch.tensor(7.0, dtype=torch.float32)}
    algo, msg = run_algo([x])
    assert bits(msg.parameter["a"]) == bits(x["a"].to(torch.float64)) and msg.parameter["s"].item() == 7.0
    assert algo.last_iterations.distances == [[0.0]] * 3


def test_infinite_clients_are_dropped():
    clients = [{"a": f64(float(x), 0.5), "b": f64(2.0)} for x in (0.0, 1.0, 3.0, 6.0, 2.0)]
    clients[1]["a"] = f64(INF, 0.5)
    clients[3]["b"] = f64(-INF)
    ws = [1.0] * 5
    algo, msg = run_algo(clients)
    want = check_against_restatement(algo, msg, clients, ws, torch.float64, torch.float64)
    assert want["dropped"] == [1, 3] and algo.last_iterations.dropped == [11, 13]
    assert all(len(d) == 3 for d in algo.last_iterations.distances)
    assert torch.isfinite(msg.parameter["a"]).all() and msg.parameter["b"].item() == 2.0
    # a norm beyond float64 is treated like an infinity
    clients = [{"a": f64(1e200, 0.0)}, {"a": f64(1.0, 2.0)}, {"a": f64(1.5, 2.5)}]
    algo, _ = run_algo(clients)
    assert algo.last_iterations.dropped == [10]
    for c in clients:
        c["a"] = f64(INF, 0.0)
    with pytest.raises(ValueError, match="infinite"):
        run_algo(clients)
    with pytest.raises(ValueError):
        ref.geometric_median([list(c.values()) for c in clients], [1.0] * 3, constants(), torch.float64)


def test_nan_input_names_the_client():
    clients = [{"a": f64(float(x), 0.5)} for x in range(5)]
    clients[3]["a"] = f64(float("nan"), 0.5)
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients)
    assert e.value.stage == "input" and e.value.bad_clients == [3]
    with pytest.raises(ref.GeomedNaN) as r:
        ref.distances_in_order([list(c.values()) for c in clients], None, constants(), torch.float64)
    assert r.value.stage == "input" and r.value.rows == [3]


def test_tolerance_stops_at_the_documented_iteration():
    clients = planted(torch.float64, gen_seed=5, with_empty=False)
    rows = [list(c.values()) for c in clients]
    full = ref.geometric_median(rows, [1.0] * len(rows), constants(), torch.float64, max_iterations=12)
    G = full["objectives"]
    tol = 1e-3
    # the first t >= 2 (1-based) with |G_{t-2} - G_{t-1}| <= tol * G_{t-1}: the rule stops there with z_{t-1}
    stop = next(t for t in range(2, 13) if abs(G[t - 2] - G[t - 1]) <= tol * G[t - 1])
    assert 2 <= stop < 12       # a condition on the inputs: the stop is neither trivial nor absent
    algo, msg = run_algo(clients, max_iterations=12, tolerance=tol)
    it = algo.last_iterations
    assert it.iterations == stop - 1 and len(it.objectives) == stop
    check_against_restatement(algo, msg, clients, [1.0] * len(rows), torch.float64, torch.float64,
                              max_iterations=12, tolerance=tol)
    # the result is z_{stop - 1}: the fold with the beta measured at z_{stop - 2}
    want = ref.fold(rows, it.betas[stop - 2])
    for got, w in zip(msg.parameter.values(), want):
        assert bits(got) == bits(torch.from_numpy(w))
    # float32 out on an early stop: the float64 point rounded to nearest even
    algo32, msg32 = run_algo(clients, max_iterations=12, tolerance=tol, out_dtype=torch.float32)
    for got, w in zip(msg32.parameter.values(), want):
        assert bits(got) == bits(torch.from_numpy(w.astype(np.float32)))


# ---- the pinned order -----------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(DTYPES))
def test_cpu_distance_follows_the_pinned_order(code):
    dtype, c = DTYPES[code], constants()
    chunk, ae = c["chunk"], c["ae"][code]
    assert point_constants(dtype) == (chunk, c["threads"], ae)
    assert (chunk, c["threads"], ae) == (POINT_DEFAULTS["point_chunk"], POINT_DEFAULTS["point_threads"],
                                         POINT_DEFAULTS[f"point_ae_{code}"])   # the documented defaults
    gen = torch.Generator().manual_seed(99)
    sizes = [1, ae - 1, chunk - 1, chunk + 1, 2 * chunk + 3]
    rows = [[ref.order_sensitive_values(gen, s, dtype).to(dtype) for s in sizes] for _ in range(8)]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    for z in (None, point):
        got = sqdist_to_point_cpu(rows, z)
        want = ref.distances_in_order(rows, z, c, dtype)
        assert bits(got) == fbits(want)
        # the data can tell this order from torch's own sum
        plain = torch.stack([sum(((x.to(torch.float64) - (0 if z is None else z[i])) ** 2).sum()
                                 for i, x in enumerate(r)) for r in rows])
        differ = sum(a != b for a, b in zip(bits(got), bits(plain)))
        print(f"{code}, {'origin' if z is None else 'point'}: {differ} of {len(rows)} clients differ from torch's sum")
        assert differ >= 1
        bound = (sum(sizes) + 2) * 2.0 ** -53
        assert bool(((got - plain).abs() <= 2 * bound * plain).all())


def test_cpu_distance_error_bound_against_rationals():
    c = constants()
    gen = torch.Generator().manual_seed(3)
    sizes = [1500, 7, 1493]
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64).to(torch.float32) for s in sizes] for _ in range(2)]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    got = sqdist_to_point_cpu(rows, point).tolist()
    for g, r in zip(got, rows):
        exact = ref.exact_distance(r, point)
        assert abs(ref.Fraction(g) - exact) <= ref.Fraction(sum(sizes) + 2, 2 ** 53) * exact


# ---- robustness and monotonicity --------------------------------------------------------------
def test_robust_to_three_of_ten_and_objective_decreases():
    gen = torch.Generator().manual_seed(2024)
    shapes = {"w": (40, 25), "b": (25,)}
    model = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(10):
        scale = 1e6 if c in (1, 4, 8) else 1.0      # 3 Byzantine clients at 10^6 times the honest scale
        clients.append({k: ((model[k] + 0.01 * torch.randn(s, generator=gen, dtype=torch.float64)) * scale)
                        .to(torch.float32) for k, s in shapes.items()})
    honest = [c for i, c in enumerate(clients) if i not in (1, 4, 8)]
    mean = {k: torch.stack([c[k].to(torch.float64) for c in honest]).mean(0) for k in shapes}

    def gap(result):
        return math.sqrt(sum(((result[k].to(torch.float64) - mean[k]) ** 2).sum().item() for k in shapes))

    algo, msg = run_algo(clients, max_iterations=8)
    folded = ref.fold([list(c.values()) for c in clients], [1.0] * 10)       # the FedAvg of all ten
    plain = {k: torch.from_numpy(v).reshape(shapes[k]) for k, v in zip(shapes, folded)}
    print("distance to the honest mean: geometric median", gap(msg.parameter), "FedAvg of all ten", gap(plain))
    assert gap(msg.parameter) < gap(plain)
    G = algo.last_iterations.objectives
    assert len(G) == 8
    for a, b in zip(G, G[1:]):
        assert b <= a * (1 + 1e-12), G
