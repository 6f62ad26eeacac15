"""Centred clipping without a GPU: ``fedavg.clipping_coefficients`` and ``ClippedFedAVGAlgorithm``
on the CPU device against the independent numpy restatement (tests/clip_reference.py, DESIGN.md
§5j), bit for bit; the refusals; the finite screen; and the rule's bound on the step. Not a
reference algorithm: the restatement is what parity means."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    ClippedFedAVGAlgorithm,
    DeltaParameterMessage,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from distributed_learning_simulation_lib_amd.fedavg import clipping_coefficients
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor
from tests import clip_reference as ref
from tests import foreign_messages as fm
from tests import geomed_reference as geo

INF = float("inf")
CPU = torch.device("cpu")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def constants() -> dict:
    return geo.native_constants(_native.kernel_constant)


def f64(*xs):
    return torch.tensor(xs, dtype=torch.float64)


def bits(t) -> list[int]:
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).reshape(-1).tolist()


def fbits(xs) -> list[int]:
    return np.asarray(xs, dtype=np.float64).reshape(-1).view(np.int64).tolist()


def run_algo(clients, previous=None, device=CPU, weights=None, msg_cls=ParameterMessage, radius=1.0, **kw):
    algo = ClippedFedAVGAlgorithm(radius, device=device, **kw)
    for wid, c in enumerate(clients):
        w = wid + 1 if weights is None else weights[wid]
        algo.process_worker_data(10 + wid, None if c is None else msg_cls(parameter=dict(c), aggregation_weight=w))
    if previous is not None:
        algo.set_old_parameter(previous)
    return algo, algo.aggregate_worker_data()


def check_against_restatement(algo, msg, clients, weights, dtype, out_dtype, previous, radius, iterations):
    """The class's record and result equal the restatement's, bit for bit."""
    counted = [c for c in clients if c is not None]
    ids = [10 + i for i, c in enumerate(clients) if c is not None]
    alpha = [weights[i] for i, c in enumerate(clients) if c is not None]
    start = None if previous is None else [previous[k] for k in counted[0]]
    want = ref.centred_clipping([list(c.values()) for c in counted], alpha, constants(), dtype, radius,
                                iterations=iterations, start=start,
                                out_dtype=np.float32 if out_dtype == torch.float32 else np.float64)
    rec = algo.last_clipping
    assert rec.worker_ids == ids and rec.dropped == [ids[r] for r in want["dropped"]]
    assert len(rec.distances) == iterations and rec.clipped == want["clipped"]
    assert fbits(rec.distances) == fbits(want["distances"])
    assert fbits(rec.coefficients) == fbits(want["coefficients"])
    assert list(msg.parameter) == list(counted[0])
    for (name, got), w in zip(msg.parameter.items(), want["result"]):
        assert got.dtype == out_dtype and got.shape == counted[0][name].shape, name
        assert bits(got) == bits(torch.from_numpy(w)), name
    return want


# ---- the host step ---------------------------------------------------------------------------
def test_clipping_coefficients_edges():
    D = [4.0, 0.0, INF, 9.0, 16.0, 4.000000000000002]
    alpha = [1.0, 2.0, 1.0, 0.0, 3.0, 1.0]
    coef, clipped = clipping_coefficients(D, alpha, 2.0)
    want, want_clipped = ref.coefficients(D, alpha, 2.0)
    assert fbits(coef) == fbits(want) and clipped == want_clipped == 4
    assert coef[0] == 1.0                      # d == radius is inside
    assert coef[1] == 2.0                      # D = 0: the client sits on the centre
    assert coef[2] == 0.0 and math.copysign(1.0, coef[2]) == 1.0   # D = +inf pulls nothing
    assert coef[3] == 0.0                      # alpha = 0 pulls nothing, clipped or not
    assert coef[4] == 3.0 * (2.0 / 4.0)
    assert coef[5] == 2.0 / math.sqrt(4.000000000000002) < 1.0     # just outside
    assert clipping_coefficients(torch.tensor([16.0], dtype=torch.float64), [3.0], 1.0) == ([0.75], 1)
    with pytest.raises(ValueError):
        clipping_coefficients([1.0], [1.0, 2.0], 1.0)
    for bad in (0.0, -1.0, INF, float("nan")):
        with pytest.raises(ValueError):
            clipping_coefficients([1.0], [1.0], bad)


# ---- constructor, messages, registration ------------------------------------------------------
def test_constructor_validation():
    for kw in ({"radius": 0.0}, {"radius": -1.0}, {"radius": INF}, {"radius": float("nan")},
               {"radius": 1.0, "iterations": 0}, {"radius": 1.0, "iterations": 1.5},
               {"radius": 1.0, "start": "origin"}):
        with pytest.raises(ValueError):
            ClippedFedAVGAlgorithm(device=CPU, **kw)
    with pytest.raises(TypeError):
        ClippedFedAVGAlgorithm(1.0, device=CPU, out_dtype=torch.float16)
    with pytest.raises(TypeError):
        ClippedFedAVGAlgorithm(device=CPU)     # the radius has no default
    algo = ClippedFedAVGAlgorithm(2.5, device=CPU)
    assert (algo.radius, algo.iterations, algo.start, algo.weighted) == (2.5, 1, "previous", False)
    assert algo.out_dtype == torch.float64 and algo.last_clipping is None


def test_delta_and_quantised_payloads_are_refused():
    algo = ClippedFedAVGAlgorithm(1.0, device=CPU)
    assert not algo.accepts_delta_messages and not algo.accepts_quantized_messages
    with pytest.raises(NotImplementedError, match="[Dd]elta"):
        algo.process_worker_data(0, DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1))
    with pytest.raises(NotImplementedError):
        algo.process_worker_data(0, fm.DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1))
    q = QuantizedTensor.__new__(QuantizedTensor)
    with pytest.raises(NotImplementedError, match="dequantise"):
        algo.process_worker_data(0, ParameterMessage(parameter={"a": q}, aggregation_weight=1))


def test_more_than_1024_clients_are_refused():
    x = {"a": f64(1.0)}
    with pytest.raises(NotImplementedError, match="1024"):
        run_algo([x] * (_native.POINT_MAX_CLIENTS + 1), previous={"a": f64(0.0)})


def test_missing_key_and_shape_are_refused():
    clients = [{"a": f64(float(x), 0.5), "b": f64(2.0)} for x in range(4)]
    del clients[3]["b"]
    with pytest.raises(ValueError, match="client 13 lacks tensor b"):
        run_algo(clients, previous={"a": f64(0.0, 0.0), "b": f64(0.0)})


def test_missing_or_mismatched_previous_model():
    clients = [{"a": f64(float(x), 0.5), "b": f64(2.0)} for x in range(4)]
    with pytest.raises(ValueError, match="set_old_parameter"):
        run_algo(clients)
    with pytest.raises(ValueError, match="lacks tensor b"):
        run_algo(clients, previous={"a": f64(0.0, 0.0)})
    with pytest.raises(ValueError, match="tensor a"):
        run_algo(clients, previous={"a": f64(0.0, 0.0, 0.0), "b": f64(0.0)})
    with pytest.raises(ValueError, match="tensor c"):
        run_algo(clients, previous={"a": f64(0.0, 0.0), "b": f64(0.0), "c": f64(1.0)})
    _, msg = run_algo(clients, start="mean")   # the mean needs no previous model
    assert torch.isfinite(msg.parameter["a"]).all()
    with pytest.raises(ValueError, match="add up to 0"):
        run_algo(clients, weights=[0.0] * 4, weighted=True, previous={"a": f64(0.0, 0.0), "b": f64(0.0)})


def test_registered_with_the_robust_rules_classes():
    assert AlgorithmRepository.has_algorithm("fed_centered_clipping")
    entry = AlgorithmRepository.config["fed_centered_clipping"]
    assert entry["server_cls"] is AlgorithmRepository.config["fed_geometric_median"]["server_cls"]
    assert entry.get("client_cls") is AlgorithmRepository.config["fed_geometric_median"].get("client_cls")
    assert isinstance(entry["algorithm_cls"](radius=1.0), ClippedFedAVGAlgorithm)


def test_message_fields_follow_fedavg():
    algo = ClippedFedAVGAlgorithm(1.0, device=CPU)
    algo.aggregate_loss = True
    for wid in range(4):
        algo.process_worker_data(wid, ParameterMessage(
            parameter={"a": f64(float(wid), 1.0)}, aggregation_weight=1 + wid, end_training=True, in_round=True,
            other_data={"training_loss": float(wid), "tag": "x"}))
    algo.set_old_parameter({"a": f64(0.0, 0.0)})
    msg = algo.aggregate_worker_data()
    assert isinstance(msg, ParameterMessage) and msg.end_training and msg.in_round
    assert msg.other_data["tag"] == "x"
    assert math.isclose(msg.other_data["training_loss"], sum((1 + w) * float(w) for w in range(4)) / 10)
    _, msg = run_algo([{"a": f64(1.0)}, {"a": f64(2.0)}], previous={"a": f64(0.0)}, msg_cls=fm.ParameterMessage)
    assert type(msg) is fm.ParameterMessage


# ---- the class on the CPU device ----------------------------------------------------------------
def planted(dtype, gen_seed=11, n=8, with_empty=True):
    """n clients around a common model, clients 2 and 5 planted far away; and the previous model."""
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
    previous = {k: base[k] + 0.02 * torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    return clients, previous


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("start", ["previous", "mean"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_cpu_class_matches_restatement(code, start, iterations):
    dtype = DTYPES[code]
    clients, previous = planted(dtype)
    clients[4] = None    # a skipped worker
    prev = previous if start == "previous" else None
    for weighted in (False, True):
        for out_dtype in (torch.float64, torch.float32):
            algo, msg = run_algo(clients, previous=prev, weighted=weighted, out_dtype=out_dtype, start=start,
                                 iterations=iterations, radius=1.0)
            assert algo.skipped_workers == {14}
            ws = [float(i + 1) if weighted else 1.0 for i in range(len(clients))]
            want = check_against_restatement(algo, msg, clients, ws, dtype, out_dtype, prev, 1.0, iterations)
            assert want["dropped"] == [] and msg.parameter["e"].shape == (0, 4)
            if start == "previous":     # rows 2 and 4 of the 7 counted clients are the planted ones
                assert want["clipped"] == [2] * iterations
                assert all(c[2] < 0.01 * ws[2] and c[4] < 0.01 * ws[5] for c in algo.last_clipping.coefficients)


def test_previous_model_in_another_dtype_is_converted_once():
    clients, previous = planted(torch.float32, with_empty=False)
    prev32 = {k: v.to(torch.float32) for k, v in previous.items()}
    algo, msg = run_algo(clients, previous=prev32, radius=0.5)
    check_against_restatement(algo, msg, clients, [1.0] * 8, torch.float32, torch.float64,
                              {k: v.to(torch.float64) for k, v in prev32.items()}, 0.5, 1)
    assert all(v.dtype == torch.float32 for v in prev32.values())     # the caller's model is untouched


def test_everyone_inside_the_radius_is_centre_plus_mean_difference():
    clients, previous = planted(torch.float64, with_empty=False)
    algo, msg = run_algo(clients, previous=previous, radius=1e6)
    assert algo.last_clipping.clipped == [0] and algo.last_clipping.coefficients == [[1.0] * 8]
    for k, got in msg.parameter.items():
        acc = None
        for c in clients:
            d = c[k] - previous[k]
            acc = d if acc is None else acc + d
        assert bits(got) == bits(previous[k] + acc / 8.0)
        mean = sum(c[k] for c in clients) / 8.0
        assert torch.allclose(got, mean, rtol=0, atol=1e-12)         # close to FedAvg, not bit-equal


def test_infinite_clients_are_dropped_and_stay_in_the_divisor():
    clients = [{"a": f64(float(x), 0.5), "b": f64(2.0)} for x in (0.0, 1.0, 3.0, 6.0, 2.0)]
    clients[1]["a"] = f64(INF, 0.5)
    clients[3]["b"] = f64(-INF)
    previous = {"a": f64(1.0, 0.5), "b": f64(2.0)}
    algo, msg = run_algo(clients, previous=previous, radius=10.0)
    want = check_against_restatement(algo, msg, clients, [1.0] * 5, torch.float64, torch.float64, previous, 10.0, 1)
    assert want["dropped"] == [1, 3] and algo.last_clipping.dropped == [11, 13]
    assert all(len(d) == 3 for d in algo.last_clipping.distances)
    # 1 + ((0 - 1) + (3 - 1) + (2 - 1)) / 5: the two dropped clients pull nothing and still count
    assert msg.parameter["a"][0].item() == 1.0 + 2.0 / 5.0 and msg.parameter["b"].item() == 2.0
    for c in clients:
        c["a"] = f64(INF, 0.0)
    with pytest.raises(ValueError, match="infinite"):
        run_algo(clients, previous=previous)


def test_nan_input_names_the_client_and_an_infinite_centre_is_an_accumulator_nan():
    clients = [{"a": f64(float(x), 0.5)} for x in range(4)]
    clients[2]["a"] = f64(float("nan"), 0.5)
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, previous={"a": f64(0.0, 0.0)})
    assert e.value.stage == "input" and list(e.value.bad_clients) == [2]
    clients[2]["a"] = f64(2.0, 0.5)
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, previous={"a": f64(INF, 0.0)})
    assert e.value.stage == "accumulator"
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, previous={"a": f64(float("nan"), 0.0)})
    assert e.value.stage == "input"


def test_one_step_moves_the_centre_by_at_most_the_radius():
    """|v_1 - v_0| <= radius (1 + 2^-40) + 2^-52 |v_0|: every term c_i (x_i - v_0) has norm at most
    alpha_i radius, so their sum over W has norm at most radius; the margins cover the n rounded
    adds and the rounding of z + r."""
    gen = torch.Generator().manual_seed(3)
    shapes = {"w": (40, 9), "b": (17,)}
    base = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(10):
        far = 1e3 * (c + 1) if c in (1, 4, 7, 8) else 0.0
        clients.append({k: (base[k] + torch.randn(s, generator=gen, dtype=torch.float64) + far).to(torch.float32)
                        for k, s in shapes.items()})
    for weighted in (False, True):
        for radius in (0.25, 3.0):
            algo, msg = run_algo(clients, previous=base, radius=radius, weighted=weighted)
            assert algo.last_clipping.clipped[0] >= 4
            move = math.sqrt(sum(float(((msg.parameter[k] - base[k]) ** 2).sum()) for k in shapes))
            norm0 = math.sqrt(sum(float((base[k] ** 2).sum()) for k in shapes))
            print(f"radius {radius} weighted {weighted}: moved {move!r}")
            assert 0 < move <= radius * (1 + 2.0 ** -40) + 2.0 ** -52 * norm0
