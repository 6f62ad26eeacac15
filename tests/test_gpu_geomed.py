"""``GeometricMedianFedAVGAlgorithm`` on the GPU: the round equals the independent numpy restatement
(tests/geomed_reference.py) and the class's own CPU path bit for bit, for
device-resident and host-resident updates, both output dtypes and both weightings; the dropped-client
round; and the result is what ``FedAVGAlgorithm`` returns for the kept messages with the round's
last Weiszfeld weights."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    FedAVGAlgorithm,
    GeometricMedianFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from tests import geomed_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
CPU = torch.device("cpu")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def as_bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy().reshape(-1)


def fbits(xs) -> list[int]:
    return np.asarray(xs, dtype=np.float64).reshape(-1).view(np.int64).tolist()


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    return ref.native_constants(_native.kernel_constant)


@functools.lru_cache(maxsize=None)
def planted_round(code: str):
    """10 workers: 7 honest ones (a common model plus small noise), 2 planted far away and one
    skipped; a tensor of more than one chunk, small ones, a scalar and an empty one. Computed once and
    left unchanged."""
    dtype = DTYPES[code]
    chunk = _native.kernel_constant("point_chunk")
    shapes = {"w": (chunk + 3,), "b": (5,), "m": (3, 7), "scalar": (), "e": (0, 2)}
    gen = torch.Generator().manual_seed(1234)
    base = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(10):
        if c == 4:
            clients.append(None)
            continue
        far = 25.0 if c in (1, 7) else 0.0
        clients.append({k: (base[k] + 0.05 * torch.randn(s, generator=gen, dtype=torch.float64) + far).to(dtype)
                        for k, s in shapes.items()})
    return clients


@functools.lru_cache(maxsize=None)
def restated(code: str, weighted: bool, out32: bool):
    clients = planted_round(code)
    rows = [list(c.values()) for c in clients if c is not None]
    alpha = [float(i + 1) if weighted else 1.0 for i, c in enumerate(clients) if c is not None]
    return ref.geometric_median(rows, alpha, constants(), DTYPES[code],
                                out_dtype=np.float32 if out32 else np.float64)


def run_round(device, clients, on_device=True, weights=None, **kw):
    algo = GeometricMedianFedAVGAlgorithm(device=device, **kw)
    for wid, c in enumerate(clients):
        if c is None:
            algo.process_worker_data(wid, None)
            continue
        params = {k: (v.to(device) if on_device else v.clone()) for k, v in c.items()}
        w = wid + 1 if weights is None else weights[wid]
        algo.process_worker_data(wid, ParameterMessage(parameter=params, aggregation_weight=w))
    return algo, algo.aggregate_worker_data()


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_round_equals_restatement_and_cpu_class(hip_device, code, on_device):
    clients = planted_round(code)
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    for weighted in (False, True):
        for out_dtype in (torch.float64, torch.float32):
            want = restated(code, weighted, out_dtype == torch.float32)
            algo, msg = run_round(hip_device, clients, on_device, weighted=weighted, out_dtype=out_dtype)
            cpu, cpu_msg = run_round(CPU, clients, False, weighted=weighted, out_dtype=out_dtype)
            it = algo.last_iterations
            assert it.worker_ids == ids and it.dropped == [] and it.iterations == 3 and algo.skipped_workers == {4}
            assert fbits(it.distances) == fbits(want["distances"]) == fbits(cpu.last_iterations.distances)
            assert fbits(it.betas) == fbits(want["betas"]) and fbits(it.objectives) == fbits(want["objectives"])
            # the two planted clients weigh least
            beta = it.betas[-1]
            alpha = [float(w + 1) if weighted else 1.0 for w in ids]
            ratio = [b / a for b, a in zip(beta, alpha)]
            assert sorted(range(len(ids)), key=lambda r: ratio[r])[:2] in ([1, 6], [6, 1])
            assert list(msg.parameter) == list(clients[0])
            for (name, got), w in zip(msg.parameter.items(), want["result"]):
                assert got.device.type == "cuda" and got.dtype == out_dtype and got.shape == clients[0][name].shape
                assert np.array_equal(as_bits(got), as_bits(torch.from_numpy(w))), (name, weighted, out_dtype)
                assert np.array_equal(as_bits(got), as_bits(cpu_msg.parameter[name])), (name, weighted, out_dtype)


def test_result_is_fedavg_of_the_kept_messages_with_the_last_beta(hip_device):
    clients = [c for c in planted_round("f32") if c is not None]
    clients = [dict(c) for c in clients]
    clients[2] = {k: v.clone() for k, v in clients[2].items()}
    clients[2]["w"][17] = INF                                  # dropped by the finite screen
    for out_dtype in (torch.float64, torch.float32):
        algo, msg = run_round(hip_device, clients, max_iterations=2, out_dtype=out_dtype)
        it = algo.last_iterations
        assert it.dropped == [2] and it.iterations == 2 and len(it.betas[-1]) == len(clients) - 1
        kept = [wid for wid in it.worker_ids if wid not in it.dropped]
        fed = FedAVGAlgorithm(device=hip_device, result_dtype=out_dtype)
        for wid, beta in zip(kept, it.betas[-1]):
            params = {k: v.to(hip_device) for k, v in clients[wid].items()}
            fed.process_worker_data(wid, ParameterMessage(parameter=params, aggregation_weight=beta))
        want = fed.aggregate_worker_data().parameter
        assert list(want) == list(msg.parameter)
        for name, got in msg.parameter.items():
            assert got.dtype == want[name].dtype == out_dtype
            assert np.array_equal(as_bits(got), as_bits(want[name])), (name, out_dtype)


def test_dropped_clients_round(hip_device):
    clients = [dict(c) for c in planted_round("f32") if c is not None]
    for r, (name, pos, v) in {0: ("w", 0, INF), 5: ("m", 20, -INF)}.items():
        clients[r] = {k: t.clone() for k, t in clients[r].items()}
        clients[r][name].view(-1)[pos] = v
    want = ref.geometric_median([list(c.values()) for c in clients], [1.0] * len(clients), constants(), torch.float32)
    assert want["dropped"] == [0, 5]
    algo, msg = run_round(hip_device, clients)
    cpu, cpu_msg = run_round(CPU, clients, False)
    it = algo.last_iterations
    assert it.dropped == [0, 5] == cpu.last_iterations.dropped
    assert fbits(it.distances) == fbits(want["distances"]) and fbits(it.betas) == fbits(want["betas"])
    for (name, got), w in zip(msg.parameter.items(), want["result"]):
        assert bool(torch.isfinite(got).all())
        assert np.array_equal(as_bits(got), as_bits(torch.from_numpy(w))), name
        assert np.array_equal(as_bits(got), as_bits(cpu_msg.parameter[name])), name
    # every client infinite: nothing is left
    for c in clients:
        c["b"] = torch.full((5,), INF)
    with pytest.raises(ValueError, match="infinite"):
        run_round(hip_device, clients)


def test_nan_input_names_the_clients(hip_device):
    clients = [dict(c) for c in planted_round("f32") if c is not None]
    clients[3] = {k: t.clone() for k, t in clients[3].items()}
    clients[3]["w"][-1] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        run_round(hip_device, clients)
    assert e.value.stage == "input" and e.value.bad_clients == [3]
    # the context stays usable
    algo, _ = run_round(hip_device, [c for i, c in enumerate(clients) if i != 3])
    assert algo.last_iterations.iterations == 3
