"""``ClippedFedAVGAlgorithm`` on the GPU: the round equals the independent numpy restatement
(tests/clip_reference.py) and the class's own CPU path bit for bit, for
device-resident and host-resident updates, both output dtypes, both starts, both weightings and
1 and 3 iterations; the dropped-client round; and the record of who was clipped."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    ClippedFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from tests import clip_reference as ref
from tests import geomed_reference as geo

pytestmark = pytest.mark.gpu

INF = float("inf")
CPU = torch.device("cpu")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
RADIUS = 2.0


def as_bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy().reshape(-1)


def fbits(xs) -> list[int]:
    return np.asarray(xs, dtype=np.float64).reshape(-1).view(np.int64).tolist()


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    return geo.native_constants(_native.kernel_constant)


@functools.lru_cache(maxsize=None)
def planted_round(code: str):
    """10 workers: 7 honest ones (a common model plus small noise), 2 planted far away and one
    skipped; a tensor of more than one tile of either kernel, small ones, a scalar and an empty one;
    and the previous global model. Computed once and left unchanged."""
    dtype = DTYPES[code]
    size = max(_native.kernel_constant("point_chunk"), _native.kernel_constant("clip_tile")) + 3
    shapes = {"w": (size,), "b": (5,), "m": (3, 7), "scalar": (), "e": (0, 2)}
    gen = torch.Generator().manual_seed(4321)
    base = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(10):
        if c == 4:
            clients.append(None)
            continue
        far = 25.0 if c in (1, 7) else 0.0
        clients.append({k: (base[k] + 0.01 * torch.randn(s, generator=gen, dtype=torch.float64) + far).to(dtype)
                        for k, s in shapes.items()})
    previous = {k: base[k] + 0.005 * torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    return clients, previous


@functools.lru_cache(maxsize=None)
def restated(code: str, weighted: bool, out32: bool, start: str, iterations: int):
    clients, previous = planted_round(code)
    rows = [list(c.values()) for c in clients if c is not None]
    alpha = [float(i + 1) if weighted else 1.0 for i, c in enumerate(clients) if c is not None]
    return ref.centred_clipping(rows, alpha, constants(), DTYPES[code], RADIUS, iterations=iterations,
                                start=list(previous.values()) if start == "previous" else None,
                                out_dtype=np.float32 if out32 else np.float64)


def run_round(device, clients, previous, on_device=True, weights=None, **kw):
    algo = ClippedFedAVGAlgorithm(RADIUS, device=device, **kw)
    for wid, c in enumerate(clients):
        if c is None:
            algo.process_worker_data(wid, None)
            continue
        params = {k: (v.to(device) if on_device else v.clone()) for k, v in c.items()}
        w = wid + 1 if weights is None else weights[wid]
        algo.process_worker_data(wid, ParameterMessage(parameter=params, aggregation_weight=w))
    if previous is not None:
        algo.set_old_parameter({k: v.clone() for k, v in previous.items()})   # the server's cache: on the host
    return algo, algo.aggregate_worker_data()


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("start", ["previous", "mean"])
@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_round_equals_restatement_and_cpu_class(hip_device, code, on_device, start, iterations):
    clients, previous = planted_round(code)
    prev = previous if start == "previous" else None
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    for weighted in (False, True):
        for out_dtype in (torch.float64, torch.float32):
            want = restated(code, weighted, out_dtype == torch.float32, start, iterations)
            kw = dict(weighted=weighted, out_dtype=out_dtype, start=start, iterations=iterations)
            algo, msg = run_round(hip_device, clients, prev, on_device, **kw)
            cpu, cpu_msg = run_round(CPU, clients, prev, False, **kw)
            rec = algo.last_clipping
            assert rec.worker_ids == ids and rec.dropped == [] and algo.skipped_workers == {4}
            assert fbits(rec.distances) == fbits(want["distances"]) == fbits(cpu.last_clipping.distances)
            assert fbits(rec.coefficients) == fbits(want["coefficients"]) == fbits(cpu.last_clipping.coefficients)
            assert rec.clipped == want["clipped"] == cpu.last_clipping.clipped
            assert list(msg.parameter) == list(clients[0])
            for (name, got), w in zip(msg.parameter.items(), want["result"]):
                assert got.device.type == "cuda" and got.dtype == out_dtype and got.shape == clients[0][name].shape
                assert np.array_equal(as_bits(got), as_bits(torch.from_numpy(w))), (name, weighted, out_dtype)
                assert np.array_equal(as_bits(got), as_bits(cpu_msg.parameter[name])), (name, weighted, out_dtype)


def test_the_planted_clients_are_the_clipped_ones(hip_device):
    clients, previous = planted_round("f32")
    algo, msg = run_round(hip_device, clients, previous, iterations=2)
    rec = algo.last_clipping
    assert rec.clipped == [2, 2]
    for coef in rec.coefficients:      # rows 1 and 6 of the 9 counted workers are workers 1 and 7
        assert [r for r, c in enumerate(coef) if c < 1.0] == [1, 6]
        assert all(c == 1.0 for r, c in enumerate(coef) if r not in (1, 6))
    # two steps of at most 2 * RADIUS / 9 each: the result stays with the honest clients
    for name, got in msg.parameter.items():
        assert float((got.cpu() - previous[name]).abs().max()) <= 2 * RADIUS if got.numel() else True


def test_dropped_clients_round(hip_device):
    clients, previous = planted_round("f32")
    clients = [dict(c) for c in clients if c is not None]
    for r, (name, pos, v) in {0: ("w", 0, INF), 5: ("m", 20, -INF)}.items():
        clients[r] = {k: t.clone() for k, t in clients[r].items()}
        clients[r][name].view(-1)[pos] = v
    want = ref.centred_clipping([list(c.values()) for c in clients], [1.0] * len(clients), constants(), torch.float32,
                                RADIUS, iterations=2, start=list(previous.values()))
    assert want["dropped"] == [0, 5]
    algo, msg = run_round(hip_device, clients, previous, iterations=2)
    cpu, cpu_msg = run_round(CPU, clients, previous, False, iterations=2)
    rec = algo.last_clipping
    assert rec.dropped == [0, 5] == cpu.last_clipping.dropped
    assert fbits(rec.distances) == fbits(want["distances"]) and fbits(rec.coefficients) == fbits(want["coefficients"])
    for (name, got), w in zip(msg.parameter.items(), want["result"]):
        assert bool(torch.isfinite(got).all())
        assert np.array_equal(as_bits(got), as_bits(torch.from_numpy(w))), name
        assert np.array_equal(as_bits(got), as_bits(cpu_msg.parameter[name])), name
    for c in clients:
        c["b"] = torch.full((5,), INF)
    with pytest.raises(ValueError, match="infinite"):
        run_round(hip_device, clients, previous)


def test_nan_and_infinite_centre(hip_device):
    clients, previous = planted_round("f32")
    clients = [dict(c) for c in clients if c is not None]
    bad = {k: v.clone() for k, v in previous.items()}
    bad["w"][5] = INF
    with pytest.raises(NaNAggregationError) as e:
        run_round(hip_device, clients, bad)
    assert e.value.stage == "accumulator"
    clients[3] = {k: t.clone() for k, t in clients[3].items()}
    clients[3]["w"][-1] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        run_round(hip_device, clients, previous)
    assert e.value.stage == "input" and e.value.bad_clients == [3]
    # the context stays usable
    algo, _ = run_round(hip_device, [c for i, c in enumerate(clients) if i != 3], previous)
    assert algo.last_clipping.clipped == [2]
    with pytest.raises(ValueError, match="set_old_parameter"):
        run_round(hip_device, clients, None)
