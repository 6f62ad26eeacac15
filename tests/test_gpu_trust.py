"""``FLTrustFedAVGAlgorithm`` on the GPU: the round equals the independent numpy restatement
(tests/trust_reference.py) and the class's own CPU path bit for bit, for
device-resident and host-resident updates and both output dtypes; a mixed-sign round in which some
clients score 0; the dropped-client round; and the server's loop, in which every round's result is
the next round's previous model."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    FLTrustFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from tests import trust_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
CPU = torch.device("cpu")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
ROOT = 3
AGAINST = (1, 7)      # the workers that step the other way


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
    """10 workers: the previous model plus a common step plus noise; workers 1 and 7 step the other
    way, worker 6 ten times as far, worker 4 is skipped, worker 3 is the root; a tensor of more than
    one chunk and more than one tile, small ones, a scalar and an empty one. Computed once and left
    unchanged."""
    dtype = DTYPES[code]
    size = max(_native.kernel_constant("trust_chunk"), _native.kernel_constant("clip_tile")) + 3
    shapes = {"w": (size,), "b": (5,), "m": (3, 7), "scalar": (), "e": (0, 2)}
    gen = torch.Generator().manual_seed(1234)
    previous = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    step = {k: 0.5 * torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(10):
        if c == 4:
            clients.append(None)
            continue
        scale = -1.0 if c in AGAINST else 10.0 if c == 6 else 1.0
        clients.append({k: (previous[k] + scale * step[k] + 0.1 * torch.randn(s, generator=gen, dtype=torch.float64))
                        .to(dtype) for k, s in shapes.items()})
    return clients, previous


def restate(clients, previous, dtype, out32: bool, root=ROOT):
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    rows = [list(c.values()) for c in clients if c is not None]
    return ref.fltrust(rows, ids.index(root), list(previous.values()), constants(), dtype,
                       out_dtype=np.float32 if out32 else np.float64)


def run_round(device, clients, previous, on_device=True, root=ROOT, **kw):
    algo = FLTrustFedAVGAlgorithm(root, device=device, **kw)
    for wid, c in enumerate(clients):
        if c is None:
            algo.process_worker_data(wid, None)
            continue
        params = {k: (v.to(device) if on_device else v.clone()) for k, v in c.items()}
        algo.process_worker_data(wid, ParameterMessage(parameter=params, aggregation_weight=wid + 1))
    if previous is not None:
        algo.set_old_parameter({k: v.clone() for k, v in previous.items()})   # the server's cache: on the host
    return algo, algo.aggregate_worker_data()


def assert_round(algo, msg, cpu, cpu_msg, want, ids, clients, out_dtype):
    rec, crec = algo.last_trust, cpu.last_trust
    assert rec.worker_ids == ids == crec.worker_ids
    assert rec.dropped == [ids[r] for r in want["dropped"]] == crec.dropped
    assert rec.kept == [ids[r] for r in want["kept"]] == crec.kept
    for field in ("dots", "sqnorms", "scores", "coefficients"):
        assert fbits(getattr(rec, field)) == fbits(want[field]) == fbits(getattr(crec, field)), field
    assert fbits([rec.total_score]) == fbits([want["total_score"]]) == fbits([crec.total_score])
    first = next(c for c in clients if c is not None)
    assert list(msg.parameter) == list(first)
    for (name, got), w in zip(msg.parameter.items(), want["result"]):
        assert got.device.type == "cuda" and got.dtype == out_dtype and got.shape == first[name].shape
        assert np.array_equal(as_bits(got), as_bits(torch.from_numpy(w))), (name, out_dtype)
        assert np.array_equal(as_bits(got), as_bits(cpu_msg.parameter[name])), (name, out_dtype)


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_round_equals_restatement_and_cpu_class(hip_device, code, on_device):
    clients, previous = planted_round(code)
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    for out_dtype in (torch.float64, torch.float32):
        want = restate(clients, previous, DTYPES[code], out_dtype == torch.float32)
        algo, msg = run_round(hip_device, clients, previous, on_device, out_dtype=out_dtype)
        cpu, cpu_msg = run_round(CPU, clients, previous, False, out_dtype=out_dtype)
        assert algo.skipped_workers == {4}
        assert_round(algo, msg, cpu, cpu_msg, want, ids, clients, out_dtype)


def test_mixed_signs_some_clients_score_zero(hip_device):
    clients, previous = planted_round("f32")
    algo, msg = run_round(hip_device, clients, previous)
    rec = algo.last_trust
    assert [w for w, s in zip(rec.kept, rec.scores) if s == 0.0] == list(AGAINST)
    assert [w for w, c in zip(rec.kept, rec.coefficients) if c == 0.0] == list(AGAINST)
    at = {w: k for k, w in enumerate(rec.kept)}
    assert rec.scores[at[ROOT]] == pytest.approx(1.0, abs=1e-12)                 # the root against itself
    assert all(0.9 < rec.scores[at[w]] < 1.0 for w in rec.kept if w not in AGAINST and w != ROOT)
    assert rec.coefficients[at[6]] == pytest.approx(rec.scores[at[6]] / 10.0, rel=0.05)   # rescaled to the root's norm
    assert rec.total_score == pytest.approx(sum(s for w, s in zip(rec.kept, rec.scores) if w != ROOT), rel=1e-12)
    # the step has the root update's direction and about its length: the result moved with the honest workers
    root = {k: v.to(torch.float64) - previous[k] for k, v in clients[ROOT].items()}
    moved = {k: v.cpu() - previous[k] for k, v in msg.parameter.items()}
    dot = sum(float((moved[k] * root[k]).sum()) for k in root)
    n_root, n_moved = (sum(float((d[k] ** 2).sum()) for k in d) ** 0.5 for d in (root, moved))
    assert dot / (n_root * n_moved) > 0.9 and 0.8 < n_moved / n_root < 1.1


def test_dropped_clients_round(hip_device):
    clients, previous = planted_round("f32")
    clients = [None if c is None else dict(c) for c in clients]
    for r, (name, pos, v) in {0: ("w", 0, INF), 8: ("m", 20, -INF)}.items():
        clients[r] = {k: t.clone() for k, t in clients[r].items()}
        clients[r][name].view(-1)[pos] = v
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    want = restate(clients, previous, torch.float32, False)
    assert [ids[r] for r in want["dropped"]] == [0, 8]
    algo, msg = run_round(hip_device, clients, previous)
    cpu, cpu_msg = run_round(CPU, clients, previous, False)
    assert_round(algo, msg, cpu, cpu_msg, want, ids, clients, torch.float64)
    assert algo.last_trust.dropped == [0, 8] and len(algo.last_trust.dots) == 7
    assert all(bool(torch.isfinite(t).all()) for t in msg.parameter.values())
    infinite_root = [None if c is None else dict(c) for c in clients]
    infinite_root[ROOT] = dict(infinite_root[ROOT], b=torch.full((5,), INF))
    with pytest.raises(ValueError, match="root worker 3 sent an infinite update"):
        run_round(hip_device, infinite_root, previous)


def test_nan_and_errors_leave_the_context_usable(hip_device):
    clients, previous = planted_round("f32")
    bad = [None if c is None else dict(c) for c in clients]
    bad[5] = {k: t.clone() for k, t in bad[5].items()}
    bad[5]["w"][-1] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        run_round(hip_device, bad, previous)
    assert e.value.stage == "input" and e.value.bad_clients == [4]             # row 4 of the 9 counted workers
    nan_prev = {k: v.clone() for k, v in previous.items()}
    nan_prev["b"][2] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        run_round(hip_device, clients, nan_prev)
    assert e.value.stage == "input"
    with pytest.raises(ValueError, match="set_old_parameter"):
        run_round(hip_device, clients, None)
    algo, _ = run_round(hip_device, clients, previous)
    assert algo.last_trust.dropped == []


def test_server_loop_feeds_every_result_back_as_the_previous_model(hip_device):
    """Three rounds on one algorithm object, as AggregationServer drives it: set_old_parameter with
    the last global model, the workers' updates, aggregate, clear."""
    clients, previous = planted_round("f32")
    gen = torch.Generator().manual_seed(77)
    algo = FLTrustFedAVGAlgorithm(ROOT, device=hip_device)
    model = {k: v.clone() for k, v in previous.items()}
    want_model = {k: v.clone() for k, v in previous.items()}
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    for rnd in range(3):
        updates = [None if c is None else
                   {k: (want_model[k] + (c[k].to(torch.float64) - previous[k])
                        + 0.01 * torch.randn(c[k].shape, generator=gen, dtype=torch.float64)).to(torch.float32)
                    for k in c} for c in clients]
        want = restate(updates, want_model, torch.float32, False)
        algo.set_old_parameter(model)
        for wid, c in enumerate(updates):
            algo.process_worker_data(wid, None if c is None else ParameterMessage(
                parameter={k: v.to(hip_device) for k, v in c.items()}, aggregation_weight=1))
        msg = algo.aggregate_worker_data()
        algo.clear_worker_data()
        assert algo.last_trust.worker_ids == ids and fbits(algo.last_trust.dots) == fbits(want["dots"])
        for (name, got), w in zip(msg.parameter.items(), want["result"]):
            assert np.array_equal(as_bits(got), as_bits(torch.from_numpy(w))), (rnd, name)
        model = msg.parameter                                                    # on the device, float64
        want_model = {k: torch.from_numpy(w).reshape(previous[k].shape) for k, w in zip(previous, want["result"])}
