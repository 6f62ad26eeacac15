"""``BulyanFedAVGAlgorithm`` on the MI355X against the numpy restatement (tests/bulyan_reference.py;
DESIGN.md §5k), bit for bit.

Values are small dyadic numbers (integers / 8 in [-4, 4], planted clients 1024 away): every
difference, square and partial sum of a distance is an integer multiple of 2^-6 far below 2^53, so
every entry of ``D`` is exact in float64 in any summation order. The selection is then unambiguous,
and the GPU path, the CPU path and the restatement must return the same bits.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    BulyanFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from tests import bulyan_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
CPU = torch.device("cpu")
NP_OUT = {torch.float64: np.float64, torch.float32: np.float32}


def as_bits(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    t = np.ascontiguousarray(t)
    return t.view(np.int64 if t.dtype == np.float64 else np.int32)


def shapes() -> dict[str, tuple[int, ...]]:
    tile = _native.kernel_constant("mam_tile")
    return {"w": (tile + 3,), "b": (5,), "m": (3, 7), "scalar": (), "empty": (0,)}


def dyadic_clients(seed: int, n: int, dtype=torch.float32) -> list:
    gen = torch.Generator().manual_seed(seed)
    return [{k: (torch.randint(-32, 33, s, generator=gen).to(torch.float64) / 8.0).to(dtype)
             for k, s in shapes().items()} for _ in range(n)]


def as_numpy(clients):
    return [None if c is None else {k: v.to(torch.float64).numpy() for k, v in c.items()} for c in clients]


def run_algo(device, clients, f, out_dtype=torch.float64, on_device=True):
    algo = BulyanFedAVGAlgorithm(num_byzantine=f, device=device, out_dtype=out_dtype)
    for k, c in enumerate(clients):
        if c is None:
            algo.process_worker_data(10 + k, None)
        else:
            p = {name: (t.to(device) if on_device else t) for name, t in c.items()}
            algo.process_worker_data(10 + k, ParameterMessage(parameter=p, aggregation_weight=1 + k))
    return algo, algo.aggregate_worker_data()


def check_round(hip_device, clients, f, out_dtype=torch.float64, on_device=True):
    """The GPU round equals the restatement and the CPU path, bit for bit."""
    want, picked, scores, rule = ref.bulyan_round(as_numpy(clients), f, NP_OUT[out_dtype])
    ids = [10 + k for k, c in enumerate(clients) if c is not None]
    algo, msg = run_algo(hip_device, clients, f, out_dtype, on_device)
    cpu_algo, cpu_msg = run_algo(CPU, clients, f, out_dtype, on_device=False)
    for a in (algo, cpu_algo):
        sel = a.last_selection
        assert sel.worker_ids == ids and sel.picked == [ids[r] for r in picked] and sel.scores == scores
        assert (sel.f, sel.theta, sel.beta) == rule
    assert list(msg.parameter) == list(want) == list(cpu_msg.parameter)
    for name, w in want.items():
        got = msg.parameter[name]
        assert got.device.type == "cuda" and tuple(got.shape) == w.shape and got.dtype == out_dtype
        assert np.array_equal(as_bits(got), as_bits(w)), name
        assert np.array_equal(as_bits(cpu_msg.parameter[name]), as_bits(w)), name
    return algo, msg


@pytest.mark.parametrize("n,f", [(7, 1), (11, 2), (12, 0), (66, 1)])
def test_rounds_match_restatement_and_cpu_path(hip_device, n, f):
    clients = dyadic_clients(100 * n + f, n)
    for out_dtype in (torch.float64, torch.float32):
        algo, _ = check_round(hip_device, clients, f, out_dtype)
    assert (algo.last_selection.theta, algo.last_selection.beta) == (n - 2 * f, n - 4 * f)


def test_host_inputs_skipped_client_and_fp16(hip_device):
    clients = dyadic_clients(5, 12)
    clients[3] = None                                   # n = 11
    check_round(hip_device, clients, 2, on_device=False)
    check_round(hip_device, clients, None, on_device=True)   # f = (11 - 3) // 4 = 2
    half = dyadic_clients(6, 7, torch.float16)
    check_round(hip_device, half, 1)
    check_round(hip_device, half, 1, torch.float32, on_device=False)


def test_67_clients_with_f_1_are_refused_before_any_launch(hip_device):
    clients = [{"a": torch.full((4,), float(k))} for k in range(67)]
    with pytest.raises(NotImplementedError, match="64"):
        run_algo(hip_device, clients, 1)
    with pytest.raises(ValueError, match="4f \\+ 3"):
        run_algo(hip_device, clients[:6], 1)


def test_planted_far_clients_are_not_picked(hip_device):
    n, f = 11, 2
    clients = dyadic_clients(7, n)
    far = (1, 8)
    for r, sign in zip(far, (1.0, -1.0)):
        clients[r] = {k: v + sign * 1024.0 for k, v in clients[r].items()}
    algo, msg = check_round(hip_device, clients, f)
    assert not {10 + r for r in far} & set(algo.last_selection.picked)
    honest = [c for r, c in enumerate(clients) if r not in far]
    for name in shapes():
        if name == "empty":
            continue
        stack = torch.stack([c[name] for c in honest]).to(torch.float64)
        got = msg.parameter[name].cpu()
        assert bool((got >= stack.min(dim=0).values).all()) and bool((got <= stack.max(dim=0).values).all())


def test_error_stages(hip_device):
    tile = _native.kernel_constant("mam_tile")
    clients = dyadic_clients(9, 7)
    clients[2]["w"][tile + 1] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        run_algo(hip_device, clients, 1)
    assert e.value.stage == "input" and e.value.bad_clients == [2]
    # the same infinity in the same element of two clients: inf - inf in a distance
    clients = dyadic_clients(9, 7)
    clients[0]["b"][1] = -INF
    clients[3]["b"][1] = -INF
    with pytest.raises(NaNAggregationError) as e:
        run_algo(hip_device, clients, 1)
    assert e.value.stage == "accumulator"
    # a lone infinity is legal, its client is not picked, and the context is usable after the errors
    clients[3]["b"][1] = 0.5
    algo, msg = check_round(hip_device, clients, 1)
    assert 10 not in algo.last_selection.picked and bool(torch.isfinite(msg.parameter["b"]).all())
