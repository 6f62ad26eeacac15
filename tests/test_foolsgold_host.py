"""FoolsGold without a GPU: the rule and the class on the CPU device against the independent numpy
restatement (tests/foolsgold_reference.py), hand cases, the history discipline, refusals."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    DeltaParameterMessage,
    FoolsGoldFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from distributed_learning_simulation_lib_amd.rules import foolsgold_coefficients
from tests import foolsgold_reference as ref

CPU = torch.device("cpu")
SHAPES = {"a": (5,), "b": (2, 3)}


def fbits(xs) -> list[int]:
    return np.asarray(xs, dtype=np.float64).reshape(-1).view(np.int64).tolist()


def clients(seed: int, n: int, dtype=torch.float32):
    """Integer values: every Gram entry is exact in any summation order, so the class's float64 matmul
    and the restatement's agree bit for bit."""
    gen = torch.Generator().manual_seed(seed)
    return [{k: torch.randint(-32, 33, s, generator=gen).to(dtype) for k, s in SHAPES.items()} for _ in range(n)]


def run_round(algo, updates, previous):
    for wid, c in enumerate(updates):
        algo.process_worker_data(10 + wid, None if c is None else ParameterMessage(parameter=dict(c), aggregation_weight=3))
    algo.set_old_parameter(previous)
    try:
        return algo.aggregate_worker_data().parameter
    finally:
        algo.clear_worker_data()                                  # as the server does between rounds


def arrays(c):
    return [t.to(torch.float64).numpy() for t in c.values()]


@pytest.mark.parametrize("n,kappa", [(2, 1.0), (5, 1.0), (9, 0.5), (16, 2.0)])
def test_rule_against_the_restatement(n, kappa):
    R = np.random.default_rng(n).standard_normal((n, 7))
    R[1] = R[0] * 0.5 + 0.01 * R[-1]           # a near-duplicate pair
    G = R @ R.T
    got, want = foolsgold_coefficients(G, kappa), ref.coefficients(G, kappa)
    assert fbits(got[0]) == fbits(want[0]) and fbits(got[1]) == fbits(want[1])
    assert fbits(foolsgold_coefficients(torch.from_numpy(G), kappa)[0]) == fbits(want[0])


def test_rule_hand_cases():
    assert foolsgold_coefficients([[4.0]]) == ([1.0], [0.0])                       # n = 1
    e = np.eye(4)
    R = np.stack([e[0] + e[1], e[0] + e[1], e[2], e[3]])                            # two identical, two honest
    alphas, cosines = foolsgold_coefficients(R @ R.T)
    assert alphas == [0.0, 0.0, 1.0, 1.0] and cosines[:2] == pytest.approx([1.0, 1.0]) and cosines[2:] == [0.0, 0.0]
    assert foolsgold_coefficients(np.ones((3, 3))) == ([0.0] * 3, [1.0] * 3)       # all identical: W == 0
    R = np.stack([e[0], e[1], np.zeros(4)])                                         # a zero-norm client: cosine 0.0
    assert foolsgold_coefficients(R @ R.T) == ([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    for bad in ([[1.0, float("nan")], [float("nan"), 1.0]], [[float("inf")]], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            foolsgold_coefficients(bad)
    for kappa in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            foolsgold_coefficients(np.eye(2), kappa)


@pytest.mark.parametrize("dtype,out_dtype", [(torch.float32, torch.float64), (torch.bfloat16, torch.float32)])
def test_class_on_cpu_two_rounds_history_skip_and_checkpoint(dtype, out_dtype):
    previous = {k: torch.randint(-32, 33, s, generator=torch.Generator().manual_seed(7)).to(torch.float64) for k, s in SHAPES.items()}
    point = arrays(previous)
    first, second = clients(1, 4, dtype), clients(2, 4, dtype)
    first[1] = {k: t.clone() for k, t in first[0].items()}       # worker 11 copies worker 10 in round 1
    second[2] = None                                              # worker 12 skips round 2
    algo = FoolsGoldFedAVGAlgorithm(device=CPU, out_dtype=out_dtype)
    np_out = np.float32 if out_dtype == torch.float32 else np.float64
    zeros = [[np.zeros(s) for s in SHAPES.values()] for _ in range(4)]
    got1 = run_round(algo, first, previous)
    want1, hist1, alphas1, _ = ref.foolsgold_round([arrays(c) for c in first], point, zeros, out_dtype=np_out)
    assert alphas1[0] == alphas1[1] == 0.0 and fbits(algo.last_foolsgold.alphas) == fbits(alphas1)
    assert algo.last_foolsgold.worker_ids == [10, 11, 12, 13]
    for g, w in zip(got1.values(), want1):
        assert g.dtype == out_dtype and np.array_equal(g.numpy().view(np.uint8), w.view(np.uint8))

    restored = FoolsGoldFedAVGAlgorithm(device=CPU, out_dtype=out_dtype)
    restored.load_state_dict(algo.state_dict())                   # round 2 from the checkpoint gives the same bits
    kept = [0, 1, 3]
    want2, hist2, alphas2, _ = ref.foolsgold_round([arrays(second[i]) for i in kept], point, [hist1[i] for i in kept],
                                                   out_dtype=np_out)
    for a in (algo, restored):
        got2 = run_round(a, second, previous)
        assert a.last_foolsgold.worker_ids == [10, 11, 13] and fbits(a.last_foolsgold.alphas) == fbits(alphas2)
        for g, w in zip(got2.values(), want2):
            assert np.array_equal(g.numpy().view(np.uint8), w.view(np.uint8))
        state = a.state_dict()["history"]
        for i, h in zip(kept, hist2):                             # carried over
            assert all(fbits(t) == fbits(x) for t, x in zip(state[10 + i].values(), h))
        assert all(fbits(t) == fbits(x) for t, x in zip(state[12].values(), hist1[2]))   # the skipped worker's: untouched


@pytest.mark.parametrize("poison,stage", [(float("nan"), "input"), (float("inf"), "accumulator")])
def test_nan_or_infinite_client_leaves_the_histories_unchanged(poison, stage):
    previous = {k: torch.zeros(s, dtype=torch.float64) for k, s in SHAPES.items()}
    algo = FoolsGoldFedAVGAlgorithm(device=CPU)
    run_round(algo, clients(3, 3), previous)
    before = algo.state_dict()["history"]
    bad = clients(4, 4)                                           # worker 13 is new in the failed round
    bad[1]["a"][2] = poison
    with pytest.raises(NaNAggregationError) as e:
        run_round(algo, bad, previous)
    assert e.value.stage == stage and (stage == "input" or e.value.bad_clients == [11])
    after = algo.state_dict()["history"]
    assert list(after) == [10, 11, 12]
    assert all(fbits(after[w][k]) == fbits(before[w][k]) for w in before for k in SHAPES)


def test_refusals_and_registration():
    assert AlgorithmRepository.has_algorithm("fed_foolsgold")
    assert not FoolsGoldFedAVGAlgorithm.accepts_delta_messages and not FoolsGoldFedAVGAlgorithm.accepts_quantized_messages
    for kappa in (0.0, float("nan")):
        with pytest.raises(ValueError):
            FoolsGoldFedAVGAlgorithm(kappa=kappa)
    with pytest.raises(TypeError):
        FoolsGoldFedAVGAlgorithm(out_dtype=torch.float16)
    algo = FoolsGoldFedAVGAlgorithm(device=CPU)
    with pytest.raises(NotImplementedError):
        algo.process_worker_data(1, DeltaParameterMessage(delta_parameter={"a": torch.zeros(5)}, aggregation_weight=1))
    x = {"a": torch.zeros(1)}
    with pytest.raises(NotImplementedError, match=str(_native.GRAM_MAX_CLIENTS)):
        run_round(FoolsGoldFedAVGAlgorithm(device=CPU), [x] * (_native.GRAM_MAX_CLIENTS + 1), {"a": torch.zeros(1)})
    with pytest.raises(ValueError):                               # no previous model: no centre
        a = FoolsGoldFedAVGAlgorithm(device=CPU)
        a.process_worker_data(1, ParameterMessage(parameter=x, aggregation_weight=1))
        a.aggregate_worker_data()
    off = FoolsGoldFedAVGAlgorithm(use_history=False, device=CPU)  # keeps no state
    run_round(off, clients(5, 3), {k: torch.zeros(s, dtype=torch.float64) for k, s in SHAPES.items()})
    assert off.state_dict()["history"] == {}
    with pytest.raises(ValueError):
        off.load_state_dict({"history": {}})
