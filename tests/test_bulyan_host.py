"""Bulyan on the host (no GPU): ``fedavg.bulyan_select``, the CPU path of the coordinate step and
``BulyanFedAVGAlgorithm(device="cpu")`` against the independent restatement
(tests/bulyan_reference.py). Everything is compared bit for bit.

The package counts the window's start (``a = #{t : (s_{t+beta} - med) < (med - s_t)}``), the
restatement shrinks the window from its ends: the two forms are compared on values full of ties,
signed zeros, subnormals of every input format, 1e308 and infinities of both signs.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    BulyanFedAVGAlgorithm,
    DeltaParameterMessage,
    NaNAggregationError,
    ParameterMessage,
)
from distributed_learning_simulation_lib_amd.algorithm.bulyan_aggregation_algorithm import (
    BulyanSelection,
    mean_around_median_cpu,
)
from distributed_learning_simulation_lib_amd.fedavg import bulyan_select
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor
from tests import bulyan_reference as ref
from tests import robust_reference as robust_ref

CPU = torch.device("cpu")
INF = float("inf")
# ties, zeros of both signs, a subnormal of every input format (2^-24: fp16; 2^-130: fp32 / bf16;
# 2^-1030: fp64), large magnitudes
FINITE = [0.0, -0.0, 1.0, 1.0, -1.0, 1.5, 0.1, -7.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -130, -(2.0 ** -130),
          2.0 ** -1030, -(2.0 ** -1030), 6.0e4, -6.0e4, 1e308, -1e308]


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def pooled(rng: np.random.Generator, pool: list[float], shape) -> np.ndarray:
    return np.asarray(pool, dtype=np.float64)[rng.integers(0, len(pool), size=shape)]


# ---- selection ----------------------------------------------------------------------------------
def random_D(rng: np.random.Generator, n: int, inf_rows: int) -> np.ndarray:
    """Symmetric, zero diagonal, small integers (exact ties are frequent), some rows at +inf."""
    A = rng.integers(1, 6, size=(n, n)).astype(np.float64)
    D = np.triu(A, 1)
    D = D + D.T
    for r in rng.choice(n, size=inf_rows, replace=False):
        D[r, :] = D[:, r] = INF
        D[r, r] = 0.0
    return D


@pytest.mark.parametrize("n,f", [(3, 0), (7, 1), (11, 2), (12, 2), (35, 8)])
def test_selection_matches_restatement(n, f):
    rng = np.random.default_rng(100 * n + f)
    for trial in range(8):
        D = random_D(rng, n, inf_rows=trial % 3 if n > 3 else 0)
        picked, scores = bulyan_select(torch.from_numpy(D), f)
        want_picked, want_scores = ref.select(D, f)
        assert picked == want_picked and bits(np.asarray(scores)).tolist() == bits(np.asarray(want_scores)).tolist()
        assert len(picked) == n - 2 * f and len(set(picked)) == len(picked)
        assert bulyan_select(D.tolist(), f) == (picked, scores)   # nested lists are taken too


def test_selection_last_steps_and_ties():
    # n = 3, f = 0: r = 3 (c = 1), r = 2 (c = max(1, -0) = 1), r = 1 (the row that is left, 0.0)
    D = [[0.0, 4.0, 1.0],
         [4.0, 0.0, 2.0],
         [1.0, 2.0, 0.0]]
    # rows 0 and 2 tie at 1.0, then rows 1 and 2 at 2.0: the earlier row each time
    assert bulyan_select(D, 0) == ([0, 1, 2], [1.0, 2.0, 0.0])
    assert ref.select(D, 0) == ([0, 1, 2], [1.0, 2.0, 0.0])
    # all distances equal: every pick is a tie and goes to the earliest row left
    E = [[0.0 if i == j else 3.0 for j in range(7)] for i in range(7)]
    assert bulyan_select(E, 1) == ([0, 1, 2, 3, 4], [12.0, 9.0, 6.0, 3.0, 3.0])
    # the neighbours tie: ascending j decides which enter the sum, the sum adds from the smallest
    big = 2.0 ** 53
    T = [[0.0, 1.0, big, 1.0, big, big, big],
         [1.0, 0.0, big, big, big, big, big],
         [big, big, 0.0, big, big, big, big],
         [1.0, big, big, 0.0, big, big, big],
         [big, big, big, big, 0.0, big, big],
         [big, big, big, big, big, 0.0, big],
         [big, big, big, big, big, big, 0.0]]
    picked, scores = bulyan_select(T, 1)
    assert picked[0] == 0 and scores[0] == (((0.0 + 1.0) + 1.0) + big) + big   # c = 7 - 1 - 2 = 4
    assert (picked, scores) == ref.select(T, 1)
    # a far row is never picked
    rng = np.random.default_rng(5)
    D = random_D(rng, 11, 0)
    D[4, :] = D[:, 4] = 1e6
    D[9, :] = D[:, 9] = 1e6
    D[4, 4] = D[9, 9] = 0.0
    picked, _ = bulyan_select(D, 2)
    assert 4 not in picked and 9 not in picked


def test_selection_refusals():
    ok = np.zeros((7, 7))
    for f, n in ((2, 7), (-1, 7), (1, 6), (0, 2)):
        with pytest.raises(ValueError, match="4f \\+ 3"):
            bulyan_select(np.zeros((n, n)), f)
    with pytest.raises(ValueError, match="square"):
        bulyan_select(ok[:, :6], 1)
    with pytest.raises(ValueError):
        ref.select(ok, 2)


# ---- the coordinate step ------------------------------------------------------------------------
def package_mam(x: np.ndarray, beta: int) -> np.ndarray:
    return mean_around_median_cpu([torch.from_numpy(r.copy()) for r in x], beta).numpy()


@pytest.mark.parametrize("n", range(1, 15))
def test_count_form_equals_shrink_form(n):
    rng = np.random.default_rng(n)
    for beta in range(1, n + 1):
        # infinities of one sign per batch, and no 1e308 of the other sign (a sum may overflow): no
        # result can be NaN, whole batches are compared
        for inf in (INF, -INF):
            x = pooled(rng, [v for v in FINITE if v != (-1e308 if inf > 0 else 1e308)] + [inf, inf, inf], (n, 96))
            got, want = package_mam(x, beta), ref.mean_around_median(list(x), beta)
            assert np.array_equal(bits(got), bits(want)), (n, beta, inf)
        # both signs: column by column, so that a NaN result of one column does not hide the others
        x = pooled(rng, [0.0, -0.0, 1.0, -1.0, 1e308, -1e308, INF, INF, -INF, -INF], (n, 10))
        for col in range(x.shape[1]):
            c = x[:, col:col + 1]
            try:
                want = ref.mean_around_median(list(c), beta)
            except ref.BulyanNaN as err:
                assert err.stage == "result"
                with pytest.raises(NaNAggregationError) as e:
                    package_mam(c, beta)
                assert e.value.stage == "result"
                continue
            assert np.array_equal(bits(package_mam(c, beta)), bits(want)), (n, beta, c.T.tolist())


def test_window_examples():
    # med = 5 (lower median of 6 values is s_2); the three closest values are 4, 5, 5.5
    x = np.asarray([[0.0], [4.0], [5.0], [5.5], [9.0], [20.0]])
    for fn in (package_mam, lambda v, b: ref.mean_around_median(list(v), b)):
        assert fn(x, 3).tolist() == [(4.0 + 5.0 + 5.5) / 3.0]
        assert fn(x, 1).tolist() == [5.0]
        assert fn(x, 6).tolist() == [((((0.0 + 4.0) + 5.0) + 5.5) + 9.0 + 20.0) / 6.0]
    # a tie between the value below and the value above: the lower one stays
    t = np.asarray([[1.0], [2.0], [3.0], [4.0]])            # med = 2; |1 - 2| = |3 - 2|
    for fn in (package_mam, lambda v, b: ref.mean_around_median(list(v), b)):
        assert fn(t, 2).tolist() == [1.5]
    # signed zeros: the sum starts at s_a, so a window of -0.0 alone stays -0.0
    z = np.asarray([[-0.0], [-0.0], [-0.0], [0.0], [7.0]])
    for fn in (package_mam, lambda v, b: ref.mean_around_median(list(v), b)):
        assert np.signbit(fn(z, 2)).tolist() == [True] and np.signbit(fn(z, 4)).tolist() == [False]
    # NaN input
    bad = np.asarray([[1.0], [float("nan")], [2.0]])
    with pytest.raises(NaNAggregationError) as e:
        package_mam(bad, 1)
    assert e.value.stage == "input" and e.value.bad_clients == [1]
    with pytest.raises(ref.BulyanNaN) as r:
        ref.mean_around_median(list(bad), 1)
    assert r.value.stage == "input"
    with pytest.raises(ValueError):
        package_mam(t, 0)
    with pytest.raises(ValueError):
        package_mam(t, 5)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 13])
def test_cross_checks_against_the_robust_restatement(n):
    """``keep = n`` is the sorted-order mean and ``keep = 1`` the lower median, bit for bit. The pool
    holds one zero only: a -0.0 below a +0.0 median ties with it (IEEE ``==``) and, as ties do not
    slide, stays — the case after the loop."""
    rng = np.random.default_rng(40 + n)
    x = pooled(rng, [v for v in FINITE if not (v == 0.0 and np.signbit(v))], (n, 200))
    rows = [torch.from_numpy(r.copy()) for r in x]
    mean = robust_ref.reduce_tensor(rows, "trimmed_mean", 0.0)
    sorted_x = robust_ref.sort_total_order(torch.stack(rows))
    lower_median = sorted_x[(n - 1) // 2]
    for fn in (package_mam, lambda v, b: ref.mean_around_median(list(v), b)):
        assert np.array_equal(bits(fn(x, n)), bits(mean))
        assert np.array_equal(bits(fn(x, 1)), bits(lower_median))
        if n % 2 == 1:
            assert np.array_equal(bits(fn(x, 1)), bits(robust_ref.reduce_tensor(rows, "median")))
    z = np.asarray([[-0.0], [0.0], [0.0], [5.0]])      # the lower median s_1 is +0.0; s_0 = -0.0 ties with it
    for fn in (package_mam, lambda v, b: ref.mean_around_median(list(v), b)):
        assert fn(z, 1).tolist() == [0.0] and np.signbit(fn(z, 1)).tolist() == [True]


# ---- the class on a CPU device ------------------------------------------------------------------
SHAPES = {"w": (37,), "b": (5,), "m": (3, 7), "scalar": (), "empty": (0,)}


def dyadic_clients(rng: np.random.Generator, n: int, dtype=torch.float64) -> list[dict[str, torch.Tensor]]:
    """Integers / 8 in [-4, 4]: every difference, square and sum of the distances is exact."""
    return [{k: (torch.as_tensor(rng.integers(-32, 33, size=s), dtype=torch.float64) / 8.0).to(dtype)
             for k, s in SHAPES.items()} for _ in range(n)]


def as_numpy(clients):
    return [None if c is None else {k: v.to(torch.float64).numpy() for k, v in c.items()} for c in clients]


def run_algo(clients, f, out_dtype=torch.float64, first_id=10):
    algo = BulyanFedAVGAlgorithm(num_byzantine=f, device=CPU, out_dtype=out_dtype)
    for k, c in enumerate(clients):
        algo.process_worker_data(first_id + k, None if c is None else
                                 ParameterMessage(parameter=c, aggregation_weight=1 + 3 * k))
    return algo, algo.aggregate_worker_data()


def check_round(clients, f, out_dtype=torch.float64):
    algo, msg = run_algo(clients, f, out_dtype)
    np_dtype = np.float64 if out_dtype == torch.float64 else np.float32
    want, picked, scores, (wf, theta, beta) = ref.bulyan_round(as_numpy(clients), f, np_dtype)
    ids = [10 + k for k, c in enumerate(clients) if c is not None]
    sel = algo.last_selection
    assert isinstance(sel, BulyanSelection)
    assert sel.worker_ids == ids and sel.picked == [ids[r] for r in picked] and sel.scores == scores
    assert (sel.f, sel.theta, sel.beta) == (wf, theta, beta)
    assert list(msg.parameter) == list(want)
    for name, w in want.items():
        got = msg.parameter[name]
        assert got.dtype == out_dtype and tuple(got.shape) == w.shape
        assert np.array_equal(bits(got), bits(w)), name
    return algo, msg


@pytest.mark.parametrize("out_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,f", [(3, 0), (7, 1), (11, 2), (12, 0), (12, None), (16, 3)])
def test_cpu_rounds_match_restatement(n, f, out_dtype):
    rng = np.random.default_rng(7 * n + (f or 0))
    clients = dyadic_clients(rng, n, torch.float32 if n == 11 else torch.float64)
    if n == 12:
        clients.insert(4, None)   # a skipped client does not count
    check_round(clients, f, out_dtype)


def test_f_zero_is_the_sorted_order_mean():
    rng = np.random.default_rng(3)
    clients = dyadic_clients(rng, 6)
    algo, msg = check_round(clients, 0)
    assert sorted(algo.last_selection.picked) == algo.last_selection.worker_ids
    for name in SHAPES:
        want = robust_ref.reduce_tensor([c[name] for c in clients], "trimmed_mean", 0.0)
        assert np.array_equal(bits(msg.parameter[name]), bits(want))


def test_planted_far_clients_are_left_out():
    rng = np.random.default_rng(9)
    clients = dyadic_clients(rng, 11)
    far = (2, 7)
    for r, sign in zip(far, (1.0, -1.0)):
        clients[r] = {k: v + sign * 1024.0 for k, v in clients[r].items()}
    algo, msg = check_round(clients, 2)
    assert not {10 + r for r in far} & set(algo.last_selection.picked)
    honest = [c for r, c in enumerate(clients) if r not in far]
    for name in SHAPES:
        if name == "empty":
            continue
        stack = torch.stack([c[name] for c in honest])
        got = msg.parameter[name]
        assert bool((got >= stack.min(dim=0).values).all()) and bool((got <= stack.max(dim=0).values).all())


def test_aggregation_weight_is_ignored():
    rng = np.random.default_rng(11)
    clients = dyadic_clients(rng, 7)
    _, a = run_algo(clients, 1)
    algo = BulyanFedAVGAlgorithm(num_byzantine=1, device=CPU)
    for k, c in enumerate(clients):
        algo.process_worker_data(10 + k, ParameterMessage(parameter=c, aggregation_weight=1000 - 100 * k))
    b = algo.aggregate_worker_data()
    for name in SHAPES:
        assert np.array_equal(bits(a.parameter[name]), bits(b.parameter[name]))


def test_refusals():
    algo = BulyanFedAVGAlgorithm(1, device=CPU)
    assert not algo.accepts_delta_messages and not algo.accepts_quantized_messages
    one = torch.ones(1, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="[Dd]elta"):
        algo.process_worker_data(0, DeltaParameterMessage(delta_parameter={"a": one}, aggregation_weight=1))
    q = QuantizedTensor.__new__(QuantizedTensor)
    with pytest.raises(NotImplementedError, match="dequantise"):
        algo.process_worker_data(0, ParameterMessage(parameter={"a": q}, aggregation_weight=1))
    rng = np.random.default_rng(13)
    clients = dyadic_clients(rng, 7)
    del clients[3]["b"]
    with pytest.raises(ValueError, match="client 13 lacks tensor b"):
        run_algo(clients, 1)
    clients = dyadic_clients(rng, 7)
    clients[2]["w"] = torch.zeros(36, dtype=torch.float64)
    with pytest.raises(ValueError, match="client 12.*w.*shape"):
        run_algo(clients, 1)
    with pytest.raises(ValueError, match="4f \\+ 3"):
        run_algo(dyadic_clients(rng, 6), 1)
    with pytest.raises(ValueError, match="4f \\+ 3"):
        run_algo(dyadic_clients(rng, 2), None)
    with pytest.raises(ValueError):
        BulyanFedAVGAlgorithm(num_byzantine=-1)
    with pytest.raises(TypeError):
        BulyanFedAVGAlgorithm(out_dtype=torch.float16)
    # theta = n - 2f = 65 selected updates: more than the coordinate step sorts
    small = [{"a": torch.tensor([float(k)], dtype=torch.float64)} for k in range(67)]
    with pytest.raises(NotImplementedError, match="64"):
        run_algo(small, 1)
    with pytest.raises(NotImplementedError, match="256"):
        run_algo([{"a": torch.tensor([float(k)], dtype=torch.float64)} for k in range(257)], 63)


def test_nan_and_infinities():
    rng = np.random.default_rng(17)
    clients = dyadic_clients(rng, 7)
    clients[3]["w"][5] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, 1)
    assert e.value.stage == "input" and e.value.bad_clients == [3]
    with pytest.raises(ref.BulyanNaN) as r:
        ref.bulyan_round(as_numpy(clients), 1)
    assert r.value.stage == "input"
    # a lone infinity is legal: that client is at +inf from everyone and is not picked
    clients = dyadic_clients(rng, 7)
    clients[1]["b"][0] = INF
    algo, msg = check_round(clients, 1)
    assert 11 not in algo.last_selection.picked and bool(torch.isfinite(msg.parameter["b"]).all())
    # the same infinity in the same element of two clients: inf - inf in a distance
    clients[4]["b"][0] = INF
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, 1)
    assert e.value.stage == "accumulator"
    with pytest.raises(ref.BulyanNaN) as r:
        ref.bulyan_round(as_numpy(clients), 1)
    assert r.value.stage == "accumulator"


def test_registration_and_message_fields():
    assert AlgorithmRepository.has_algorithm("fed_bulyan")
    entry = AlgorithmRepository.config["fed_bulyan"]
    assert entry["server_cls"] is AlgorithmRepository.config["fed_trimmed_mean"]["server_cls"]
    assert entry.get("client_cls") is AlgorithmRepository.config["fed_trimmed_mean"].get("client_cls")
    algo = entry["algorithm_cls"]()
    assert isinstance(algo, BulyanFedAVGAlgorithm) and algo.num_byzantine is None and algo.last_selection is None
    rng = np.random.default_rng(19)
    algo = BulyanFedAVGAlgorithm(1, device=CPU)
    for wid, c in enumerate(dyadic_clients(rng, 7)):
        algo.process_worker_data(wid, ParameterMessage(parameter=c, aggregation_weight=1, end_training=True,
                                                       in_round=True, other_data={"tag": "x"}))
    msg = algo.aggregate_worker_data()
    assert isinstance(msg, ParameterMessage) and msg.end_training and msg.in_round and msg.other_data == {"tag": "x"}
    assert algo.last_selection._fields == ("worker_ids", "picked", "scores", "f", "theta", "beta")
