"""Krum / Multi-Krum without a GPU: hand-computed answers for the torch restatement
(tests/krum_reference.py) and for ``krum_select``, and ``KrumFedAVGAlgorithm`` on the CPU device
against the restatement and, bit for bit, against the FedAvg oracle run on the chosen messages.
Neither rule is a reference algorithm; the restatement is what parity means.
The last section checks the order-exact restatement itself: that its data can tell the contract's
summation order from others, which is what makes the GPU comparison with it worth something."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    DeltaParameterMessage,
    KrumFedAVGAlgorithm,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from distributed_learning_simulation_lib_amd.fedavg import krum_select
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor
from oracle.fedavg_oracle import OracleFedAvg, OracleMessage
from tests import foreign_messages as fm
from tests import krum_reference as ref

INF = float("inf")
CPU = torch.device("cpu")


def f64(*xs):
    return torch.tensor(xs, dtype=torch.float64)


def bits(t) -> list[int]:
    t = torch.as_tensor(t).contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).reshape(-1).tolist()


# Five clients on a line at 0, 1, 3, 6, 10 (a second, constant tensor adds nothing):
#   D = (x_i - x_j)^2
LINE = [0.0, 1.0, 3.0, 6.0, 10.0]
LINE_D = [[0, 1, 9, 36, 100],
          [1, 0, 4, 25, 81],
          [9, 4, 0, 9, 49],
          [36, 25, 9, 0, 16],
          [100, 81, 49, 16, 0]]
# f = 1 (n = 2f + 3 exactly): the 2 smallest per row; f = 0: the 3 smallest
LINE_SCORES_F1 = [1 + 9, 1 + 4, 4 + 9, 9 + 16, 16 + 49]
LINE_SCORES_F0 = [1 + 9 + 36, 1 + 4 + 25, 4 + 9 + 9, 9 + 16 + 25, 16 + 49 + 81]


def line_clients(xs=LINE):
    return [{"a": f64(x, 0.5), "b": f64(2.0).reshape(1, 1)} for x in xs]


def run_algo(clients, f, m=1, weighted=False, out_dtype=torch.float64, msg_cls=ParameterMessage, weights=None, **kw):
    algo = KrumFedAVGAlgorithm(f, m, weighted=weighted, device=CPU, out_dtype=out_dtype)
    for wid, c in enumerate(clients):
        w = wid + 1 if weights is None else weights[wid]
        algo.process_worker_data(10 + wid, None if c is None else msg_cls(parameter=dict(c), aggregation_weight=w, **kw))
    return algo, algo.aggregate_worker_data()


def oracle_over(clients, chosen_rows, weights, out_dtype=torch.float64):
    """The FedAvg oracle (streaming path) run on the chosen clients in arrival order."""
    o = OracleFedAvg()
    for r in chosen_rows:
        o.process_worker_data(r, OracleMessage(parameter={k: v.numpy() for k, v in clients[r].items()},
                                               aggregation_weight=weights[r]))
    out = o.aggregate_parameter()
    return {k: torch.from_numpy(np.asarray(v).astype(np.float32 if out_dtype == torch.float32 else np.float64))
            for k, v in out.items()}


# ---- known answers ------------------------------------------------------------------------
@pytest.mark.parametrize("select", [ref.select, krum_select], ids=["restatement", "krum_select"])
def test_line_example(select):
    D = ref.distances([list(c.values()) for c in line_clients()])
    assert D.tolist() == LINE_D
    sc, rows = select(D, 1, 1)          # n = 2f + 3 exactly
    assert sc == LINE_SCORES_F1 and rows == [1]
    assert select(D, 1, 2)[1] == [0, 1]
    assert select(D, 1, 4)[1] == [0, 1, 2, 3]   # m = n - f: the far client alone is left out
    sc, rows = select(D, 0, 1)
    assert sc == LINE_SCORES_F0 and rows == [2]
    assert select(D, 0, 5)[1] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("select", [ref.select, krum_select], ids=["restatement", "krum_select"])
def test_tie_goes_to_the_earlier_arrival(select):
    D = ref.distances([[f64(x)] for x in (5.0, 0.0, 0.0, 1.0, 9.0)])
    sc, rows = select(D, 1, 1)
    assert sc[1] == sc[2] == 1.0 and rows == [1]
    assert select(D, 1, 2)[1] == [1, 2]
    # ties inside a row: equal distances are taken in ascending j, which cannot change a sum
    D = ref.distances([[f64(x)] for x in (0.0, 1.0, -1.0, 2.0, -2.0)])
    assert select(D, 1, 1)[0][0] == 2.0


@pytest.mark.parametrize("select", [ref.select, krum_select], ids=["restatement", "krum_select"])
def test_rule_errors(select):
    D = ref.distances([[f64(x)] for x in LINE])
    for f, m in ((2, 1), (-1, 1), (1, 0), (1, 5), (0, 6)):   # n < 2f + 3; m outside [1, n - f]
        with pytest.raises(ValueError):
            select(D, f, m)


def test_scores_add_from_the_smallest():
    # 1 + 1 + 1e16 differs from 1e16 + 1 + 1 in fp64
    D = [[0.0, 1e16, 1.0, 1.0, 4e16], [1e16, 0.0, 1e16, 1e16, 4e16], [1.0, 1e16, 0.0, 1.0, 4e16],
         [1.0, 1e16, 1.0, 0.0, 4e16], [4e16] * 4 + [0.0]]
    sc, _ = krum_select(torch.tensor(D, dtype=torch.float64), 0, 1)
    assert sc[0] == (1.0 + 1.0) + 1e16 != (1e16 + 1.0) + 1.0
    assert sc == ref.select(torch.tensor(D, dtype=torch.float64), 0, 1)[0]


# ---- the class on the CPU device ------------------------------------------------------------
def test_class_on_the_line_example():
    clients = line_clients()
    algo, msg = run_algo(clients, 1, 1)
    assert algo.last_selection.worker_ids == [10, 11, 12, 13, 14]
    assert algo.last_selection.scores == LINE_SCORES_F1
    assert algo.last_selection.chosen == [11]
    assert list(msg.parameter) == ["a", "b"]
    # Krum's result is the chosen update converted to float64
    assert bits(msg.parameter["a"]) == bits(clients[1]["a"]) and msg.parameter["b"].shape == (1, 1)
    algo, msg = run_algo(clients, 1, None)   # num_selected=None: n - f
    assert algo.last_selection.chosen == [10, 11, 12, 13]
    assert msg.parameter["a"].tolist() == [(0.0 + 1.0 + 3.0 + 6.0) / 4.0, 0.5]
    algo, _ = run_algo(clients, None, 1)     # num_byzantine=None: (n - 3) // 2 = 1
    assert algo.last_selection.scores == LINE_SCORES_F1
    with pytest.raises(ValueError, match="2f \\+ 3"):
        run_algo(clients, 2, 1)
    with pytest.raises(ValueError, match="n - f"):
        run_algo(clients, 1, 5)
    with pytest.raises(ValueError):
        KrumFedAVGAlgorithm(-1, device=CPU)
    with pytest.raises(ValueError):
        KrumFedAVGAlgorithm(1, 0, device=CPU)
    with pytest.raises(TypeError):
        KrumFedAVGAlgorithm(1, device=CPU, out_dtype=torch.float16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_cpu_class_matches_restatement_and_oracle(dtype):
    gen = torch.Generator().manual_seed(7)
    shapes = {"w": (5, 7), "b": (3,), "s": ()}
    n, f = 9, 2
    P = 5 * 7 + 3 + 1
    base = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    clients = []
    for c in range(n):
        far = 40.0 if c in (2, 6) else 0.0     # two planted outliers
        clients.append({k: (base[k] + 0.05 * torch.randn(s, generator=gen, dtype=torch.float64) + far).to(dtype)
                        for k, s in shapes.items()})
    D = ref.distances([list(c.values()) for c in clients])
    for m in (1, 3, n - f):
        want_scores, want_rows = ref.select(D, f, m)
        assert 2 not in want_rows and 6 not in want_rows
        for weighted in (False, True):
            for out_dtype in (torch.float64, torch.float32):
                algo, msg = run_algo(clients, f, m, weighted=weighted, out_dtype=out_dtype)
                sel = algo.last_selection
                assert sel.chosen == [10 + r for r in want_rows]
                # both sides' distances are within (P + 2) * 2^-53 of exact, the n score adds n * 2^-53 more
                tol = 2 * (P + 2 + n) * 2.0 ** -53
                assert all(abs(a - b) <= tol * b for a, b in zip(sel.scores, want_scores))
                if dtype in (torch.float32, torch.float64):   # formats the oracle reads from numpy
                    ws = [float(i + 1) if weighted else 1.0 for i in range(n)]
                    want = oracle_over(clients, want_rows, ws, out_dtype)
                    assert list(msg.parameter) == list(want)
                    for name in want:
                        got = msg.parameter[name]
                        assert got.dtype == out_dtype and got.shape == clients[0][name].shape
                        assert bits(got) == bits(want[name].reshape(got.shape)), (name, m, weighted, out_dtype)


def test_skipped_clients_do_not_count():
    clients = line_clients([0.0, 50.0, 1.0, 3.0, 6.0, 10.0])
    clients[1] = None
    algo, msg = run_algo(clients, 1, 1)
    assert algo.skipped_workers == {11}
    assert algo.last_selection.worker_ids == [10, 12, 13, 14, 15]
    assert algo.last_selection.scores == LINE_SCORES_F1 and algo.last_selection.chosen == [12]
    assert msg.parameter["a"].tolist() == [1.0, 0.5]


def test_missing_key_and_shape_are_refused():
    clients = line_clients()
    del clients[3]["b"]
    with pytest.raises(ValueError, match="client 13 lacks tensor b"):
        run_algo(clients, 1, 1)
    clients = line_clients()
    clients[2]["a"] = f64(1.0, 2.0, 3.0)
    with pytest.raises(ValueError, match="shape"):
        run_algo(clients, 1, 1)


def test_delta_and_quantised_payloads_are_refused():
    algo = KrumFedAVGAlgorithm(1, device=CPU)
    assert not algo.accepts_delta_messages and not algo.accepts_quantized_messages
    with pytest.raises(NotImplementedError, match="[Dd]elta"):
        algo.process_worker_data(0, DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1))
    with pytest.raises(NotImplementedError):
        algo.process_worker_data(0, fm.DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1))
    q = QuantizedTensor.__new__(QuantizedTensor)
    with pytest.raises(NotImplementedError, match="dequantise"):
        algo.process_worker_data(0, ParameterMessage(parameter={"a": q}, aggregation_weight=1))


def test_more_than_256_clients_are_refused():
    algo = KrumFedAVGAlgorithm(1, device=CPU)
    for wid in range(257):
        algo.process_worker_data(wid, ParameterMessage(parameter={"a": f64(float(wid))}, aggregation_weight=1))
    with pytest.raises(NotImplementedError, match="256"):
        algo.aggregate_worker_data()


def test_nan_and_infinities():
    clients = line_clients()
    clients[3]["a"] = f64(float("nan"), 0.5)
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, 1, 1)
    assert e.value.stage == "input" and e.value.bad_clients == [3]
    with pytest.raises(ref.KrumNaN) as r:
        ref.distances([list(c.values()) for c in clients])
    assert r.value.stage == "input"
    # a lone infinity is legal: its distances are +inf and it is never chosen
    clients = line_clients()
    clients[1]["a"] = f64(INF, 0.5)
    D = ref.distances([list(c.values()) for c in clients])
    assert D[1].tolist() == [INF, 0.0, INF, INF, INF]
    algo, msg = run_algo(clients, 1, 4)
    assert algo.last_selection.scores[1] == INF and algo.last_selection.chosen == [10, 12, 13, 14]
    assert algo.last_selection.chosen == [10 + r for r in ref.select(D, 1, 4)[1]]
    assert math.isfinite(msg.parameter["a"].sum().item())
    # two clients with a same-signed infinity in the same element: inf - inf
    clients[4]["a"] = f64(INF, 0.5)
    with pytest.raises(NaNAggregationError) as e:
        run_algo(clients, 1, 1)
    assert e.value.stage == "accumulator"
    with pytest.raises(ref.KrumNaN) as r:
        ref.distances([list(c.values()) for c in clients])
    assert r.value.stage == "accumulator"
    # opposite signs are a distance of +inf, not an error
    clients[4]["a"] = f64(-INF, 0.5)
    algo, _ = run_algo(clients, 1, 1)
    assert algo.last_selection.chosen == [12]   # rows 0, 2, 3 at 0, 3, 6: the middle one


def test_message_fields_follow_fedavg():
    clients = line_clients()
    algo = KrumFedAVGAlgorithm(1, device=CPU)
    algo.aggregate_loss = True
    for wid, c in enumerate(clients):
        algo.process_worker_data(wid, ParameterMessage(
            parameter=c, aggregation_weight=1 + wid, end_training=True, in_round=True,
            other_data={"training_loss": float(wid), "tag": "x"}))
    msg = algo.aggregate_worker_data()
    assert isinstance(msg, ParameterMessage) and msg.end_training and msg.in_round
    assert set(msg.other_data) == {"training_loss", "tag"} and msg.other_data["tag"] == "x"
    assert math.isclose(msg.other_data["training_loss"], sum((1 + w) * float(w) for w in range(5)) / 15)
    algo.clear_worker_data()
    algo.aggregate_loss = False
    for wid, c in enumerate(clients):
        algo.process_worker_data(wid, ParameterMessage(parameter=c, aggregation_weight=1, other_data={"tag": wid}))
    with pytest.raises(RuntimeError, match="different values on key tag"):
        algo.aggregate_worker_data()


def test_foreign_wire_classes():
    _, msg = run_algo(line_clients(), 1, 1, msg_cls=fm.ParameterMessage, in_round=True)
    assert type(msg) is fm.ParameterMessage and msg.in_round
    assert msg.parameter["a"].tolist() == [1.0, 0.5]


def test_registration_names_resolve():
    for name, selected in (("krum", 1), ("multi_krum", None)):
        assert AlgorithmRepository.has_algorithm(name)
        entry = AlgorithmRepository.config[name]
        assert entry["server_cls"] is AlgorithmRepository.config["fed_trimmed_mean"]["server_cls"]
        assert entry.get("client_cls") is AlgorithmRepository.config["fed_trimmed_mean"].get("client_cls")
        algo = entry["algorithm_cls"]()
        assert isinstance(algo, KrumFedAVGAlgorithm) and algo.num_selected == selected and not algo.weighted


# ---- the order-exact restatement: can its data tell one summation order from another? -----------
# tests/test_gpu_krum_contract.py compares the kernel bit for bit with ``ref.distances_in_order`` on
# ``ref.order_sensitive_values``. That is worth something only if (a) the kernel's FMA and the
# restatement's multiply-then-add agree, i.e. every square is exact, and (b) another order would
# give other bits. Both are conditions on the inputs and are established here, on the layouts of
# that module's order test at n = 17.
ORDER_DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
ORDER_N = 17


def order_case(code, n=ORDER_N):
    """(sizes, chunk, rows of float64 tensors): the layout and the data of the GPU module's order
    test (same sizes, same seed)."""
    from tests.test_gpu_krum_contract import order_layout, order_rows

    sizes = order_layout(code)
    return sizes, _native.kernel_constant("krum_chunk"), order_rows(n, sizes)


def bits_differ(a, b) -> int:
    """Pairs i < j whose entries differ in bits."""
    iu, ju = np.triu_indices(a.shape[0], 1)
    x = a.contiguous().view(torch.int64).numpy()[iu, ju]
    y = b.contiguous().view(torch.int64).numpy()[iu, ju]
    return int((x != y).sum())


def reversed_partials(rows, chunk):
    """A wrong order: the chunk partials added from the last chunk to the first."""
    partials, iu, ju = ref.chunk_partials(rows, chunk)
    total = np.zeros(len(iu))
    for p in partials[::-1]:
        total = total + p
    D = torch.zeros((len(rows), len(rows)), dtype=torch.float64)
    D[iu, ju] = torch.from_numpy(total)
    return D + D.t()


def two_accumulators(rows, chunk):
    """A wrong order: a chunk's even and odd elements in two accumulators, added at its end."""
    n = len(rows)
    iu, ju = np.triu_indices(n, 1)
    total = np.zeros(len(iu))
    for t in range(len(rows[0])):
        x = np.stack([r[t].to(torch.float64).numpy() for r in rows], axis=1)
        for start in range(0, x.shape[0], chunk):
            acc = [np.zeros(len(iu)), np.zeros(len(iu))]
            for e, row in enumerate(x[start:start + chunk]):
                d = row[iu] - row[ju]
                acc[e % 2] = acc[e % 2] + d * d
            total = total + (acc[0] + acc[1])
    D = torch.zeros((n, n), dtype=torch.float64)
    D[iu, ju] = torch.from_numpy(total)
    return D + D.t()


@pytest.mark.parametrize("code", list(ORDER_DTYPES))
def test_order_sensitive_values_are_exact_in_every_format(code):
    sizes, _, rows = order_case(code)
    flat = torch.cat([torch.cat(r) for r in rows])
    assert flat.dtype == torch.float64 and bool(torch.isfinite(flat).all()) and bool((flat != 0).all())
    for dtype in ORDER_DTYPES.values():   # the drawn values round-trip through all four formats
        assert bits(flat.to(dtype).to(torch.float64)) == bits(flat), dtype
    # every square of a difference is exact: 2000 element pairs of random clients, as rationals
    gen = torch.Generator().manual_seed(5)
    P = sum(sizes)
    x = torch.stack([torch.cat(r) for r in rows])
    e = torch.randint(0, P, (2000,), generator=gen)
    i = torch.randint(0, ORDER_N, (2000,), generator=gen)
    j = (i + 1 + torch.randint(0, ORDER_N - 1, (2000,), generator=gen)) % ORDER_N
    for a, b in zip(x[i, e].tolist(), x[j, e].tolist()):
        d = a - b
        assert Fraction(a) - Fraction(b) == Fraction(d)
        assert Fraction(d) * Fraction(d) == Fraction(d * d)


@pytest.mark.parametrize("code", list(ORDER_DTYPES))
def test_in_order_restatement_tells_orders_apart(code):
    sizes, chunk, rows = order_case(code)
    pairs = ORDER_N * (ORDER_N - 1) // 2
    D = ref.distances_in_order(rows, chunk)
    assert D.dtype == torch.float64 and D.shape == (ORDER_N, ORDER_N)
    assert bits(D) == bits(D.t().contiguous()) and not any(bits(torch.diagonal(D)))
    plain = ref.distances(rows)
    one_chunk = ref.distances_in_order([[torch.cat(r)] for r in rows], sum(sizes))   # no chunk boundary
    k_plain, k_one = bits_differ(D, plain), bits_differ(D, one_chunk)
    k_rev, k_two = bits_differ(D, reversed_partials(rows, chunk)), bits_differ(D, two_accumulators(rows, chunk))
    print(f"{code}: sizes {sizes}: distances_in_order differs in bits from ref.distances in {k_plain} of {pairs} "
          f"pairs, from the no-chunk variant in {k_one}, from reversed chunk partials in {k_rev}, "
          f"from two interleaved accumulators in {k_two}")
    assert 2 * k_plain >= pairs
    assert k_one >= 1
    assert k_rev >= 1 and k_two >= 1     # a kernel with either wrong order would fail the GPU test
    # and it is a summation of the same terms: within the contract's bound of the plain restatement
    bound = 2 * (sum(sizes) + 2) * 2.0 ** -53
    assert bool(((D - plain).abs() <= bound * plain).all())


def test_fused_restatement_agrees_where_squares_are_exact_and_differs_elsewhere():
    gen = torch.Generator().manual_seed(11)
    sizes, chunk = [5, 70, 3], 32
    rows = [[ref.order_sensitive_values(gen, s) for s in sizes] for _ in range(4)]
    assert bits(ref.distances_in_order_fused(rows, chunk)) == bits(ref.distances_in_order(rows, chunk))
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes] for _ in range(4)]
    fused, plain = ref.distances_in_order_fused(rows, chunk), ref.distances_in_order(rows, chunk)
    assert bits_differ(fused, plain) >= 1     # N(0, 1): the FMA's single rounding shows
    assert bool(((fused - plain).abs() <= 2 * (sum(sizes) + 2) * 2.0 ** -53 * plain).all())
