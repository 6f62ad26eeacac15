"""The FedOpt server optimisers without a GPU: ``fedavg.check_server_opt``,
``fedavg.server_opt_update`` and ``ServerOptFedAVGAlgorithm`` on the CPU device against the
independent numpy restatement (tests/opt_reference.py), bit for bit over consecutive
rounds, outputs and state; that a failed round leaves the state as it was; the checkpoint; the
registry; and the refusals. Not a reference algorithm: the restatement is what parity means."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    DeltaParameterMessage,
    NaNAggregationError,
    ParameterMessage,
    ServerOptFedAVGAlgorithm,
    _native,
)
from distributed_learning_simulation_lib_amd.fedavg import SERVER_OPT_MODES, check_server_opt, server_opt_update
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor
from tests import foreign_messages as fm
from tests import geomed_reference as geo
from tests import opt_reference as ref

INF = float("inf")
NAN = float("nan")
CPU = torch.device("cpu")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
HYPER = {"learning_rate": 0.03, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
ROUNDS = 3


def f64(*xs):
    return torch.tensor(xs, dtype=torch.float64)


def bits(t) -> list[int]:
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).reshape(-1).tolist()


def rounds_of(dtype, n=5, seed=3, with_empty=True):
    """The model before round 0 and ROUNDS rounds of n clients: the model plus a drifting step plus
    noise, in the client dtype. Shapes: a matrix, a vector, a 0-d tensor and an empty tensor."""
    gen = torch.Generator().manual_seed(seed)
    shapes = {"w": (5, 7), "b": (3,), "s": ()}
    if with_empty:
        shapes["e"] = (0, 4)
    start = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    rounds = []
    for r in range(ROUNDS):
        step = {k: 0.1 * torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
        rounds.append([{k: (start[k] + step[k] + 0.02 * torch.randn(s, generator=gen, dtype=torch.float64)).to(dtype)
                        for k, s in shapes.items()} for _ in range(n)])
    return start, rounds


def feed(algo, clients, previous, msg_cls=ParameterMessage):
    algo.clear_worker_data()
    for wid, c in enumerate(clients):
        algo.process_worker_data(10 + wid, None if c is None else msg_cls(parameter=dict(c), aggregation_weight=wid + 1))
    if previous is not None:
        algo.set_old_parameter(previous)
    return algo.aggregate_worker_data()


def state_bits(algo):
    sd = algo.state_dict()
    return (sd["rounds_done"], None if sd["m"] is None else {k: bits(t) for k, t in sd["m"].items()},
            None if sd["v"] is None else {k: bits(t) for k, t in sd["v"].items()})


def run_rounds(algo, start, rounds, want, out_dtype=torch.float64, first=0):
    """Rounds ``first ..`` of ``rounds`` through ``algo``, every round's result fed back as the next
    previous model, each checked bit for bit (outputs and state) against ``want`` (ref.rounds)."""
    previous = start
    for r in range(first, len(rounds)):
        msg = feed(algo, rounds[r], previous)
        outs, m, v = want[r]
        names = list(rounds[r][0])
        assert list(msg.parameter) == names and algo.rounds_done == r + 1
        sd = algo.state_dict()
        for i, name in enumerate(names):
            got = msg.parameter[name]
            assert got.dtype == out_dtype and got.shape == rounds[r][0][name].shape, name
            assert bits(got) == bits(outs[i]), (r, name)
            assert sd["m"][name].device.type == "cpu" and sd["m"][name].shape == got.shape
            assert bits(sd["m"][name]) == bits(m[i]), (r, name, "m")
            if v is None:
                assert sd["v"] is None
            else:
                assert bits(sd["v"][name]) == bits(v[i]), (r, name, "v")
        previous = msg.parameter
    return previous


def restated(start, rounds, mode, out_dtype=np.float64, **hyper):
    h = {**HYPER, **hyper}
    names = list(start)
    return ref.rounds([[list(c.values()) for c in cl] for cl in rounds],
                      [[float(i + 1) for i in range(len(cl))] for cl in rounds], [start[k] for k in names], mode,
                      h["learning_rate"], h["beta1"], h["beta2"], h["tau"], h.get("initial_second_moment"), out_dtype)


# ---- the host helpers ----------------------------------------------------------------------------
def test_check_server_opt_validates_like_the_c_call():
    assert SERVER_OPT_MODES == ("avgm", "adagrad", "yogi", "adam")
    assert (_native.OPT_AVGM, _native.OPT_ADAGRAD, _native.OPT_YOGI, _native.OPT_ADAM) == (0, 1, 2, 3)
    code, lr, b1, omb1, b2, omb2, tau = check_server_opt("yogi", 0.1, 0.9, 0.99, 1e-3)
    assert (code, lr, b1, b2, tau) == (2, 0.1, 0.9, 0.99, 1e-3)
    assert omb1 == 1.0 - 0.9 == ref.one_minus(0.9) and omb2 == 1.0 - 0.99 == ref.one_minus(0.99)
    assert check_server_opt("avgm", 1, 0, 0, NAN)[0] == 0            # avgm ignores tau; beta = 0 is allowed
    with pytest.raises(ValueError, match="mode"):
        check_server_opt("sgd", 0.1, 0.9, 0.99, 1e-3)
    for lr in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="learning rate"):
            check_server_opt("adam", lr, 0.9, 0.99, 1e-3)
    for b in (-0.1, 1.0, 1.5, NAN, INF):
        with pytest.raises(ValueError, match="beta1"):
            check_server_opt("adam", 0.1, b, 0.99, 1e-3)
        with pytest.raises(ValueError, match="beta2"):
            check_server_opt("avgm", 0.1, 0.9, b, 1e-3)
    for tau in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="tau"):
            check_server_opt("adagrad", 0.1, 0.9, 0.99, tau)


@pytest.mark.parametrize("mode", SERVER_OPT_MODES)
def test_server_opt_update_is_the_restatement_line_by_line(mode):
    gen = torch.Generator().manual_seed(17)
    z = torch.zeros(600, dtype=torch.float64)
    x = geo.order_sensitive_values(gen, 600, torch.float64)
    m = torch.randn(600, generator=gen, dtype=torch.float64)
    v = torch.rand(600, generator=gen, dtype=torch.float64) * x * x * 2.0     # on both sides of delta^2 for yogi
    v[:3] = 0.0
    x[3:6] = 0.0
    x[4] = -0.0
    _, lr, b1, omb1, b2, omb2, tau = check_server_opt(mode, 0.07, 0.9, 0.99, 1e-3)
    m_new, v_new, u = server_opt_update(mode, x, m, None if mode == "avgm" else v, lr, b1, omb1, b2, omb2, tau)
    outs, wm, wv, flags = ref.step([[x]], [1.0], 1.0, [z], [m], [v], mode, 0.07, 0.9, 0.99, 1e-3)
    assert flags == 0
    assert bits(z + u) == bits(outs[0]) and bits(m_new) == bits(wm[0])
    assert (v_new is None and wv is None) if mode == "avgm" else bits(v_new) == bits(wv[0])


# ---- the constructor -----------------------------------------------------------------------------
def test_learning_rate_none_is_one_for_avgm_and_an_error_for_the_adaptive_optimisers():
    assert ServerOptFedAVGAlgorithm("avgm", device=CPU).learning_rate == 1.0
    for mode in ("adagrad", "yogi", "adam"):
        with pytest.raises(ValueError, match="no default"):
            ServerOptFedAVGAlgorithm(mode, device=CPU)
        assert ServerOptFedAVGAlgorithm(mode, 0.5, device=CPU).learning_rate == 0.5


def test_constructor_validation_and_defaults():
    a = ServerOptFedAVGAlgorithm("adam", 0.1, device=CPU)
    assert (a.beta1, a.beta2, a.tau, a.weighted, a.out_dtype) == (0.9, 0.99, 1e-3, True, torch.float64)
    assert a.initial_second_moment == 1e-3 * 1e-3 and a.rounds_done == 0 and a.last_step is None
    assert ServerOptFedAVGAlgorithm("adam", 0.1, tau=0.5, initial_second_moment=2.0, device=CPU).initial_second_moment == 2.0
    with pytest.raises(ValueError, match="optimizer"):
        ServerOptFedAVGAlgorithm("sgd", 0.1, device=CPU)
    for kw, match in (({"learning_rate": 0.0}, "learning rate"), ({"learning_rate": INF}, "learning rate"),
                      ({"beta1": 1.0}, "beta1"), ({"beta2": -0.5}, "beta2"), ({"tau": 0.0}, "tau"),
                      ({"initial_second_moment": -1.0}, "initial_second_moment"),
                      ({"initial_second_moment": NAN}, "initial_second_moment")):
        with pytest.raises(ValueError, match=match):
            ServerOptFedAVGAlgorithm("yogi", **{"learning_rate": 0.1, **kw}, device=CPU)
    with pytest.raises(TypeError):
        ServerOptFedAVGAlgorithm("avgm", out_dtype=torch.float16, device=CPU)
    assert not ServerOptFedAVGAlgorithm.accepts_delta_messages and not ServerOptFedAVGAlgorithm.accepts_quantized_messages


def test_registry_entries():
    for name, mode in (("fed_avgm", "avgm"), ("fed_adagrad", "adagrad"), ("fed_yogi", "yogi"), ("fed_adam", "adam")):
        assert AlgorithmRepository.has_algorithm(name)
        assert AlgorithmRepository.config[name]["server_cls"] is AlgorithmRepository.config["fed_avg"]["server_cls"]
        entry = AlgorithmRepository.config[name]["algorithm_cls"]
        assert isinstance(entry, functools.partial) and entry.func is ServerOptFedAVGAlgorithm
        assert entry.keywords == {"optimizer": mode}
        if mode == "avgm":
            assert entry(device=CPU).optimizer == "avgm"
        else:       # the caller binds the learning rate
            with pytest.raises(ValueError, match="no default"):
                entry(device=CPU)
            assert functools.partial(entry, learning_rate=0.01)(device=CPU).optimizer == mode


# ---- the class on the CPU device -----------------------------------------------------------------
@pytest.mark.parametrize("mode", SERVER_OPT_MODES)
def test_cpu_class_matches_restatement_over_three_rounds(mode):
    for code, out_dtype in (("f32", torch.float64), ("bf16", torch.float32), ("f64", torch.float64),
                            ("f16", torch.float64)):
        start, rounds = rounds_of(DTYPES[code])
        want = restated(start, rounds, mode, np.float32 if out_dtype == torch.float32 else np.float64)
        algo = ServerOptFedAVGAlgorithm(mode, **HYPER, device=CPU, out_dtype=out_dtype)
        run_rounds(algo, start, rounds, want, out_dtype)
        assert algo.last_step.worker_ids == [10, 11, 12, 13, 14] and algo.last_step.weights == [1.0, 2.0, 3.0, 4.0, 5.0]
        assert algo.last_step.total_weight == 15.0 and algo.last_step.mode == mode


def test_unweighted_skipped_workers_and_initial_second_moment():
    start, rounds = rounds_of(torch.float32, with_empty=False)
    rounds = [[c if i != 2 else None for i, c in enumerate(cl)] for cl in rounds]
    counted = [[c for c in cl if c is not None] for cl in rounds]
    names = list(start)
    want = ref.rounds([[list(c.values()) for c in cl] for cl in counted], [[1.0] * 4] * ROUNDS,
                      [start[k] for k in names], "adagrad", 0.05, 0.8, 0.99, 0.01, 0.25)
    algo = ServerOptFedAVGAlgorithm("adagrad", 0.05, beta1=0.8, tau=0.01, initial_second_moment=0.25, weighted=False,
                                    device=CPU)
    previous = start
    for r in range(ROUNDS):
        msg = feed(algo, rounds[r], previous)
        assert algo.skipped_workers == {12} and algo.last_step.worker_ids == [10, 11, 13, 14]
        assert algo.last_step.weights == [1.0] * 4 and algo.last_step.total_weight == 4.0
        for i, name in enumerate(names):
            assert bits(msg.parameter[name]) == bits(want[r][0][i])
        previous = msg.parameter


def test_avgm_with_beta_zero_and_rate_one_is_the_weighted_mean_about_the_previous_model():
    previous = {"a": f64(1.0, 2.0, 3.0)}
    clients = [{"a": f64(2.0, 2.0, 3.0)}, {"a": f64(1.5, 2.5, 3.0)}]
    algo = ServerOptFedAVGAlgorithm("avgm", beta1=0.0, device=CPU)
    msg = feed(algo, clients, previous)
    assert msg.parameter["a"].tolist() == [1.0 + (1.0 * 1.0 + 2.0 * 0.5) / 3.0, 2.0 + (2.0 * 0.5) / 3.0, 3.0]
    assert algo.state_dict()["m"]["a"].tolist() == [(1.0 + 1.0) / 3.0, 1.0 / 3.0, 0.0]


def test_state_is_untouched_after_a_failed_round():
    start, rounds = rounds_of(torch.float64, with_empty=False)
    for mode in SERVER_OPT_MODES:
        want = restated(start, rounds, mode)
        algo = ServerOptFedAVGAlgorithm(mode, **HYPER, device=CPU)
        # a failing first round allocates nothing
        bad = [dict(c) for c in rounds[0]]
        bad[1]["b"] = f64(1.0, NAN, 2.0)
        with pytest.raises(NaNAggregationError) as e:
            feed(algo, bad, start)
        assert e.value.stage == "input" and state_bits(algo) == (0, None, None)
        previous = run_rounds(algo, start, rounds[:1], want)
        before = state_bits(algo)
        with pytest.raises(NaNAggregationError) as e:                      # a NaN client
            feed(algo, bad, previous)
        assert e.value.stage == "input" and list(e.value.bad_clients) == [1] and state_bits(algo) == before
        with pytest.raises(NaNAggregationError) as e:                      # a NaN previous model
            feed(algo, rounds[1], {**previous, "s": f64(NAN).reshape(())})
        assert e.value.stage == "input" and state_bits(algo) == before
        shaped = [dict(c) for c in rounds[1]]
        shaped[3]["b"] = f64(1.0, 2.0)
        with pytest.raises(ValueError, match="tensor b: shape"):           # a shape mismatch between clients
            feed(algo, shaped, previous)
        assert state_bits(algo) == before
        other = [{"w": c["w"], "b": c["b"]} for c in rounds[1]]            # another layout than the state's
        with pytest.raises(ValueError, match="reset_state"):
            feed(algo, other, {"w": previous["w"], "b": previous["b"]})
        assert state_bits(algo) == before
        with pytest.raises(ValueError, match="set_old_parameter|lacks tensor"):
            feed(algo, rounds[1], {"w": previous["w"]})
        assert state_bits(algo) == before
        infinite = [dict(c) for c in rounds[1]]
        infinite[0]["b"] = f64(1.0, INF, 2.0)
        if mode != "avgm":                                                 # u = inf / inf: an error, not a drop
            with pytest.raises(NaNAggregationError) as e:
                feed(algo, infinite, previous)
            assert e.value.stage == "result" and state_bits(algo) == before
        # and the next good round continues as if nothing had happened
        feed(algo, rounds[1], previous)
        assert algo.rounds_done == 2
        names = list(start)
        sd = algo.state_dict()
        assert all(bits(sd["m"][k]) == bits(want[1][1][i]) for i, k in enumerate(names))


@pytest.mark.parametrize("mode", SERVER_OPT_MODES)
def test_checkpoint_continues_with_the_same_bits(mode):
    start, rounds = rounds_of(torch.float32)
    want = restated(start, rounds, mode)
    algo = ServerOptFedAVGAlgorithm(mode, **HYPER, device=CPU)
    previous = run_rounds(algo, start, rounds[:2], want)
    sd = algo.state_dict()
    assert sd["optimizer"] == mode and sd["rounds_done"] == 2 and sd["learning_rate"] == HYPER["learning_rate"]
    assert (sd["v"] is None) == (mode == "avgm") and all(t.dtype == torch.float64 for t in sd["m"].values())
    fresh = ServerOptFedAVGAlgorithm(mode, **HYPER, device=CPU)
    fresh.load_state_dict(sd)
    assert state_bits(fresh) == state_bits(algo)
    sd["m"]["b"].fill_(7.0)                                     # the checkpoint was copied in both directions
    assert state_bits(fresh) == state_bits(algo)
    msg = feed(fresh, rounds[2], previous)
    for i, name in enumerate(start):
        assert bits(msg.parameter[name]) == bits(want[2][0][i]) and bits(fresh.state_dict()["m"][name]) == bits(want[2][1][i])
    assert fresh.rounds_done == 3
    fresh.reset_state()
    assert state_bits(fresh) == (0, None, None)
    empty = ServerOptFedAVGAlgorithm(mode, **HYPER, device=CPU)
    empty.load_state_dict(empty.state_dict())                  # a checkpoint from before the first round
    assert state_bits(empty) == (0, None, None)


def test_load_state_dict_validates_on_the_host():
    start, rounds = rounds_of(torch.float64, with_empty=False)
    algo = ServerOptFedAVGAlgorithm("adam", **HYPER, device=CPU)
    feed(algo, rounds[0], start)
    good = algo.state_dict()
    before = state_bits(algo)

    def broken(**changes):
        sd = {k: ({n: t.clone() for n, t in v.items()} if isinstance(v, dict) else v) for k, v in good.items()}
        for k, v in changes.items():
            sd[k] = v
        return sd

    missing = broken()
    del missing["beta1"]
    nan_m = broken()
    nan_m["m"]["b"][1] = NAN
    inf_v = broken()
    inf_v["v"]["w"][0, 0] = INF
    neg_v = broken()
    neg_v["v"]["s"].fill_(-1e-30)
    shape_v = broken()
    shape_v["v"]["b"] = torch.zeros(4, dtype=torch.float64)
    names_v = broken()
    names_v["v"] = {("x" if k == "b" else k): t for k, t in names_v["v"].items()}
    for sd, match in ((missing, "keys"), (broken(extra=1), "keys"), (broken(optimizer="yogi"), "optimizer"),
                      (broken(rounds_done=-1), "rounds_done"), (broken(rounds_done=1.5), "rounds_done"),
                      (nan_m, "not finite"), (inf_v, "not finite"), (neg_v, "negative"), (shape_v, "shape"),
                      (names_v, "different tensors"), (broken(v=None), "second moments"),
                      (broken(m=None), "without first moments")):
        with pytest.raises(ValueError, match=match):
            algo.load_state_dict(sd)
        assert state_bits(algo) == before
    with pytest.raises(ValueError, match="second moments"):
        ServerOptFedAVGAlgorithm("avgm", device=CPU).load_state_dict(broken(optimizer="avgm"))


# ---- refusals ------------------------------------------------------------------------------------
def test_delta_quantised_and_foreign_messages():
    algo = ServerOptFedAVGAlgorithm("avgm", device=CPU)
    with pytest.raises(NotImplementedError, match="DeltaParameterMessage"):
        algo.process_worker_data(0, DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1.0))
    with pytest.raises(NotImplementedError, match="DeltaParameterMessage"):
        algo.process_worker_data(0, fm.DeltaParameterMessage(delta_parameter={"a": f64(1.0)}, aggregation_weight=1.0))
    record = QuantizedTensor.__new__(QuantizedTensor)
    with pytest.raises(NotImplementedError, match="dequantise"):
        algo.process_worker_data(0, ParameterMessage(parameter={"a": record}, aggregation_weight=1.0))
    with pytest.raises(TypeError, match="ParameterMessage"):
        algo.process_worker_data(0, fm.Message())
    msg = feed(ServerOptFedAVGAlgorithm("avgm", device=CPU), [{"a": f64(1.0)}, {"a": f64(2.0)}], {"a": f64(0.0)},
               msg_cls=fm.ParameterMessage)
    assert type(msg) is fm.ParameterMessage


def test_value_errors_of_the_round():
    clients = [{"a": f64(float(x) + 1.0, 0.5), "b": f64(2.0)} for x in range(4)]
    previous = {"a": f64(0.0, 0.0), "b": f64(0.0)}

    def run(cl, prev, **kw):
        return feed(ServerOptFedAVGAlgorithm("avgm", device=CPU, **kw), cl, prev)

    holed = [dict(c) for c in clients]
    del holed[3]["b"]
    with pytest.raises(ValueError, match="client 13 lacks tensor b"):
        run(holed, previous)
    with pytest.raises(ValueError, match="set_old_parameter"):
        run(clients, None)
    with pytest.raises(ValueError, match="lacks tensor b"):
        run(clients, {"a": f64(0.0, 0.0)})
    with pytest.raises(ValueError, match="tensor a"):
        run(clients, {"a": f64(0.0, 0.0, 0.0), "b": f64(0.0)})
    with pytest.raises(ValueError, match="tensor c"):
        run(clients, {**previous, "c": f64(1.0)})
    algo = ServerOptFedAVGAlgorithm("avgm", device=CPU)
    for wid, c in enumerate(clients):
        algo.process_worker_data(wid, ParameterMessage(parameter=c, aggregation_weight=0.0))
    algo.set_old_parameter(previous)
    with pytest.raises(ValueError, match="add up to 0"):
        algo.aggregate_worker_data()
    with pytest.raises(NotImplementedError, match="1024"):
        run([{"a": f64(1.0)}] * (_native.POINT_MAX_CLIENTS + 1), {"a": f64(0.0)})


def test_message_fields_follow_fedavg():
    algo = ServerOptFedAVGAlgorithm("adam", 0.1, device=CPU)
    algo.aggregate_loss = True
    for wid in range(4):
        algo.process_worker_data(wid, ParameterMessage(
            parameter={"a": f64(float(wid) + 1.0, 1.0)}, aggregation_weight=1 + wid, end_training=True, in_round=True,
            other_data={"training_loss": float(wid), "tag": "x"}))
    algo.set_old_parameter({"a": f64(0.0, 0.0)})
    msg = algo.aggregate_worker_data()
    assert isinstance(msg, ParameterMessage) and msg.end_training and msg.in_round
    assert msg.other_data["tag"] == "x"
    assert math.isclose(msg.other_data["training_loss"], sum((1 + w) * float(w) for w in range(4)) / 10)
