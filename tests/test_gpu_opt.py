"""``ServerOptFedAVGAlgorithm`` on the GPU: three consecutive rounds per optimiser,
outputs and state bit for bit against the class on the CPU and against the numpy restatement
(tests/opt_reference.py), on a small multi-tensor layout with an empty and a 0-d tensor; that a failed
round leaves the state and the context as they were; the checkpoint; and one round per registered
name through ``AggregationServer``. The helpers are those of tests/test_opt_host.py."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    NaNAggregationError,
    ParameterMessage,
    ServerOptFedAVGAlgorithm,
)
from distributed_learning_simulation_lib_amd.fedavg import SERVER_OPT_MODES
from distributed_learning_simulation_lib_amd.server import AggregationServer
from tests.test_opt_host import CPU, DTYPES, HYPER, INF, NAN, bits, f64, feed, restated, rounds_of, run_rounds, state_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", SERVER_OPT_MODES)
def test_three_rounds_equal_the_restatement_and_the_cpu_class(hip_device, mode):
    for code, out_dtype in (("f32", torch.float64), ("bf16", torch.float32)):
        start, rounds = rounds_of(DTYPES[code])
        want = restated(start, rounds, mode, np.float32 if out_dtype == torch.float32 else np.float64)
        gpu = ServerOptFedAVGAlgorithm(mode, **HYPER, device=hip_device, out_dtype=out_dtype)
        cpu = ServerOptFedAVGAlgorithm(mode, **HYPER, device=CPU, out_dtype=out_dtype)
        last = run_rounds(gpu, start, rounds, want, out_dtype)
        assert all(t.device == hip_device for t in last.values()) and last["e"].shape == (0, 4) and last["s"].shape == ()
        run_rounds(cpu, start, rounds, want, out_dtype)
        assert state_bits(gpu) == state_bits(cpu)
        assert gpu.last_step == cpu.last_step and gpu.last_step.mode == mode
        # updates that already live on the device, and a previous model there too
        again = ServerOptFedAVGAlgorithm(mode, **HYPER, device=hip_device, out_dtype=out_dtype)
        on_device = [[{k: t.to(hip_device) for k, t in c.items()} for c in cl] for cl in rounds]
        run_rounds(again, {k: t.to(hip_device) for k, t in start.items()}, on_device, want, out_dtype)


def test_a_failed_round_leaves_the_state_and_the_context_usable(hip_device):
    start, rounds = rounds_of(torch.float32, with_empty=False)
    for mode in ("avgm", "yogi"):
        want = restated(start, rounds, mode)
        algo = ServerOptFedAVGAlgorithm(mode, **HYPER, device=hip_device)
        bad = [dict(c) for c in rounds[0]]
        bad[1]["b"] = torch.tensor([1.0, NAN, 2.0])
        with pytest.raises(NaNAggregationError) as e:                      # a failing first round allocates nothing
            feed(algo, bad, start)
        assert e.value.stage == "input" and list(e.value.bad_clients) == [1] and state_bits(algo) == (0, None, None)
        previous = run_rounds(algo, start, rounds[:1], want)
        before = state_bits(algo)
        with pytest.raises(NaNAggregationError) as e:
            feed(algo, bad, previous)
        assert e.value.stage == "input" and state_bits(algo) == before
        with pytest.raises(NaNAggregationError) as e:                      # a NaN previous model
            feed(algo, rounds[1], {**previous, "s": f64(NAN).reshape(())})
        assert e.value.stage == "input" and state_bits(algo) == before
        shaped = [dict(c) for c in rounds[1]]
        shaped[3]["b"] = torch.tensor([1.0, 2.0])
        with pytest.raises(ValueError, match="tensor b: shape"):
            feed(algo, shaped, previous)
        other = [{"w": c["w"], "b": c["b"]} for c in rounds[1]]
        with pytest.raises(ValueError, match="reset_state"):
            feed(algo, other, {"w": previous["w"], "b": previous["b"]})
        assert state_bits(algo) == before
        if mode != "avgm":                                                 # u = inf / inf: an error, not a drop
            infinite = [dict(c) for c in rounds[1]]
            infinite[0]["b"] = torch.tensor([1.0, INF, 2.0])
            with pytest.raises(NaNAggregationError) as e:
                feed(algo, infinite, previous)
            assert e.value.stage == "result" and state_bits(algo) == before
        run_rounds(algo, previous, rounds, want, first=1)                  # the next good rounds: the same bits


@pytest.mark.parametrize("mode", ["avgm", "adam"])
def test_checkpoint_moves_between_devices(hip_device, mode):
    start, rounds = rounds_of(torch.float32)
    want = restated(start, rounds, mode)
    algo = ServerOptFedAVGAlgorithm(mode, **HYPER, device=hip_device)
    previous = run_rounds(algo, start, rounds[:2], want)
    sd = algo.state_dict()
    assert all(t.device.type == "cpu" and t.dtype == torch.float64 for t in sd["m"].values())
    for device in (hip_device, CPU):
        fresh = ServerOptFedAVGAlgorithm(mode, **HYPER, device=device)
        fresh.load_state_dict(sd)
        assert state_bits(fresh) == state_bits(algo)
        run_rounds(fresh, previous, rounds, want, first=2)
        assert fresh.rounds_done == 3


def test_one_round_per_registered_name_through_the_server(hip_device):
    start, rounds = rounds_of(torch.float32)
    for name, mode in (("fed_avgm", "avgm"), ("fed_adagrad", "adagrad"), ("fed_yogi", "yogi"), ("fed_adam", "adam")):
        entry = AlgorithmRepository.config[name]["algorithm_cls"]
        assert AlgorithmRepository.config[name]["server_cls"] is AggregationServer
        hyper = dict(HYPER) if mode != "avgm" else {"learning_rate": 1.0, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
        algo = functools.partial(entry, learning_rate=hyper["learning_rate"])(device=hip_device)
        srv = AggregationServer(algorithm=algo, worker_number=len(rounds[0]), round_number=1)
        srv.current_aggregated_model.cache_parameter({k: t.clone() for k, t in start.items()})
        for wid, c in enumerate(rounds[0]):
            srv._process_worker_data(wid, ParameterMessage(parameter=dict(c), aggregation_weight=wid + 1))
        assert len(srv.results) == 1 and algo.rounds_done == 1 and algo.last_step.mode == mode
        want = restated(start, rounds[:1], mode, **hyper)
        for i, k in enumerate(start):
            assert bits(srv.results[0].parameter[k]) == bits(want[0][0][i]), (name, k)
