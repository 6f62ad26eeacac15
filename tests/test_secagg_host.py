"""Secure aggregation on the host (SecAggFedAVGAlgorithm on a CPU device) through the
server, bit for bit against the restatement in tests/secagg_reference.py."""

import itertools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (DeltaParameterMessage, ParameterMessage,
                                                     SecAggEndpoint, SecAggFedAVGAlgorithm, SecAggSession,
                                                     SignFedAVGAlgorithm, secagg_mask_parameter)
from distributed_learning_simulation_lib_amd.server import AggregationServer
from tests import secagg_reference as ref

SEED, F, VB = 0x1234_5678_9ABC_DEF1, 24, 40
WEIGHTS = [3, 0, 5, 1, 2]  # a zero-weight client


def test_masks_cancel_for_every_subset():
    xs = [[0.5 * i - 1.0, -0.0, 2.0 ** -F * 1.5] for i in range(5)]
    ys = [ref.masked(x, w, ref.client_table(SEED, 5, i, 9), 9, 2, F, VB)[0] for i, (x, w) in enumerate(zip(xs, WEIGHTS))]
    for k in range(1, 6):
        for A in itertools.combinations(range(5), k):
            D = [i for i in range(5) if i not in A]
            S = sum(ys[i] for i in A) + ref.table_sum(ref.server_table(SEED, A, D, 9), 9, 2, 3)
            assert np.array_equal(S, sum(ref.encode(xs[i], WEIGHTS[i], F, VB)[0] for i in A)), A


class Recorder:
    def __init__(self):
        self.sent = []

    def send(self, data):
        self.sent.append(data)


def init_model():
    return {"w": torch.linspace(-1.0, 1.0, 15, dtype=torch.float64).reshape(3, 5), "b": torch.tensor([0.1], dtype=torch.float64),
            "none": torch.zeros(0, 3, dtype=torch.float64)}


def secagg_rounds(device, present, out_dtype=torch.float64, dtype=torch.float32, client_device="cpu",
                  algorithm_cls=SecAggFedAVGAlgorithm, endpoint_cls=SecAggEndpoint):
    """Rounds through endpoints and server, each checked against the restatement; present[r] lists
    the workers that report in round r. Returns the results."""
    n, init = len(WEIGHTS), init_model()
    server = AggregationServer(algorithm_cls(SEED, device=device, out_dtype=out_dtype, value_bits=VB),
                               worker_number=n, round_number=len(present), init_parameter=init)
    server._send_result(ParameterMessage(parameter=init, in_round=True, is_initial=True))
    ends = [endpoint_cls(Recorder(), session_seed=SEED, worker_id=i, worker_number=n, frac_bits=F, value_bits=VB)
            for i in range(n)]
    gen, base = torch.Generator().manual_seed(3), init
    for rnd, A in enumerate(present):
        deltas = [{k: torch.randn(v.shape, generator=gen).to(dtype).to(client_device) for k, v in init.items()}
                  for _ in range(n)]
        for i in range(n):  # every client masks every round (the endpoints count them); a dropout's message is lost
            ends[i].send(DeltaParameterMessage(delta_parameter=deltas[i], aggregation_weight=WEIGHTS[i]))
            server._process_worker_data(i, ends[i]._endpoint.sent[-1] if i in A else None)
        got = server.results[-1].parameter
        D, W = [i for i in range(n) if i not in A], sum(WEIGHTS[i] for i in A)
        for t, name in enumerate(("w", "b")):
            ys = [ref.masked(deltas[i][name].double().reshape(-1).cpu().numpy(), WEIGHTS[i],
                             ref.client_table(SEED, n, i, rnd), rnd, t, F, VB)[0] for i in A]
            sent = [ends[i]._endpoint.sent[-1].delta_parameter[name].words.cpu().numpy() for i in A]
            assert all(np.array_equal(s.view(np.uint64), y) for s, y in zip(sent, ys)), (rnd, name)
            want = ref.unmasked(ys, ref.server_table(SEED, A, D, rnd), rnd, t, F, W,
                                base[name].double().reshape(-1).numpy(), out_dtype == torch.float32)
            want = torch.from_numpy(want.astype(np.float64))  # the server's cache widens a float32 result, exactly
            assert torch.equal(got[name].reshape(-1).cpu().view(torch.int64), want.view(torch.int64)), (rnd, name)
        base = got
    return server.results


def test_cpu_rounds_match_the_restatement():
    # all report (worker 1 has weight 0); workers 1 and 4 skipped, under the next round's masks; three skipped
    secagg_rounds(torch.device("cpu"), [[0, 1, 2, 3, 4], [0, 2, 3], [2, 0]])


def masked_message(weight=1, frac_bits=F, plain=()):
    d = secagg_mask_parameter({"w": torch.ones(3, 5), "b": torch.ones(1), "none": torch.zeros(0, 3)}, 1,
                              SecAggSession(SEED, 2), 0, 0, frac_bits, VB)
    d.update({k: torch.ones(1) for k in plain})
    return DeltaParameterMessage(delta_parameter=d, aggregation_weight=weight)


@pytest.mark.parametrize("case", ["fractional", "wraps", "mixed", "plain", "parameter", "frac_bits", "other"])
def test_refusals(case):
    alg = SecAggFedAVGAlgorithm(SEED, device=torch.device("cpu"), value_bits=VB)
    alg.set_old_parameter(init_model())
    if case == "fractional":
        with pytest.raises(ValueError, match="integer"):
            secagg_mask_parameter({"w": torch.ones(2)}, 1.5, SecAggSession(SEED, 2), 0, 0)
    elif case == "wraps":  # 40 + bit_length(2^22 + 2^22) = 64 > 63; each weight alone fits (63)
        alg.process_worker_data(0, masked_message(1 << 22))
        alg.process_worker_data(1, masked_message(1 << 22))
        with pytest.raises(ValueError, match="wrap"):
            alg.aggregate_worker_data()
    elif case in ("mixed", "plain"):
        msg = masked_message(plain=("b",)) if case == "mixed" else DeltaParameterMessage(
            delta_parameter={"w": torch.ones(3, 5)}, aggregation_weight=1)
        with pytest.raises(ValueError, match="plain"):
            alg.process_worker_data(0, msg)
    elif case == "parameter":
        with pytest.raises(NotImplementedError, match="ParameterMessage"):
            alg.process_worker_data(0, ParameterMessage(parameter=init_model(), aggregation_weight=1))
    elif case == "frac_bits":
        alg.process_worker_data(0, masked_message())
        alg.process_worker_data(1, masked_message(frac_bits=F + 1))
        with pytest.raises(ValueError, match="frac_bits"):
            alg.aggregate_worker_data()
    else:  # another algorithm cannot densify a masked delta
        server = AggregationServer(SignFedAVGAlgorithm(device=torch.device("cpu")), worker_number=2, round_number=1,
                                   init_parameter=init_model())
        server._send_result(ParameterMessage(parameter=init_model(), in_round=True, is_initial=True))
        with pytest.raises(TypeError, match="masked"):
            server._process_worker_data(0, masked_message())
