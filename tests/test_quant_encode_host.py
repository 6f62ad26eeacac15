"""The broadcast encoder without a GPU: the uniform stream's known answers, the package's CPU path
against the numpy restatement (tests/quant_encode_reference.py), the refusals, and a loopback round
through ``AggregationServer(broadcast_quantizer=...)`` with pipe workers."""

from __future__ import annotations

import multiprocessing as mp
import threading

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import BroadcastQuantizer, philox_uniforms
from distributed_learning_simulation_lib_amd.message import DeltaParameterMessage, ParameterMessage
from distributed_learning_simulation_lib_amd.quantized import (
    QuantizedTensor,
    codec_for,
    dequantize_parameter,
    dequantize_tensor,
    philox4x32,
)
from distributed_learning_simulation_lib_amd.server import AggregationServer, PipeServerEndpoint
from tests.helpers import OracleAlgorithm
from tests.quant_encode_cases import DRAW, LEVELS, SEED, WEIGHTS, check_records, torch_parameter
from tests.quant_encode_reference import expected_records, philox_scalar, uniforms

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, out):
    assert philox_scalar(ctr, key) == out  # the restatement
    assert tuple(int(w) for w in philox4x32(np.array(ctr, dtype=np.uint32), key)) == out  # the package


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_philox_uniforms_equal_the_restatement(dtype):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    for seed, draw, t, n in [(0, 0, 0, 1), (SEED, DRAW, 3, 1001), ((1 << 64) - 1, (1 << 32) - 1, 77, 10)]:
        u = philox_uniforms(seed, draw, t, n, dtype)
        assert u.dtype == dtype and u.shape == (n,)
        want = uniforms(seed, draw, t, n, npdt)
        assert np.array_equal(u.numpy(), want) and want.dtype == npdt
        assert (want >= 0).all() and (want < 1).all()
    # the first word of the all-zero known answer, by the definition
    first = philox_uniforms(0, 0, 0, 1, dtype).item()
    assert first == ((0x6627E8D5 >> 8) * 2.0**-24 if dtype == torch.float32
                     else ((0xE169C58D >> 5) * 2.0**26 + (0x6627E8D5 >> 6)) * 2.0**-53)
    with pytest.raises(TypeError):
        philox_uniforms(0, 0, 0, 4, torch.float16)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cpu_qsgd_records_are_the_restatements(dtype, level):
    p, tp = torch_parameter(dtype)
    check_records(BroadcastQuantizer("qsgd", level, seed=SEED)(tp, DRAW), p, "qsgd", level=level, what="cpu")


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cpu_nnadq_records_are_the_restatements(dtype, weight):
    p, tp = torch_parameter(dtype)
    got = BroadcastQuantizer("nnadq", weight=weight)(tp, DRAW)
    check_records(got, p, "nnadq", weight=weight, what="cpu")
    # the contract's header rule where numpy's min is free: -0.0 < +0.0
    lo = got["mixed_zero_minimum"].record[0:8].view(torch.float64)[0]
    assert lo == 0 and bool(torch.signbit(lo))


def test_mixed_dtypes_keep_dict_positions():
    rng = np.random.default_rng(8)
    p = {"a": rng.standard_normal(50).astype(np.float32), "b": rng.standard_normal(70),
         "c": rng.standard_normal((3, 5)).astype(np.float32)}
    tp = {k: torch.from_numpy(v) for k, v in p.items()}
    for scheme in ("qsgd", "nnadq"):
        check_records(BroadcastQuantizer(scheme, seed=SEED)(tp, DRAW), p, scheme)


def test_draw_tensor_index_and_seed_change_qsgd_only():
    x = torch.from_numpy(np.random.default_rng(1).standard_normal(4000).astype(np.float32))
    base = BroadcastQuantizer("qsgd", seed=1)({"w": x}, 0)["w"]
    assert torch.equal(base.record, BroadcastQuantizer("qsgd", seed=1)({"w": x}, 0)["w"].record)
    others = [BroadcastQuantizer("qsgd", seed=1)({"w": x}, 1)["w"],
              BroadcastQuantizer("qsgd", seed=2)({"w": x}, 0)["w"],
              BroadcastQuantizer("qsgd", seed=1)({"pad": x[:3], "w": x}, 0)["w"]]
    for o in others:
        assert not torch.equal(o.slots, base.slots)
        assert torch.equal(o.sign_bits, base.sign_bits) and o.norm == base.norm
    nbase = BroadcastQuantizer("nnadq", seed=1)({"w": x}, 0)["w"].record
    assert torch.equal(nbase, BroadcastQuantizer("nnadq", seed=2)({"w": x}, 9)["w"].record)
    assert torch.equal(nbase, BroadcastQuantizer("nnadq", seed=1)({"pad": x[:3], "w": x}, 0)["w"].record)


def test_refusals():
    x = torch.ones(10)
    for bad in (float("nan"), float("inf"), float("-inf")):
        y = x.clone()
        y[7] = bad
        for scheme in ("qsgd", "nnadq"):
            with pytest.raises(AssertionError):
                BroadcastQuantizer(scheme)({"ok": x, "w": y}, 0)
    with pytest.raises(NotImplementedError):
        BroadcastQuantizer("qsgd", use_l2_norm=True)
    for level in (0, 256, -1, 2.5):
        with pytest.raises(ValueError):
            BroadcastQuantizer("qsgd", quantization_level=level)
    for weight in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            BroadcastQuantizer("nnadq", weight=weight)
    with pytest.raises(ValueError):
        BroadcastQuantizer("topk")
    for dtype in (torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(TypeError):
            BroadcastQuantizer("qsgd")({"w": torch.zeros(4, dtype=dtype)}, 0)
    with pytest.raises(ValueError):
        BroadcastQuantizer("qsgd")({"w": x}, 1 << 32)


def test_default_server_broadcasts_the_dense_copy():
    class Capture:
        worker_num = 1

        def __init__(self):
            self.sent = []

        def broadcast(self, data, worker_ids=None):
            self.sent.append(data)

    cap = Capture()
    srv = AggregationServer(algorithm=OracleAlgorithm(), worker_number=1, endpoint=cap)
    srv._process_worker_data(0, ParameterMessage(parameter={"w": torch.ones(4)}, aggregation_weight=1.0))
    assert cap.sent[0] is srv.results[0] and "quantized" not in cap.sent[0].other_data
    assert cap.sent[0].parameter["w"].dtype == torch.float64


WORKERS = 3
SHAPES = {"w": (1500,), "b": (33,), "m": (4, 6)}


def _full(wid: int) -> dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(100 + wid)
    return {k: torch.randn(s, generator=g, dtype=torch.float64) for k, s in SHAPES.items()}


def _delta(wid: int) -> dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(200 + wid)
    return {k: torch.randn(s, generator=g, dtype=torch.float64) * 1e-3 for k, s in SHAPES.items()}


def _pipe_worker(conn, wid: int, received: list) -> None:
    received.append(conn.recv())  # the initial model
    conn.send(ParameterMessage(parameter=_full(wid), aggregation_weight=1.0 + wid))
    received.append(conn.recv())
    conn.send(DeltaParameterMessage(delta_parameter=_delta(wid), aggregation_weight=2.0 + wid))
    received.append(conn.recv())
    conn.close()


@pytest.mark.parametrize("scheme", ["qsgd", "nnadq"])
def test_loopback_round_with_a_broadcast_quantizer(scheme):
    pipes = [mp.Pipe() for _ in range(WORKERS)]
    received: list[list] = [[] for _ in range(WORKERS)]
    threads = [threading.Thread(target=_pipe_worker, args=(pipes[i][1], i, received[i])) for i in range(WORKERS)]
    for t in threads:
        t.start()
    init = {k: torch.zeros(s, dtype=torch.float32) + 0.25 for k, s in SHAPES.items()}
    srv = AggregationServer(algorithm=OracleAlgorithm(), worker_number=WORKERS,
                            endpoint=PipeServerEndpoint([p[0] for p in pipes]), round_number=2, init_parameter=init,
                            broadcast_quantizer=BroadcastQuantizer(scheme, seed=SEED))
    srv.start()
    for t in threads:
        t.join(timeout=60)
        assert not t.is_alive()

    # self.results is dense and full precision: the initial model, then the two rounds
    assert len(srv.results) == 3
    for res in srv.results:
        assert all(isinstance(v, torch.Tensor) and v.dtype == torch.float64 for v in res.parameter.values())
        assert "quantized" not in res.other_data
    # round 2's deltas were restored against the full-precision cached model, not a dequantised one
    order = srv.arrivals[2]
    acc = {k: sum((srv.results[1].parameter[k] + _delta(w)[k]) * (2.0 + w) for w in order) for k in SHAPES}
    total = sum(2.0 + w for w in order)
    for k in SHAPES:
        assert torch.allclose(srv.results[2].parameter[k], acc[k] / total, rtol=1e-12, atol=0)
    assert all(torch.equal(srv.current_aggregated_model.parameter[k], srv.results[2].parameter[k]) for k in SHAPES)

    # what every worker received: records with the flag, draw = the broadcast count
    for wid in range(WORKERS):
        assert len(received[wid]) == 3
        for draw, (msg, dense) in enumerate(zip(received[wid], srv.results)):
            assert msg.other_data["quantized"] is True
            assert msg.is_initial == (draw == 0)
            assert all(isinstance(v, QuantizedTensor) for v in msg.parameter.values())
            # the initial model is fp32 (encoded as it was given), the aggregates fp64
            src = init if draw == 0 else dense.parameter
            want = expected_records({k: v.numpy() for k, v in src.items()}, scheme, seed=SEED, draw=draw)
            got = dequantize_parameter(msg.parameter)
            for k, v in src.items():
                rec = QuantizedTensor(torch.from_numpy(want[k]), tuple(v.shape), codec_for(v.dtype, scheme))
                ref = dequantize_tensor(rec)
                assert got[k].dtype == ref.dtype == v.dtype and got[k].shape == v.shape
                assert np.array_equal(got[k].numpy().view(np.uint8), ref.numpy().view(np.uint8)), (wid, draw, k)
