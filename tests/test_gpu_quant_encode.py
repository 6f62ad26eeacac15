"""The broadcast encoder on the GPU (fedavg_quant_encode): records byte-identical to
the numpy restatement (tests/quant_encode_reference.py: the oracles' own quantisers fed with the
contract's Philox stream) and to the package's CPU path, for both codecs and both dtypes, written
into memory pre-filled with 0xA5."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import BroadcastQuantizer, FedAVGAlgorithm, ParameterMessage, _native
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout, NaNAggregationError
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor, codec_for, dequantize_parameter
from distributed_learning_simulation_lib_amd.server import AggregationServer
from tests.quant_encode_cases import DRAW, LEVELS, SEED, WEIGHTS, check_records, tile, torch_parameter
from tests.quant_encode_reference import expected_records

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _prefilled(q: BroadcastQuantizer, tp, device) -> None:
    """Run once so the quantizer owns its blob, then poison every byte of it."""
    q(tp, 0)
    q.device_blob(device).fill_(0xA5)
    torch.cuda.synchronize(device)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_qsgd_records_match_restatement_and_cpu_path(hip_device, dtype, level):
    p, tp = torch_parameter(dtype, hip_device)
    q = BroadcastQuantizer("qsgd", level, seed=SEED)
    _prefilled(q, tp, hip_device)
    got = q(tp, DRAW)
    assert all(r.record.device == hip_device for r in got.values())
    check_records(got, p, "qsgd", level=level, what="gpu")
    cpu = q({k: v.cpu() for k, v in tp.items()}, DRAW)
    for k in p:
        assert torch.equal(got[k].record.cpu(), cpu[k].record), k


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nnadq_records_match_restatement_and_cpu_path(hip_device, dtype, weight):
    p, tp = torch_parameter(dtype, hip_device)
    q = BroadcastQuantizer("nnadq", weight=weight)
    _prefilled(q, tp, hip_device)
    got = q(tp, DRAW)
    check_records(got, p, "nnadq", weight=weight, what="gpu")
    cpu = q({k: v.cpu() for k, v in tp.items()}, DRAW)
    for k in p:  # the package's two paths agree on every byte, the zero-extremum header included
        assert torch.equal(got[k].record.cpu(), cpu[k].record), k


@pytest.mark.parametrize("scheme", ["qsgd", "nnadq"])
def test_c_entry_writes_every_byte_of_caller_memory(hip_device, scheme):
    """The C entry point on records the caller allocated and poisoned, one tensor per call and the
    tensors' own stream ids: nothing of 0xA5 survives and nothing outside a record is written."""
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    p, tp = torch_parameter(np.float32, hip_device)
    want = expected_records(p, scheme, 255, 0.01, SEED, DRAW)
    codec = codec_for(torch.float32, scheme)
    names = list(p)
    pick = [names.index(k) for k in ("n1", "n17", f"n{tile() + 1}", "offset_large", "zeros")]
    guard = 64
    bufs = [torch.full((codec.record_bytes(p[names[i]].size) + 2 * guard,), 0xA5, dtype=torch.uint8, device=hip_device)
            for i in pick]
    recs = [b[guard:-guard] for b in bufs]
    ctx.quant_encode(codec.code, [tp[names[i]] for i in pick], recs, 255, 0.01, SEED, DRAW, pick)
    ctx.raise_on_nan()
    for i, b, r in zip(pick, bufs, recs):
        assert np.array_equal(r.cpu().numpy(), want[names[i]]), names[i]
        assert bool((b[:guard] == 0xA5).all()) and bool((b[-guard:] == 0xA5).all()), names[i]
    ctx.close()


def test_c_entry_refusals(hip_device):
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    x = torch.zeros(20, device=hip_device)
    rec = torch.empty(codec_for(torch.float32).record_bytes(20), dtype=torch.uint8, device=hip_device)
    for level in (0, 256):
        with pytest.raises(_native.NativeError) as e:
            ctx.quant_encode(_native.QSGD_F32, [x], [rec], level)
        assert e.value.status == _native.ERR_INVALID
    nrec = torch.empty(codec_for(torch.float32, "nnadq").record_bytes(20), dtype=torch.uint8, device=hip_device)
    for weight in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_native.NativeError) as e:
            ctx.quant_encode(_native.NNADQ_F32, [x], [nrec], weight=weight)
        assert e.value.status == _native.ERR_INVALID
    lib = ctx._lib
    ptr = np.array([x.data_ptr()], dtype=np.uint64)
    n = np.array([20], dtype=np.int64)
    bad_rec = np.array([rec.data_ptr() + 8], dtype=np.uint64)  # not 16-byte aligned
    assert lib.fedavg_quant_encode(ctx._h, _native.QSGD_F32, ptr.ctypes.data, n.ctypes.data, None, 1,
                                   bad_rec.ctypes.data, 255, 0.01, 0, 0, ctx.stream) == _native.ERR_INVALID
    good = np.array([rec.data_ptr()], dtype=np.uint64)
    assert lib.fedavg_quant_encode(ctx._h, _native.F32, ptr.ctypes.data, n.ctypes.data, None, 1, good.ctypes.data,
                                   255, 0.01, 0, 0, ctx.stream) == _native.ERR_INVALID
    assert lib.fedavg_quant_encode(ctx._h, _native.QSGD_F32, ptr.ctypes.data, n.ctypes.data, None, 0,
                                   good.ctypes.data, 255, 0.01, 0, 0, ctx.stream) == _native.ERR_INVALID
    assert ctx.flags() == 0
    ctx.close()


@pytest.mark.parametrize("scheme", ["qsgd", "nnadq"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_element_is_refused(hip_device, scheme, bad):
    q = BroadcastQuantizer(scheme)
    x = torch.randn(tile() + 9, dtype=torch.float64, device=hip_device)
    assert q({"w": x}, 0)["w"].numel == x.numel()
    x[-1] = bad  # the very last element of a tail tile
    with pytest.raises(AssertionError) as e:
        q({"a": torch.ones(3, dtype=torch.float64, device=hip_device), "w": x}, 1)
    assert isinstance(e.value, NaNAggregationError) and e.value.stage == "input"
    x[-1] = 1.0  # the context is usable again
    got = q({"w": x}, 2)
    want = expected_records({"w": x.cpu().numpy()}, scheme, draw=2)
    assert np.array_equal(got["w"].record.cpu().numpy(), want["w"])


def test_same_seed_and_draw_give_the_same_bytes_and_others_do_not(hip_device):
    x = {"w": torch.randn(3 * tile() + 1, device=hip_device), "b": torch.randn(65, device=hip_device)}
    q = BroadcastQuantizer("qsgd", seed=11)
    a = {k: v.record.clone() for k, v in q(x, 4).items()}
    b = {k: v.record.clone() for k, v in q(x, 4).items()}
    c = {k: v.record.clone() for k, v in q(x, 5).items()}
    d = {k: v.record.clone() for k, v in BroadcastQuantizer("qsgd", seed=12)(x, 4).items()}
    for k in x:
        assert torch.equal(a[k], b[k])
        assert not torch.equal(a[k], c[k]) and not torch.equal(a[k], d[k])
    # the tensor's position enters the stream: the same values at another position encode differently
    y = {"pad": x["b"], "w": x["w"]}
    assert not torch.equal(q(y, 4)["w"].record, a["w"])


@pytest.mark.parametrize("scheme", ["qsgd", "nnadq"])
def test_blob_reuse_after_a_larger_layout(hip_device, scheme):
    rng = np.random.default_rng(3)
    big = {f"t{i}": rng.standard_normal(n).astype(np.float32) for i, n in enumerate([2 * tile() + 5, 129, 4000])}
    small = {"a": rng.standard_normal(17), "b": rng.standard_normal(tile() + 1).astype(np.float32), "c": np.zeros(5)}
    q = BroadcastQuantizer(scheme, seed=SEED)
    dev = lambda p: {k: torch.from_numpy(v).to(hip_device) for k, v in p.items()}  # noqa: E731
    check_records(q(dev(big), 1), big, scheme, draw=1, what="big")
    blob = q.device_blob(hip_device)
    check_records(q(dev(small), 2), small, scheme, draw=2, what="small after big (mixed dtypes)")
    assert q.device_blob(hip_device) is blob  # reused, not reallocated
    check_records(q(dev(big), 3), big, scheme, draw=3, what="big again")
    host = q.encode_to_host(dev(small), 4)
    assert all(r.record.device.type == "cpu" for r in host.values())
    check_records(host, small, scheme, draw=4, what="host records")


def test_unsupported_dtype_and_empty_tensor(hip_device):
    q = BroadcastQuantizer("qsgd")
    with pytest.raises(TypeError):
        q({"h": torch.zeros(4, dtype=torch.float16, device=hip_device)}, 0)
    p = {"e": np.zeros((0, 3), dtype=np.float32), "w": np.arange(5, dtype=np.float32)}
    for scheme in ("qsgd", "nnadq"):
        got = BroadcastQuantizer(scheme)({k: torch.from_numpy(v).to(hip_device) for k, v in p.items()}, 0)
        check_records(got, p, scheme, seed=0, draw=0)


@pytest.mark.parametrize("scheme", ["qsgd", "nnadq"])
def test_plugin_round_broadcasts_the_encoded_result(hip_device, scheme):
    """FedAVGAlgorithm on the GPU, then the server with a quantizer: what goes out is the
    restatement applied to the aggregated result; a refused model leaves the cache intact."""

    class Capture:
        worker_num = 3

        def __init__(self):
            self.sent = []

        def broadcast(self, data, worker_ids=None):
            self.sent.append(data)

    cap = Capture()
    srv = AggregationServer(algorithm=FedAVGAlgorithm(device=hip_device), worker_number=3, endpoint=cap,
                            round_number=3, broadcast_quantizer=BroadcastQuantizer(scheme, seed=5))
    g = torch.Generator().manual_seed(1)
    shapes = {"w": (tile() + 3,), "b": (33,), "m": (7, 9)}

    def one_round(poison=False):
        for wid in range(3):
            param = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
            if poison and wid == 1:
                param["b"][5] = float("inf")
            srv._process_worker_data(wid, ParameterMessage(parameter=param, aggregation_weight=1.0 + wid))

    one_round()
    one_round()
    assert len(cap.sent) == 2 and len(srv.results) == 2
    for draw, (msg, dense) in enumerate(zip(cap.sent, srv.results)):
        assert msg.other_data["quantized"] is True and "quantized" not in dense.other_data
        assert all(isinstance(v, QuantizedTensor) and v.record.device.type == "cpu" for v in msg.parameter.values())
        agg = {k: v.numpy() for k, v in dense.parameter.items()}
        assert all(v.dtype == np.float64 for v in agg.values())
        check_records(msg.parameter, agg, scheme, seed=5, draw=draw, what=f"round {draw}")
        deq = dequantize_parameter(msg.parameter)
        assert all(deq[k].shape == dense.parameter[k].shape for k in deq)
    cached = {k: v.clone() for k, v in srv.current_aggregated_model.parameter.items()}
    with pytest.raises(AssertionError):
        one_round(poison=True)  # inf in one client: the aggregate holds a non-finite element
    assert len(cap.sent) == 2
    for k, v in cached.items():
        assert torch.equal(srv.current_aggregated_model.parameter[k], v)
