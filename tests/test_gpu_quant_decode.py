"""The record decoder on the GPU (fedavg_quant_decode): bits identical to the oracles'
``dequantize`` for both codecs and both dtypes, written into guarded memory pre-filled with 0xA5,
through 16-byte aligned outputs and outputs one element off; the fp64 copy; host records through one
upload; the flag; the C entry's refusals; the server's ``_dequantize_if_needed`` consumer."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    BroadcastDequantizer,
    BroadcastQuantizer,
    FedAVGAlgorithm,
    NNADQClientEndpoint,
    ParameterMessage,
    RobustFedAVGAlgorithm,
    StochasticQuantClientEndpoint,
    _native,
)
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout, NaNAggregationError, OutputTable
from distributed_learning_simulation_lib_amd.quantized import codec_for, dequantize_parameter, dequantize_tensor
from distributed_learning_simulation_lib_amd.server import AggregationServer
from tests.quant_decode_cases import (
    DTYPES,
    SCHEMES,
    as_quantized,
    assert_guards_intact,
    assert_same_bits,
    bad_header_record,
    encoded_records,
    guarded,
    handmade_records,
    overflow_record,
    quantized_dict,
    torch_dtype,
)
from tests.quant_encode_cases import tile

pytestmark = pytest.mark.gpu


def _all_cases(dtype, scheme):
    return {**encoded_records(dtype, scheme), **handmade_records(dtype, scheme)}


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "one_element_off"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_decoded_bits_equal_the_oracle(hip_device, dtype, scheme, offset):
    cases = _all_cases(dtype, scheme)
    records = quantized_dict(cases, dtype, scheme, hip_device)
    kept = {k: q.record.clone() for k, q in records.items()}
    bufs = {k: guarded(shape, torch_dtype(dtype), hip_device, offset) for k, (_, shape) in cases.items()}
    deq = BroadcastDequantizer()
    got = deq(records, out={k: view for k, (_, view) in bufs.items()})
    assert list(got) == list(cases)
    for k, (rec, shape) in cases.items():
        buf, view = bufs[k]
        assert got[k] is view
        assert_same_bits(view, rec, shape, dtype, scheme, f"{scheme} {np.dtype(dtype)} {k}")
        assert_guards_intact(buf, view, k)
        assert torch.equal(records[k].record, kept[k]), k  # the records are only read
    if not offset:  # and into tensors the dequantizer allocates
        fresh = deq(records)
        for k, (rec, shape) in cases.items():
            assert fresh[k].device == hip_device
            assert_same_bits(fresh[k], rec, shape, dtype, scheme, f"fresh {k}")


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "one_element_off"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_fp64_copy_is_the_exact_widening(hip_device, scheme, offset):
    cases = _all_cases(np.float32, scheme)
    records = quantized_dict(cases, np.float32, scheme, hip_device)
    outs = {k: guarded(shape, torch.float32, hip_device, offset) for k, (_, shape) in cases.items()}
    wides = {k: guarded(shape, torch.float64, hip_device, offset) for k, (_, shape) in cases.items()}
    got = BroadcastDequantizer()(records, out={k: v for k, (_, v) in outs.items()},
                                 f64_out={k: v for k, (_, v) in wides.items()})
    for k, (rec, shape) in cases.items():
        assert_same_bits(got[k], rec, shape, np.float32, scheme, k)
        assert torch.equal(wides[k][1], got[k].to(torch.float64)), k
        assert_guards_intact(*outs[k], k)
        assert_guards_intact(*wides[k], k)
    # an fp64 codec has no wider copy: refused by the wrapper and by the C entry (see the refusals)
    rec, shape = next(iter(handmade_records(np.float64, scheme).values()))
    q = as_quantized(rec, shape, np.float64, scheme, hip_device)
    o = torch.empty(shape, dtype=torch.float64, device=hip_device)
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    with pytest.raises(ValueError):
        ctx.quant_decode(q.codec.code, [q.record], [o.reshape(-1)], [torch.empty_like(o).reshape(-1)])
    with pytest.raises(ValueError):
        BroadcastDequantizer()({"w": q}, f64_out={"w": torch.empty_like(o)})
    ctx.close()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_records_with_a_device_and_the_plain_functions(hip_device, dtype, scheme):
    cases = _all_cases(dtype, scheme)
    host = quantized_dict(cases, dtype, scheme)
    deq = BroadcastDequantizer()
    up = deq(host, device=hip_device)  # one pinned blob, one copy, decoded on the device
    dev = quantized_dict(cases, dtype, scheme, hip_device)
    plain_dev = dequantize_parameter(dev)  # the server's _dequantize_if_needed path
    plain_host = dequantize_parameter(host)
    for k, (rec, shape) in cases.items():
        assert up[k].device == hip_device and plain_dev[k].device == hip_device and plain_host[k].device.type == "cpu"
        assert_same_bits(up[k], rec, shape, dtype, scheme, f"uploaded {k}")
        assert_same_bits(plain_dev[k], rec, shape, dtype, scheme, f"dequantize_parameter {k}")
        assert torch.equal(plain_dev[k].cpu().view(torch.uint8), plain_host[k].view(torch.uint8)), k
    name = f"n{tile() + 1}@" + ("L255" if scheme == "qsgd" else "W0.01")
    assert_same_bits(dequantize_tensor(dev[name]), *cases[name], dtype, scheme, "dequantize_tensor")
    up2 = deq(host, device=hip_device)  # the blobs are reused
    assert all(torch.equal(up2[k], up[k]) for k in cases)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_and_bad_headers_are_flagged(hip_device, dtype, scheme):
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    rec, shape = overflow_record(dtype, scheme)
    q = as_quantized(rec, shape, dtype, scheme, hip_device)
    buf, view = guarded(shape, torch_dtype(dtype), hip_device)
    ctx.quant_decode(q.codec.code, [q.record], [view.reshape(-1)])
    assert ctx.flags() & _native.FLAG_INPUT_NAN
    assert_same_bits(view, rec, shape, dtype, scheme, "overflow")  # infinities where the oracle has them
    assert not np.isfinite(view.cpu().numpy()).all()
    assert_guards_intact(buf, view)
    ctx.reset()
    assert ctx.flags() == 0
    good_rec, good_shape = next(iter(handmade_records(dtype, scheme).values()))
    good = as_quantized(good_rec, good_shape, dtype, scheme, hip_device)
    deq = BroadcastDequantizer()
    bads = [(rec, shape), bad_header_record(scheme, 0), bad_header_record(scheme, 256)]
    for where in ("device", "uploaded"):
        for brec, bshape in bads:
            bad = as_quantized(brec, bshape, dtype, scheme, hip_device if where == "device" else "cpu")
            g = good if where == "device" else good.to("cpu")
            with pytest.raises(AssertionError) as e:
                deq({"good": g, "bad": bad}, device=hip_device)
            assert isinstance(e.value, NaNAggregationError) and e.value.stage == "input"
            # the context is usable afterwards
            assert_same_bits(deq({"good": g}, device=hip_device)["good"], good_rec, good_shape, dtype, scheme, where)
    # a bad header alone raises the flag at the C entry too
    brec, bshape = bad_header_record(scheme, 256)
    bq = as_quantized(brec, bshape, dtype, scheme, hip_device)
    buf, view = guarded(bshape, torch_dtype(dtype), hip_device)
    ctx.quant_decode(bq.codec.code, [bq.record], [view.reshape(-1)])
    assert ctx.flags() & _native.FLAG_INPUT_NAN
    assert_guards_intact(buf, view)
    ctx.close()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_launch_of_mixed_sizes_equals_per_tensor_calls(hip_device, scheme):
    cases = encoded_records(np.float32, scheme)
    tag = "@L255" if scheme == "qsgd" else "@W0.01"
    names = [k for k in cases if k.endswith(tag)]
    records = quantized_dict({k: cases[k] for k in names}, np.float32, scheme, hip_device)
    code = codec_for(torch.float32, scheme).code
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    batched = [torch.full((records[k].numel,), 9.0, device=hip_device) for k in names]
    ctx.quant_decode(code, [records[k].record for k in names], batched)
    single = [torch.full((records[k].numel,), 9.0, device=hip_device) for k in names]
    for k, o in zip(names, single):
        ctx.quant_decode(code, [records[k].record], [o])
    assert ctx.flags() == 0
    for k, a, b in zip(names, batched, single):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        assert_same_bits(a.reshape(cases[k][1]), *cases[k], np.float32, scheme, k)
    ctx.close()


def test_c_entry_refusals(hip_device):
    lib = _native.load()
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    n = 20
    rec = torch.zeros(codec_for(torch.float32).record_bytes(n) + 16, dtype=torch.uint8, device=hip_device)
    rec[8] = rec[24] = 255  # level 255 and norm 0 at offsets 0 and 16: either record decodes to zeros
    buf, out = guarded((n,), torch.float32, hip_device)
    wbuf, wide = guarded((n,), torch.float64, hip_device)
    u64 = lambda *a: np.array(a, dtype=np.uint64)  # noqa: E731
    i64 = lambda *a: np.array(a, dtype=np.int64)  # noqa: E731
    good = dict(codec=_native.QSGD_F32, r=u64(rec.data_ptr()), n=i64(n), T=1, o=u64(out.data_ptr()), w=None)

    def call(handle=None, **kw):
        a = dict(good)
        a.update(kw)
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.fedavg_quant_decode(handle or ctx._h, a["codec"], p(a["r"]), p(a["n"]), a["T"], p(a["o"]), p(a["w"]),
                                       ctx.stream)

    null = u64(0)
    for kw in (dict(codec=_native.F32), dict(codec=-1), dict(codec=8),  # a bad codec
               dict(r=None), dict(n=None), dict(o=None),  # a NULL table
               dict(T=0), dict(T=-1), dict(T=(1 << 20) + 1),  # the number of tensors
               dict(n=i64(-1)),  # a negative count
               dict(r=null), dict(r=u64(rec.data_ptr() + 8)),  # a NULL or misaligned record
               dict(o=null), dict(o=u64(out.data_ptr() + 2)),  # a NULL output, one not aligned to its element
               dict(w=null), dict(w=u64(wide.data_ptr() + 4)),  # the same for the fp64 output
               dict(codec=_native.QSGD_F64, w=u64(wide.data_ptr())),  # the fp64 copy of an fp64 codec
               dict(codec=_native.NNADQ_F64, w=u64(wide.data_ptr())),
               dict(n=i64((1 << 31) * tile()))):  # 2^31 tiles
        assert call(**kw) == _native.ERR_INVALID and _native.last_error(), kw
    layout = ModelLayout.flat(10_000)
    busy = FedAvgContext(layout, hip_device)
    try:
        table = NativeClientTable(1, hip_device.index or 0)
        for y in [torch.randn(10_000, device=hip_device) for _ in range(7)]:
            table.add_client([y], [1.0])
        res = torch.empty(10_000, dtype=torch.float64, device=hip_device)
        busy.dyn_open(torch.float32, 16)
        assert call(handle=busy._h) == _native.ERR_STATE  # refused while the wave is open
        torch.cuda.current_stream(hip_device).synchronize()
        assert busy.dyn_publish(table) == 7
        assert busy.dyn_close(OutputTable([res], layout, hip_device, torch.float64), torch.float64) == (7, True)
        busy.raise_on_nan()
    finally:
        busy.close()
    assert ctx.flags() == 0  # waits for the stream
    assert bool((buf == 0xA5).all()) and bool((wbuf == 0xA5).all())  # nothing was written
    # NULL where nothing is read or written, and the same arguments are accepted once they are right
    assert call(r=null, o=null, n=i64(0)) == _native.OK
    assert call(r=null, o=null, w=null, n=i64(0)) == _native.OK
    assert call(r=u64(rec.data_ptr() + 16)) == _native.OK  # any 16-byte aligned address
    assert call(w=u64(wide.data_ptr())) == _native.OK
    assert ctx.flags() == 0
    assert bool((out == 0).all()) and bool((wide == 0).all())
    assert_guards_intact(buf, out)
    assert_guards_intact(wbuf, wide)
    ctx.close()


class _Capture:
    def __init__(self, worker_num):
        self.worker_num = worker_num
        self.sent = []

    def broadcast(self, data, worker_ids=None):
        self.sent.append(data)


class _Wire:
    def __init__(self, inbox=()):
        self.inbox = list(inbox)
        self.sent = []

    def get(self):
        return self.inbox.pop(0)

    def send(self, data):
        self.sent.append(data)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_robust_server_round_with_device_records_equals_host_dequantised(hip_device, scheme):
    """The ``_dequantize_if_needed`` consumer: an algorithm that does not fold records gets them
    decoded by the kernel; the round equals the one whose updates were dequantised on the host."""
    shapes = {"w": (tile() + 3,), "b": (33,), "m": (7, 9)}
    g = torch.Generator().manual_seed(8)
    updates = [{k: torch.randn(s, generator=g) for k, s in shapes.items()} for _ in range(5)]
    quant = BroadcastQuantizer(scheme, seed=2)
    host_records = [quant(u, draw) for draw, u in enumerate(updates)]
    results = []
    for on_device in (True, False):
        cap = _Capture(5)
        srv = AggregationServer(algorithm=RobustFedAVGAlgorithm(mode="median", device=hip_device), worker_number=5,
                                endpoint=cap)
        for wid, recs in enumerate(host_records):
            param = ({k: q.to(hip_device) for k, q in recs.items()} if on_device
                     else {k: v.to(hip_device) for k, v in dequantize_parameter(recs).items()})
            srv._process_worker_data(wid, ParameterMessage(parameter=param, aggregation_weight=1.0))
        assert len(srv.results) == 1
        results.append(srv.results[0].parameter)
    for k in shapes:
        a, b = results
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


@pytest.mark.parametrize("scheme", SCHEMES)
def test_round_trip_on_the_device(hip_device, scheme):
    """Workers whose updates lie on the GPU send through their endpoints (the GPU encoder), the
    server folds the records and broadcasts records, a switched-on endpoint uploads and decodes
    them into the model's own parameters: the oracle's decode of what the server sent."""
    shapes = {"w": (tile() + 3,), "b": (33,), "m": (7, 9)}
    g = torch.Generator().manual_seed(9)
    cap = _Capture(3)
    srv = AggregationServer(algorithm=FedAVGAlgorithm(device=hip_device), worker_number=3, endpoint=cap,
                            broadcast_quantizer=BroadcastQuantizer(scheme, seed=5))

    def endpoint(wire, **kw):
        return (StochasticQuantClientEndpoint(endpoint=wire, seed=1, **kw) if scheme == "qsgd"
                else NNADQClientEndpoint(0.01, endpoint=wire, **kw))

    for wid in range(3):
        wire = _Wire()
        update = {k: torch.randn(s, generator=g).to(hip_device) for k, s in shapes.items()}
        endpoint(wire).send(ParameterMessage(parameter=update, aggregation_weight=1.0 + wid))
        assert all(q.record.device == hip_device for q in wire.sent[0].parameter.values())
        cpu = endpoint(_Wire())
        cpu.send(ParameterMessage(parameter={k: v.cpu() for k, v in update.items()}))
        for k in shapes:  # host updates give the same bytes
            assert torch.equal(wire.sent[0].parameter[k].record.cpu(), cpu.sent[0].parameter[k].record), k
        srv._process_worker_data(wid, wire.sent[0])
    assert len(cap.sent) == 1 and cap.sent[0].other_data["quantized"] is True
    sent = {k: (q.record.numpy().copy(), q.shape) for k, q in cap.sent[0].parameter.items()}
    model = {k: torch.zeros(s, dtype=torch.float64, device=hip_device) for k, s in shapes.items()}
    ep = endpoint(_Wire([cap.sent[0]]), device=hip_device, out=model)
    ep.dequant_server_data()
    got = ep.get().parameter
    for k, (rec, shape) in sent.items():
        assert got[k] is model[k]
        assert_same_bits(model[k], rec, shape, np.float64, scheme, k)  # the aggregate is fp64
