"""The record decoder and the quantised client endpoints without a GPU: ``BroadcastDequantizer`` on
host records against the oracles, bit for bit; the endpoints' semantics (quantized_endpoint.py:17-51)
against a fake endpoint; a round trip through ``AggregationServer(broadcast_quantizer=...)``; the
registrations; the refusals."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    BroadcastDequantizer,
    BroadcastQuantizer,
    FedAVGAlgorithm,
    NNADQClientEndpoint,
    QuantClientEndpoint,
    StochasticQuantClientEndpoint,
)
from distributed_learning_simulation_lib_amd.fedavg import NaNAggregationError
from distributed_learning_simulation_lib_amd.message import DeltaParameterMessage, FeatureMessage, ParameterMessage
from distributed_learning_simulation_lib_amd.quantized import (
    NeuralNetworkAdaptiveDeterministicQuant,
    QuantizedTensor,
    dequantize_parameter,
)
from distributed_learning_simulation_lib_amd.server import AggregationServer
from tests.helpers import OracleAlgorithm
from tests.quant_decode_cases import (
    DTYPES,
    SCHEMES,
    as_quantized,
    assert_same_bits,
    bad_header_record,
    encoded_records,
    handmade_records,
    overflow_record,
    quantized_dict,
)
from tests.quant_encode_reference import expected_records


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_records_decode_to_the_oracle_bits(dtype, scheme):
    cases = {**encoded_records(dtype, scheme), **handmade_records(dtype, scheme)}
    records = quantized_dict(cases, dtype, scheme)
    records["dense"] = torch.arange(5.0)  # a dense value passes through
    kept = {k: v.record.clone() for k, v in records.items() if isinstance(v, QuantizedTensor)}
    got = BroadcastDequantizer()(records)
    assert list(got) == list(records) and got["dense"] is records["dense"]
    for k, (rec, shape) in cases.items():
        assert_same_bits(got[k], rec, shape, dtype, scheme, f"{scheme} {np.dtype(dtype)} {k}")
        assert torch.equal(records[k].record, kept[k])  # the records are only read
    # the module-level functions keep the host path: the same bits
    plain = dequantize_parameter(records)
    for k, (rec, shape) in cases.items():
        assert_same_bits(plain[k], rec, shape, dtype, scheme, f"plain {k}")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_and_f64_out_are_written_in_place(scheme):
    cases = handmade_records(np.float32, scheme)
    records = quantized_dict(cases, np.float32, scheme)
    out = {k: torch.full(s, 7.0) for k, (_, s) in cases.items()}
    wide = {k: torch.full(s, 7.0, dtype=torch.float64) for k, (_, s) in cases.items()}
    first = next(iter(cases))
    del out[first]  # a name `out` does not hold gets a new tensor
    got = BroadcastDequantizer()(records, out=out, f64_out=wide)
    for k, (rec, shape) in cases.items():
        assert (got[k] is out[k]) if k in out else (k == first)
        assert_same_bits(got[k], rec, shape, np.float32, scheme, k)
        assert torch.equal(wide[k], got[k].to(torch.float64))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_refusals(scheme):
    cases = handmade_records(np.float32, scheme)
    name, (rec, shape) = next(iter(cases.items()))
    records = {name: as_quantized(rec, shape, np.float32, scheme)}
    deq = BroadcastDequantizer()
    with pytest.raises(ValueError):
        deq(records, out={name: torch.zeros(shape, dtype=torch.float64)})  # wrong dtype
    with pytest.raises(ValueError):
        deq(records, out={name: torch.zeros(*shape, 2)[..., 0]})  # not contiguous
    with pytest.raises(ValueError):
        deq(records, out={name: torch.zeros(7)})  # wrong shape
    with pytest.raises(ValueError):
        deq(records, f64_out={name: torch.zeros(shape)})  # the wide copy is fp64
    rec64, shape64 = next(iter(handmade_records(np.float64, scheme).values()))
    with pytest.raises(ValueError):  # an fp64 record has no wide copy
        deq({"w": as_quantized(rec64, shape64, np.float64, scheme)},
            f64_out={"w": torch.zeros(shape64, dtype=torch.float64)})
    # flagged records: an overflow, a level outside [1, 255]; nothing is handed out
    for dtype in DTYPES:
        for bad, bshape in [overflow_record(dtype, scheme), bad_header_record(scheme, 0),
                            bad_header_record(scheme, 256)]:
            with pytest.raises(AssertionError) as e:
                deq({**records, "bad": as_quantized(bad, bshape, dtype, scheme)})
            assert isinstance(e.value, NaNAggregationError) and e.value.stage == "input"
    assert_same_bits(deq(records)[name], rec, shape, np.float32, scheme, "after the refusals")


class FakeEndpoint:
    """What the endpoints wrap: a queue to ``get`` from and a list of what was sent."""

    color = "green"

    def __init__(self, inbox=()):
        self.inbox = list(inbox)
        self.sent = []

    def get(self):
        return self.inbox.pop(0)

    def send(self, data):
        self.sent.append(data)

    def has_data(self):
        return bool(self.inbox)


def _records(scheme="qsgd"):
    x = {"w": torch.linspace(-1, 1, 300), "b": torch.linspace(0, 3, 17, dtype=torch.float64)}
    return x, BroadcastQuantizer(scheme, seed=3)(x, 1)


@pytest.mark.parametrize("make", [lambda e: StochasticQuantClientEndpoint(endpoint=e, seed=9),
                                  lambda e: NNADQClientEndpoint(0.01, endpoint=e)], ids=["qsgd", "nnadq"])
def test_get_decodes_only_once_switched_on(make):
    scheme = "qsgd" if isinstance(make(FakeEndpoint()), StochasticQuantClientEndpoint) else "nnadq"
    _, recs = _records(scheme)
    feature = FeatureMessage(feature=torch.ones(3))
    inner = FakeEndpoint([ParameterMessage(parameter=dict(recs)), None, ParameterMessage(parameter=dict(recs)), None,
                          feature])
    ep = make(inner)
    assert ep.color == "green" and ep.has_data() is True  # every other attribute is the wrapped endpoint's
    with pytest.raises(AttributeError):
        ep.no_such_attribute  # noqa: B018
    first = ep.get()
    assert all(isinstance(v, QuantizedTensor) for v in first.parameter.values())  # not switched on: untouched
    assert ep.get() is None
    ep.dequant_server_data()
    msg = ep.get()
    for k, q in recs.items():
        dt = np.float64 if q.codec.value_dtype == torch.float64 else np.float32
        assert_same_bits(msg.parameter[k], q.record.numpy(), q.shape, dt, scheme, k)
    assert ep.get() is None  # None passes through
    with pytest.raises(AssertionError):
        ep.get()  # a FeatureMessage where the broadcast is expected


def test_get_decodes_into_the_configured_out():
    x, recs = _records("qsgd")
    out = {k: torch.zeros_like(v) for k, v in x.items()}
    ep = StochasticQuantClientEndpoint(endpoint=FakeEndpoint([ParameterMessage(parameter=dict(recs))]), seed=1, out=out)
    ep.dequant_server_data()
    msg = ep.get()
    assert all(msg.parameter[k] is out[k] for k in x)
    assert_same_bits(out["w"], recs["w"].record.numpy(), recs["w"].shape, np.float32, "qsgd")


def test_send_quantises_parameter_messages_only():
    x, _ = _records()
    inner = FakeEndpoint()
    ep = StochasticQuantClientEndpoint(endpoint=inner, seed=0x1234)
    assert ep.seed == 0x1234 and ep.draw == 0
    delta = DeltaParameterMessage(delta_parameter=dict(x))
    feature = FeatureMessage(feature=torch.ones(2))
    for data in (delta, feature, None, "text"):
        ep.send(data)
    assert inner.sent[0] is delta and all(delta.delta_parameter[k] is x[k] for k in x)  # the client sends deltas dense
    assert inner.sent[1] is feature and inner.sent[2] is None and inner.sent[3] == "text"
    assert ep.draw == 0  # nothing was drawn for them
    ep.send(ParameterMessage(parameter=dict(x), aggregation_weight=3.0))
    ep.send(ParameterMessage(parameter=dict(x), aggregation_weight=3.0))
    a, b = inner.sent[4], inner.sent[5]
    assert ep.draw == 2 and a.aggregation_weight == 3.0
    p = {k: v.numpy() for k, v in x.items()}
    for draw, msg in enumerate((a, b)):  # the contract's records at level 255, draw = the send's number
        want = expected_records(p, "qsgd", 255, seed=0x1234, draw=draw)
        for k in x:
            assert np.array_equal(msg.parameter[k].record.numpy(), want[k]), (draw, k)
    assert not torch.equal(a.parameter["w"].record, b.parameter["w"].record)  # the draw advances per send
    again = StochasticQuantClientEndpoint(endpoint=FakeEndpoint(), seed=0x1234)
    again.send(ParameterMessage(parameter=dict(x)))
    assert all(torch.equal(again.sent[0].parameter[k].record, a.parameter[k].record) for k in x)  # same seed and draw
    fresh = [StochasticQuantClientEndpoint(endpoint=FakeEndpoint()).seed for _ in range(2)]
    assert fresh[0] != fresh[1] and all(0 <= s < 1 << 64 for s in fresh)  # seed=None: os.urandom


def test_after_quant_is_called(monkeypatch):
    x, _ = _records()
    calls = []
    monkeypatch.setattr(NeuralNetworkAdaptiveDeterministicQuant, "check_compression_ratio",
                        staticmethod(lambda quantized_data, prefix="": calls.append((quantized_data, prefix))))
    inner = FakeEndpoint()
    ep = NNADQClientEndpoint(weight=0.5, endpoint=inner)
    msg = ParameterMessage(parameter=dict(x))
    ep.send(msg)
    ep.send(DeltaParameterMessage(delta_parameter=dict(x)))
    assert calls == [(msg, "worker")]
    want = expected_records({k: v.numpy() for k, v in x.items()}, "nnadq", weight=0.5)
    assert all(np.array_equal(inner.sent[0].parameter[k].record.numpy(), want[k]) for k in x)

    class Counting(QuantClientEndpoint):
        seen = 0

        def _after_quant(self, data):
            type(self).seen += 1

    plain = Counting(lambda p: {k: v * 2 for k, v in p.items()}, lambda p: p, endpoint=FakeEndpoint())
    plain.send(ParameterMessage(parameter={"w": torch.ones(2)}))
    assert Counting.seen == 1 and torch.equal(plain.sent[0].parameter["w"], torch.full((2,), 2.0))
    with pytest.raises(TypeError):
        QuantClientEndpoint(lambda p: p, lambda p: p, endpoint=FakeEndpoint(), color="red")
    with pytest.raises(TypeError):
        QuantClientEndpoint(lambda p: p, lambda p: p, endpoint=object())
    with pytest.raises(TypeError):
        NNADQClientEndpoint(endpoint=FakeEndpoint())  # the weight has no default


@pytest.mark.parametrize("scheme", SCHEMES)
def test_round_trip_through_the_server(scheme):
    """Workers send through their endpoints, the server aggregates and broadcasts records, a
    switched-on endpoint decodes them: the oracle's decode of the records the server sent."""

    class Capture:
        worker_num = 2

        def __init__(self):
            self.sent = []

        def broadcast(self, data, worker_ids=None):
            self.sent.append(data)

    cap = Capture()
    srv = AggregationServer(algorithm=OracleAlgorithm(), worker_number=2, endpoint=cap,
                            broadcast_quantizer=BroadcastQuantizer(scheme, seed=5))
    shapes = {"w": (700,), "b": (33,), "m": (4, 6)}
    g = torch.Generator().manual_seed(4)
    for wid in range(2):
        wire = FakeEndpoint()
        ep = (StochasticQuantClientEndpoint(endpoint=wire, seed=wid) if scheme == "qsgd"
              else NNADQClientEndpoint(0.01, endpoint=wire))
        ep.send(ParameterMessage(parameter={k: torch.randn(s, generator=g) for k, s in shapes.items()},
                                 aggregation_weight=1.0 + wid))
        assert all(isinstance(v, QuantizedTensor) for v in wire.sent[0].parameter.values())
        srv._process_worker_data(wid, wire.sent[0])
    assert len(cap.sent) == 1 and cap.sent[0].other_data["quantized"] is True
    sent = {k: (v.record.numpy().copy(), v.shape) for k, v in cap.sent[0].parameter.items()}
    ep = (StochasticQuantClientEndpoint if scheme == "qsgd" else lambda **kw: NNADQClientEndpoint(0.01, **kw))(
        endpoint=FakeEndpoint([cap.sent[0]]))
    ep.dequant_server_data()
    got = ep.get().parameter
    for k, (rec, shape) in sent.items():
        assert_same_bits(got[k], rec, shape, np.float64, scheme, k)  # the aggregate is fp64


def test_registrations_exist_and_construct(monkeypatch):
    for name, cls in (("fed_avg_qsgd", StochasticQuantClientEndpoint), ("fed_avg_nnadq", NNADQClientEndpoint)):
        entry = AlgorithmRepository.config[name]
        assert entry["server_cls"] is AggregationServer and entry["algorithm_cls"] is FedAVGAlgorithm
        assert entry["client_endpoint_cls"] is cls

    class Context:  # what create_client asks of the simulator's context
        def create_client_endpoint(self, endpoint_cls, **kwargs):
            return endpoint_cls(endpoint=FakeEndpoint(), **kwargs)

    class Worker:
        def __init__(self, endpoint, context):
            self.endpoint = endpoint

    # the client class is the simulator's worker, outside this package: a stand-in for the construction
    for name in ("fed_avg_qsgd", "fed_avg_nnadq"):
        monkeypatch.setitem(AlgorithmRepository.config[name], "client_cls", Worker)
    a = AlgorithmRepository.create_client("fed_avg_qsgd", {}, {"seed": 7}, context=Context())
    assert isinstance(a.endpoint, StochasticQuantClientEndpoint) and a.endpoint.seed == 7
    b = AlgorithmRepository.create_client("fed_avg_nnadq", {}, {"weight": 0.25}, context=Context())
    assert isinstance(b.endpoint, NNADQClientEndpoint) and b.endpoint._quant.weight == 0.25
    with pytest.raises(TypeError):
        AlgorithmRepository.create_client("fed_avg_nnadq", {}, {}, context=Context())
