"""The client-side top-k step above the kernel, on the CPU: the dict function against
the per-tensor calls, the error-feedback state, the endpoint, the registration and the ABI names.
The oracle is the per-tensor CPU ``topk_sparsify`` (torch's stable sort) and the numpy restatement
``tests/sparse_reference.topk``. No GPU needed.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    DeltaParameterMessage,
    ParameterMessage,
    SparseDelta,
    SparseFedAVGAlgorithm,
    TopKErrorFeedback,
    TopKSparseEndpoint,
    _native,
    topk_sparsify,
    topk_sparsify_parameter,
)
from distributed_learning_simulation_lib_amd.server import AggregationServer
from distributed_learning_simulation_lib_amd.sparse import topk_count
from tests import sparse_reference as ref
from tests.test_abi import header_functions


def same_sparse(got: SparseDelta, want: SparseDelta, what: str) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype and got.indices.dtype == torch.int32, what
    assert got.indices.tolist() == want.indices.tolist(), what
    same_dense(got.values, want.values, what)


def same_dense(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype, what
    as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    assert torch.equal(got.contiguous().view(as_int), want.contiguous().view(as_int)), what


def model(dtype=torch.float32, seed=5):
    gen = torch.Generator().manual_seed(seed)
    shapes = {"conv.weight": (6, 3, 3, 3), "bn.bias": (6,), "fc.weight": (10, 37), "scalar": (), "empty": (0, 4)}
    return {n: (torch.randn(s, generator=gen) * 0.1).to(dtype) for n, s in shapes.items()}


@pytest.mark.parametrize("kw", [{"k": 1}, {"k": 9}, {"ratio": 0.1}, {"ratio": 1.0}])
def test_dict_function_equals_the_per_tensor_calls(kw):
    delta = model()
    error = {n: v * 0.5 for n, v in model(seed=6).items() if n != "bn.bias"}  # one name has no residual yet
    for err in (None, error):
        sent, residual = topk_sparsify_parameter(delta, error=err, **kw)
        assert list(sent) == list(delta) == list(residual)
        for n, v in delta.items():
            s, r = topk_sparsify(v, error=None if err is None else err.get(n), **kw)
            assert sent[n].nnz == topk_count(v.numel(), **kw)
            same_sparse(sent[n], s, n)
            same_dense(residual[n], r, n)
            total = v if err is None or n not in err else v + err[n]
            idx, val, res = ref.topk(total.numpy(), sent[n].nnz)
            assert sent[n].indices.tolist() == idx.tolist() and np.array_equal(residual[n].numpy().reshape(-1), res)
            assert np.array_equal(sent[n].values.numpy(), val)


def test_dict_function_with_mixed_dtypes_and_its_refusals():
    delta = {"a": model()["fc.weight"], "b": model(torch.float16)["fc.weight"], "c": model(torch.float64)["bn.bias"],
             "d": model(torch.bfloat16)["conv.weight"]}
    sent, residual = topk_sparsify_parameter(delta, ratio=0.25)
    for n, v in delta.items():
        s, r = topk_sparsify(v, ratio=0.25)
        same_sparse(sent[n], s, n)
        same_dense(residual[n], r, n)
    assert topk_sparsify_parameter({}, k=1) == ({}, {})
    with pytest.raises(TypeError):
        topk_sparsify_parameter({"a": delta["a"], "n": torch.arange(4)}, k=1)
    with pytest.raises(TypeError):
        topk_sparsify_parameter({"a": [1.0, 2.0]}, k=1)
    for bad in ({}, {"k": 3, "ratio": 0.5}, {"ratio": 0.0}, {"ratio": 1.5}, {"k": -1}, {"k": 2.5}):
        with pytest.raises(ValueError):
            topk_sparsify_parameter(delta, **bad)
        with pytest.raises(ValueError):
            TopKErrorFeedback(**bad)


def test_error_feedback_sends_or_keeps_every_element_whole_over_three_rounds():
    gen = torch.Generator().manual_seed(9)
    shapes = {"w": (20, 9), "b": (7,), "steps": (3,)}
    fb = TopKErrorFeedback(ratio=0.1)
    assert fb.error("w") is None
    for rnd in range(3):
        delta = {"w": torch.randn(shapes["w"], generator=gen) * 0.1,
                 "b": (torch.randn(shapes["b"], generator=gen) * 0.1).to(torch.float16),
                 "steps": torch.tensor([rnd, 2 * rnd, 7], dtype=torch.int64)}
        old = {n: fb.error(n) for n in delta}
        msg = DeltaParameterMessage(delta_parameter=delta, aggregation_weight=3.0, in_round=True,
                                    other_data={"round": rnd})
        out = fb.sparsify(msg)
        assert type(out) is DeltaParameterMessage and out is not msg and msg.delta_parameter is delta
        assert out.aggregation_weight == 3.0 and out.in_round and out.other_data == {"round": rnd}
        assert out.delta_parameter["steps"] is delta["steps"] and fb.error("steps") is None  # dense and untouched
        for n in ("w", "b"):
            sent = out.delta_parameter[n]
            assert isinstance(sent, SparseDelta) and sent.nnz == topk_count(delta[n].numel(), ratio=0.1)
            total = delta[n] if old[n] is None else delta[n] + old[n]
            assert (old[n] is None) == (rnd == 0)
            same_dense(sent.to_dense() + fb.error(n), total, f"round {rnd} {n}")
            want, res = topk_sparsify(delta[n], ratio=0.1, error=old[n])
            same_sparse(sent, want, n)
            same_dense(fb.error(n), res, n)
    with pytest.raises(ValueError, match="w"):
        fb.sparsify(DeltaParameterMessage(delta_parameter={"w": torch.zeros(21, 9)}))
    with pytest.raises(ValueError, match="b"):
        fb.sparsify(DeltaParameterMessage(delta_parameter={"b": torch.zeros(7)}))  # fp16 before
    fb.reset()
    assert fb.error("w") is None and fb.error("b") is None
    out = fb.sparsify(DeltaParameterMessage(delta_parameter={"w": torch.ones(21, 9)}))
    assert out.delta_parameter["w"].indices.tolist() == list(range(topk_count(189, ratio=0.1)))


class Sink:
    def __init__(self):
        self.sent = []
        self.worker_id = 4

    def send(self, data):
        self.sent.append(data)


def test_endpoint_sparsifies_diffs_and_forwards_everything_else():
    sink = Sink()
    ep = TopKSparseEndpoint(sink, k=3)
    assert ep.worker_id == 4 and ep.feedback.k == 3
    full = ParameterMessage(parameter={"w": torch.ones(5)})
    ep.send(full)
    ep.send("anything")
    assert sink.sent[0] is full and torch.equal(full.parameter["w"], torch.ones(5)) and sink.sent[1] == "anything"
    delta = {"w": torch.tensor([0.5, -3.0, 2.0, -2.0, 0.25, 1.0])}
    ep.send(DeltaParameterMessage(delta_parameter=delta, aggregation_weight=2.0))
    got = sink.sent[2]
    assert got.aggregation_weight == 2.0 and got.delta_parameter["w"].indices.tolist() == [1, 2, 3]
    assert ep.feedback.error("w").tolist() == [0.5, 0.0, 0.0, 0.0, 0.25, 1.0]
    ep.send(DeltaParameterMessage(delta_parameter={"w": torch.zeros(6)}))
    assert sink.sent[3].delta_parameter["w"].indices.tolist() == [0, 4, 5]  # the residual goes out next
    assert TopKSparseEndpoint(Sink()).feedback.ratio == 0.01
    with pytest.raises(TypeError):
        TopKSparseEndpoint(object(), k=1)
    with pytest.raises(TypeError):
        TopKSparseEndpoint(Sink(), k=1, colour="red")
    with pytest.raises(ValueError):
        TopKSparseEndpoint(Sink(), k=1, ratio=0.5)


def test_registration_and_abi_names():
    entry = AlgorithmRepository.config["fed_avg_sparse_topk"]
    assert entry["client_endpoint_cls"] is TopKSparseEndpoint
    assert entry["algorithm_cls"] is SparseFedAVGAlgorithm and entry["server_cls"] is AggregationServer
    assert header_functions() == set(_native.SIGNATURES) and "fedavg_topk_sparsify" in _native.SIGNATURES
    tile, chunk, threads = (_native.kernel_constant(f"topk_{n}") for n in ("tile", "chunk", "threads"))
    assert tile > 0 and chunk > 0 and threads % 64 == 0 and tile % threads == 0
