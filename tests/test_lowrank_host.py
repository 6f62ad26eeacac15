"""Low-rank deltas on the host: the wire type against the numpy restatement (tests/lowrank_reference.py,
DESIGN.md §5aa), the power-iteration client step and its error feedback, and the CPU path of
LowRankFedAVGAlgorithm bit for bit against the restatement."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AlgorithmRepository,
    DeltaParameterMessage,
    LowRankDelta,
    LowRankEndpoint,
    LowRankErrorFeedback,
    LowRankFedAVGAlgorithm,
    lowrank_compress,
)
from distributed_learning_simulation_lib_amd.lowrank import densify_parameter, is_lowrank
from tests import lowrank_reference as ref

CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64], ids=["f32", "f16", "bf16", "f64"])
def test_to_dense_is_the_restatement_rounded_into_the_dtype(dtype):
    gen = torch.Generator().manual_seed(3)
    d = LowRankDelta(torch.randn(7, 3, generator=gen).to(dtype), torch.randn(3, 10, generator=gen).to(dtype), (7, 5, 2))
    want, _, _ = ref.lowrank_fold([d.left.double().numpy()], [d.right.double().numpy()], [1.0], 1.0, np.zeros((7, 10)))
    dense = d.to_dense()
    assert dense.dtype == dtype and dense.shape == (7, 5, 2) and d.numel == 70 and d.rank == 3
    assert torch.equal(dense.reshape(7, 10), torch.from_numpy(want).to(dtype))
    assert is_lowrank({"w": d}) and not is_lowrank({"w": dense})
    assert torch.equal(densify_parameter({"w": d, "b": dense})["w"], dense)


def test_compress_is_one_power_iteration_step_with_an_exact_residual():
    gen = torch.Generator().manual_seed(5)
    delta = torch.randn(24, 6, 5, generator=gen, dtype=torch.float64)
    error = torch.randn(24, 6, 5, generator=gen, dtype=torch.float64) * 0.1
    sent, new_error = lowrank_compress(delta, 4, error=error)
    assert isinstance(sent, LowRankDelta) and sent.left.shape == (24, 4) and sent.right.shape == (4, 30)
    gram = sent.left.T @ sent.left
    assert float((gram - torch.eye(4, dtype=torch.float64)).abs().max()) <= 1e-12
    M = (delta + error).reshape(24, 30)
    assert torch.equal(sent.right, sent.left.T @ M)
    # left @ right + new_error is M up to the rounding of the product, the subtraction and this sum
    back = sent.left @ sent.right + new_error.reshape(24, 30)
    assert float((back - M).abs().max()) <= 8 * 2.0 ** -53 * float(M.abs().max() + (sent.left.abs() @ sent.right.abs()).max())
    # the dense fallback: 1-D tensors and tensors the factors would not make smaller
    for small in (torch.randn(9, generator=gen), torch.randn(4, 4, generator=gen)):
        out, err = lowrank_compress(small, 2)
        assert out is small and not err.any() and err.shape == small.shape
    with pytest.raises(ValueError, match="rank"):
        lowrank_compress(delta, 17)


def test_error_feedback_carries_the_error_and_the_warm_start():
    gen = torch.Generator().manual_seed(7)
    feedback = LowRankErrorFeedback(rank=2)
    diffs = [{"w": torch.randn(12, 9, generator=gen, dtype=torch.float64), "b": torch.randn(12, generator=gen)}
             for _ in range(2)]
    first = feedback.compress(DeltaParameterMessage(delta_parameter=diffs[0], aggregation_weight=3.0))
    assert isinstance(first.delta_parameter["w"], LowRankDelta) and first.delta_parameter["b"] is diffs[0]["b"]
    assert first.aggregation_weight == 3.0
    want0, err0 = lowrank_compress(diffs[0]["w"], 2)
    assert torch.equal(feedback.error("w"), err0) and torch.equal(feedback.warm_start("w"), want0.right)
    second = feedback.compress(DeltaParameterMessage(delta_parameter=diffs[1], aggregation_weight=1.0))
    want1, err1 = lowrank_compress(diffs[1]["w"], 2, right_prev=want0.right, error=err0)
    assert torch.equal(second.delta_parameter["w"].left, want1.left) and torch.equal(feedback.error("w"), err1)
    sent = []
    LowRankEndpoint(type("Sink", (), {"send": lambda self, d: sent.append(d)})(), rank=2).send(
        DeltaParameterMessage(delta_parameter=diffs[0], aggregation_weight=1.0))
    assert torch.equal(sent[0].delta_parameter["w"].left, want0.left)
    assert AlgorithmRepository.has_algorithm("fed_avg_lowrank")
    assert AlgorithmRepository.config["fed_avg_lowrank_ef"]["client_endpoint_cls"] is LowRankEndpoint


@pytest.mark.parametrize("integers", [True, False], ids=["integers", "gaussian"])
def test_the_cpu_class_is_the_restatement_bit_for_bit(integers):
    gen = torch.Generator().manual_seed(11)

    def draw(*shape):
        x = torch.randint(-8, 9, shape, generator=gen).double() if integers else torch.randn(*shape, generator=gen, dtype=torch.float64)
        return x.float()

    prev = {"w": draw(19, 6, 3).double(), "b": draw(19).double()}
    msgs = [({"w": LowRankDelta(draw(19, 3), draw(3, 18), (19, 6, 3)), "b": draw(19)}, w) for w in (1.0, 2.5, 0.75)]
    algorithm = LowRankFedAVGAlgorithm(device=CPU)
    algorithm.set_old_parameter(prev)
    for wid, (d, w) in enumerate(msgs):
        algorithm.process_worker_data(wid, DeltaParameterMessage(delta_parameter=d, aggregation_weight=w))
    got = algorithm.aggregate_worker_data().parameter
    ws = [w for _, w in msgs]
    W = ws[0] + ws[1] + ws[2]
    want, _, _ = ref.lowrank_fold([d["w"].left.double().numpy() for d, _ in msgs], [d["w"].right.double().numpy() for d, _ in msgs],
                                  ws, W, prev["w"].numpy().reshape(19, 18))
    assert got["w"].shape == (19, 6, 3) and got["w"].dtype == torch.float64
    assert torch.equal(got["w"].reshape(19, 18).view(torch.int64), torch.from_numpy(want).view(torch.int64))
    acc = None
    for d, w in msgs:
        p = (prev["b"].numpy() + d["b"].double().numpy()) * np.float64(w)
        acc = p if acc is None else acc + p
    assert torch.equal(got["b"].view(torch.int64), torch.from_numpy(acc / np.float64(W)).view(torch.int64))
