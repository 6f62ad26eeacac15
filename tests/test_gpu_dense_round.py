"""The eight side algorithms at the smallest round each allows, on the GPU: a layout with an empty
tensor in the middle, which the native layout leaves out and the result must still hold in its place.
Every output's key order, shape, dtype and device, and the same bits as the class gives on the CPU
device (the values are small integers, so every sum is exact)."""

from __future__ import annotations

import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    BulyanFedAVGAlgorithm,
    ClippedFedAVGAlgorithm,
    DeltaParameterMessage,
    FLTrustFedAVGAlgorithm,
    GeometricMedianFedAVGAlgorithm,
    KrumFedAVGAlgorithm,
    ParameterMessage,
    RobustFedAVGAlgorithm,
    ServerOptFedAVGAlgorithm,
    SparseFedAVGAlgorithm,
)

pytestmark = pytest.mark.gpu

SHAPES = {"a": (5,), "e": (0,), "b": (2, 3)}     # in this key order
# (the class, its smallest valid arguments, the fewest clients its rule allows)
CASES = {
    "robust": (RobustFedAVGAlgorithm, {}, 2),
    "krum": (KrumFedAVGAlgorithm, {"num_byzantine": 0}, 3),
    "bulyan": (BulyanFedAVGAlgorithm, {"num_byzantine": 0}, 3),
    "geomed": (GeometricMedianFedAVGAlgorithm, {}, 2),
    "clip": (ClippedFedAVGAlgorithm, {"radius": 1.0}, 2),
    "fltrust": (FLTrustFedAVGAlgorithm, {"root_worker": 10}, 2),
    "opt": (ServerOptFedAVGAlgorithm, {"optimizer": "avgm"}, 2),
    "sparse": (SparseFedAVGAlgorithm, {}, 2),
}


def model(offset: int) -> dict[str, torch.Tensor]:
    """fp32 tensors of SHAPES holding the integers offset, offset + 1, ..."""
    out, start = {}, offset
    for name, shape in SHAPES.items():
        numel = torch.Size(shape).numel()
        out[name] = torch.arange(start, start + numel, dtype=torch.float32).reshape(shape)
        start += numel
    return out


def run(name: str, device: str, out_dtype: torch.dtype) -> dict[str, torch.Tensor]:
    cls, kwargs, n = CASES[name]
    algo = cls(device=device, out_dtype=out_dtype, **kwargs)
    algo.set_old_parameter(model(1))
    for row in range(n):
        update = model(3 + 2 * row)
        if name == "sparse":
            msg = DeltaParameterMessage(delta_parameter=update, aggregation_weight=1 + row)
        else:
            msg = ParameterMessage(parameter=update, aggregation_weight=1 + row)
        algo.process_worker_data(10 + row, msg)
    return algo.aggregate_worker_data().parameter


@pytest.mark.parametrize("name", list(CASES))
def test_smallest_round_with_an_empty_tensor(name):
    here = torch.device("cuda", torch.cuda.current_device())
    for out_dtype in (torch.float64, torch.float32):
        got = run(name, "cuda", out_dtype)
        want = run(name, "cpu", out_dtype)
        assert list(got) == list(SHAPES) == list(want)
        for key, shape in SHAPES.items():
            assert tuple(got[key].shape) == shape and got[key].dtype == out_dtype, key
            assert got[key].device == here, key          # "cuda" resolved to the current device's index
            assert want[key].device.type == "cpu" and want[key].dtype == out_dtype, key
            assert torch.equal(got[key].cpu().view(torch.uint8), want[key].contiguous().view(torch.uint8)), key
