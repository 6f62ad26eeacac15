"""The low-rank client step without a GPU (fedavg_lowrank_compress): the binding, the
kernel's geometry constants, and the torch composition as the path of host tensors."""

from __future__ import annotations

import pytest
import torch

from distributed_learning_simulation_lib_amd import LowRankDelta, _native, lowrank_compress
from distributed_learning_simulation_lib_amd.lowrank import _lowrank_compress_torch


def test_the_binding_declares_the_step():
    assert "fedavg_lowrank_compress" in _native.SIGNATURES


def test_the_geometry_is_readable_without_a_gpu():
    tm, tn = _native.kernel_constant("lowrank_tm"), _native.kernel_constant("lowrank_tn")
    assert _native.kernel_constant("lowrank_chunk_cols") % tn == 0
    assert _native.kernel_constant("lowrank_chunk_rows") % tm == 0
    # P of that many rows, 16 fp64 columns wide, fits the 64 KiB of a workgroup
    assert 0 < _native.kernel_constant("lowrank_ortho_lds_rows") * 16 * 8 < 64 * 1024


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_host_tensor_takes_the_torch_composition(dtype):
    gen = torch.Generator().manual_seed(2)
    delta, error = torch.randn(20, 3, 5, generator=gen).to(dtype), torch.randn(20, 3, 5, generator=gen).to(dtype)
    start = torch.randn(3, 15, generator=gen).to(dtype)
    got, want = lowrank_compress(delta, 3, start, error), _lowrank_compress_torch(delta, 3, start, error)
    assert isinstance(got[0], LowRankDelta)
    assert torch.equal(got[0].left, want[0].left) and torch.equal(got[0].right, want[0].right)
    assert torch.equal(got[1], want[1])
    flat = torch.randn(9, generator=gen).to(dtype)
    assert lowrank_compress(flat, 3)[0] is flat and _lowrank_compress_torch(flat, 3)[0] is flat
