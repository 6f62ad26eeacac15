"""The top-k step (fedavg_topk_sparsify) on a tensor of more than 256 tiles, bit for bit
against the CPU ``topk_sparsify``: the scan of the tile counts makes a second trip there and carries
the counts of the greater and of the equal keys into it; and the workspace regrown between calls that
are still in flight. The shapes up to two chunks are in tests/test_gpu_topk.py."""

from __future__ import annotations

import functools

import pytest
import torch

from distributed_learning_simulation_lib_amd import _native
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout
from tests.test_gpu_topk import Call, chunk, tile, values

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


def edge() -> int:
    """The first element of the scan's second trip: one tile per lane in the first."""
    return _native.kernel_constant("topk_threads") * tile()


def numel() -> int:
    return edge() + tile() + 7


@pytest.fixture(scope="module")
def ctx(hip_device):
    c = FedAvgContext(ModelLayout.flat(1, "topk"), hip_device)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def straddling(dtype: torch.dtype) -> tuple[torch.Tensor, int]:
    """(delta, the number of its magnitudes above 1.5): small values, 40 values of magnitude 3 on both
    sides of the edge, and 40 of magnitude 1.5 with alternating signs from 20 before it to 20 past it."""
    n, e = numel(), edge()
    gen = torch.Generator().manual_seed(43)
    delta = values(gen, n, dtype, 0.001)
    before = torch.randperm(e - 20, generator=gen)[:20]
    after = e + 20 + torch.randperm(n - e - 20, generator=gen)[:20]
    delta[torch.cat([before, after])] = 3.0
    group = torch.arange(e - 20, e + 20)
    delta[group] = torch.where(group % 2 == 0, 1.5, -1.5).to(dtype)
    above = int((delta.abs() > 1.5).sum())
    assert above == 40 and int((delta.abs() == 1.5).sum()) == 40 and float(delta.abs().max()) == 3.0
    return delta, above


def test_the_shape_reaches_the_second_trip():
    threads, tl = _native.kernel_constant("topk_threads"), tile()
    assert -(-numel() // tl) == threads + 2 and numel() % tl == 7  # two tiles in the second trip, the last ragged
    assert -(-numel() // chunk()) * 2048 * 4 > 1 << 16  # the chunks' histograms outgrow the first 64 KiB


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_equal_keys_past_256_tiles_go_to_the_lower_index(ctx, hip_device, dtype):
    """Every key equal: the equal-count prefix alone decides, and it has to cross into the second trip."""
    n, e = numel(), edge()
    delta = torch.full((n,), -0.75, dtype=dtype)
    keeps = [e, e + 5, n]
    c = Call(hip_device, [delta] * 3, [None] * 3, keeps).run(ctx)
    c.check("all equal")
    for (i, _, _), k in zip(c.outputs(), keeps):
        assert torch.equal(i, torch.arange(k, dtype=torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cut_before_at_and_after_the_second_trip(ctx, hip_device, dtype):
    delta, above = straddling(dtype)
    keeps = [above, above + 1, above + 19, above + 20, above + 21, above + 40, above + 41]
    Call(hip_device, [delta] * len(keeps), [None] * len(keeps), keeps).run(ctx).check("group over the scan's edge")


def test_workspace_regrown_between_calls_in_flight(hip_device):
    """A fresh context: a small call, the call of 33 chunks that outgrows the first 64 KiB, and the
    small call again, with nothing waiting in between."""
    gen = torch.Generator().manual_seed(47)
    sizes = [tile() + 3, 5]
    deltas = [values(gen, s, torch.float32) for s in sizes]
    errors = [values(gen, sizes[0], torch.float32, 0.03), None]
    big, above = straddling(torch.float32)
    first, again = (Call(hip_device, deltas, errors, [40, 2], [1, 0]) for _ in range(2))
    large = Call(hip_device, [big], [None], [above + 20])
    fresh = FedAvgContext(ModelLayout.flat(1, "topk"), hip_device)
    try:
        torch.cuda.synchronize(hip_device)
        for c in (first, large, again):
            c.run(fresh)
        torch.cuda.synchronize(hip_device)
    finally:
        fresh.close()
    first.check("the small call")
    large.check("the large call")
    again.check("the small call again")
