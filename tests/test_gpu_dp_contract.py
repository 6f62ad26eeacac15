"""What the clip-and-noise kernels (fedavg_dp_noise) promise beyond the shapes of
tests/test_gpu_dp.py, bit for bit against the numpy restatement (tests/dp_reference.py): the
workspace regrown between calls that are still in flight, shifted groups that cross from one row into
the next, and the one rounding into fp16 and bf16 at rows where a second rounding shows. The teams
of 64, 128 and 256 lanes, the 1500 rows and the scale pass's second trip come in through
``dp_cases.row_cases()`` and the list case "many", which tests/test_gpu_dp.py runs."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout
from tests import dp_cases as cases
from tests import dp_reference as ref
from tests import dp_rounding_cases as rounding
from tests.test_gpu_dp import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_device):
    c = FedAvgContext(ModelLayout.flat(1, "dp"), hip_device)
    yield c
    c.close()


def _same(got: bytes, want: bytes, itemsize: int, what) -> None:
    if got != want:
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        bad = np.unique(np.flatnonzero(a != b) // itemsize)
        raise AssertionError(f"{what}: {bad.size} elements differ from the restatement, first at {bad[:8]}")


def _run(ctx, src, dst, c, noise_scale, ids=None, row_len=0) -> None:
    ctx.dp_noise([g.tensor for g in src], [g.tensor for g in dst], c, noise_scale, cases.SEED, cases.DRAW, ids, row_len)


def test_workspace_regrown_between_calls_in_flight(hip_device):
    """A fresh context: a small whole-list call, the 1500-row call that outgrows the partials' and
    the scales' first 1024 entries, and the small call again, with nothing waiting in between."""
    rows, length = max(cases.row_cases())
    assert rows > 1024
    xs, c, want_small = cases.list_case("three", "f32")
    big, want_big = cases.row_case(rows, length, "f32")
    offsets = cases.list_offsets("three")
    src = [Guarded(x, hip_device, o) for x, o in zip(xs, offsets)]
    first, again = ([Guarded(torch.zeros_like(x), hip_device, o) for x, o in zip(xs, offsets)] for _ in range(2))
    big_src, big_dst = Guarded(big, hip_device), Guarded(torch.zeros_like(big), hip_device)
    fresh = FedAvgContext(ModelLayout.flat(1, "dp"), hip_device)
    try:
        torch.cuda.synchronize(hip_device)
        _run(fresh, src, first, c, cases.SIGMA * c)
        _run(fresh, [big_src], [big_dst], cases.C, cases.SIGMA * cases.C, [5], length)
        _run(fresh, src, again, c, cases.SIGMA * c)
        assert fresh.flags() == 0  # waits for the stream
    finally:
        fresh.close()
    for name, outs in (("first", first), ("again", again)):
        for t, (g, w) in enumerate(zip(outs, want_small)):
            _same(g.bytes(), w, 4, f"the small call ({name}), tensor {t}")
    _same(big_dst.bytes(), want_big, 4, f"{rows} rows")
    assert all(g.guards_intact() for g in src + first + again + [big_src, big_dst])
    assert [g.bytes() for g in src] == [cases.raw(x) for x in xs] and big_src.bytes() == cases.raw(big)


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("rows,length", [(5, 7), (7, 200)])
def test_rows_under_a_shift(ctx, hip_device, rows, length, dtype):
    """Row mode off 16 bytes. One element off, every group goes element by element; two elements off,
    the groups are shifted: a head group starts inside row 0, and with rows of 7 and of 200 elements
    nearly every group ends in another row than it started in. fp64 has groups of two: one element
    off is its only misalignment."""
    assert (rows, length) in cases.row_cases()
    x, want = cases.row_case(rows, length, dtype)
    places = [(1, 1)] if ref.group(dtype) == 2 else [(1, 1), (2, 2), (2, 0)]
    size = ref.ITEMSIZE[dtype]
    for in_off, out_off in places:
        src, dst = Guarded(x, hip_device, in_off), Guarded(torch.zeros_like(x), hip_device, out_off)
        _run(ctx, [src], [dst], cases.C, cases.SIGMA * cases.C, [5], length)
        assert ctx.flags() == 0
        _same(dst.bytes(), want, size, f"input {in_off} off, output {out_off} off")
        assert src.bytes() == cases.raw(x) and src.guards_intact() and dst.guards_intact(), (in_off, out_off)
        if in_off == out_off:
            _run(ctx, [src], [src], cases.C, cases.SIGMA * cases.C, [5], length)
            assert ctx.flags() == 0
            _same(src.bytes(), want, size, f"in place, {in_off} off")
            assert src.guards_intact()


@pytest.mark.parametrize("dtype", rounding.DTYPES)
def test_one_rounding_into_the_16_bit_types(ctx, hip_device, dtype):
    """The frozen rows whose fp64 ``o`` rounds to other bits through float32 than at once
    (tests/test_dp_host.py proves each), and the exact ties that go to even both ways."""
    for what, (x, want), c in (("sharp pairs", rounding.sharp_rows(dtype), rounding.SHARP_C),
                               ("exact ties", rounding.tie_rows(dtype), rounding.TIE_C)):
        src, dst = Guarded(x, hip_device), Guarded(torch.zeros_like(x), hip_device)
        _run(ctx, [src], [dst], c, 0.0, None, 2)
        assert ctx.flags() == 0
        _same(dst.bytes(), want, 2, what)
        _run(ctx, [src], [src], c, 0.0, None, 2)
        assert ctx.flags() == 0
        _same(src.bytes(), want, 2, f"{what}, in place")
        assert src.guards_intact() and dst.guards_intact()
