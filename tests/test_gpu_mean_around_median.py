"""The mean-around-median kernel (csrc/robust_kernels.hip, ``fedavg_mean_around_median``) on the
MI355X against the numpy restatement (tests/bulyan_reference.py). Tolerance: none —
every result is compared bit for bit, as integer views.

Sizes come from the build's own geometry (``fedavg_kernel_constant``): 1, one element short of a
16-byte vector, tile - 1 / tile / tile + 1, and a segment whose storage starts off a 16-byte
boundary. Client counts sit on both sides of every network width (2, 4, ..., 64); ``keep`` takes
both ends, their neighbours and the middle. Values are drawn from a small pool so that ties, signed
zeros, subnormals and infinities are frequent — which makes the window's start differ between the
lanes of one wave; a segment holds infinities of one sign only (both in a window would be the
result-NaN error, tested separately). No input asks the kernel to read past a tensor.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, NaNAggregationError, _native
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import OutputTable
from tests import bulyan_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
SENTINEL = 12345.0
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
COUNTS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]
# finite pool: zeros of both signs, ties, a subnormal of every input format (2^-24: fp16; 2^-130:
# fp32 / bf16; 2^-1030: fp64), large magnitudes; the segment's infinity is appended
POOL = [0.0, -0.0, 1.0, 1.0, -1.0, 1.5, 0.1, -7.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -130, -(2.0 ** -130),
        2.0 ** -1030, 6.0e4, -6.0e4, 3.0e38]
NP_OUT = {torch.float64: np.float64, torch.float32: np.float32}


def as_bits(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    t = np.ascontiguousarray(t)
    return t.view(np.int64 if t.dtype == np.float64 else np.int32)


def f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().to(torch.float64).numpy()


def draw(gen: torch.Generator, numel: int, dtype: torch.dtype, inf: float) -> torch.Tensor:
    # 3e38 would round to +inf in fp16, beside a segment's -inf
    finite = [6.0e4 if (dtype == torch.float16 and v == 3.0e38) else v for v in POOL]
    pool = torch.tensor(finite + [inf, inf], dtype=torch.float64)
    return pool[torch.randint(0, len(pool), (numel,), generator=gen)].to(dtype)


def edge_sizes(code: str) -> list[int]:
    tile = _native.kernel_constant("mam_tile")
    ae = _native.kernel_constant(f"mam_ae_{code}")
    return [1, ae - 1, tile - 1, tile, tile + 1, 2 * ae + 1]


def keeps_for(n: int) -> list[int]:
    return sorted({k for k in (1, 2, (n + 1) // 2, n - 1, n) if 1 <= k <= n})


def place(t: torch.Tensor, device, misalign: bool) -> torch.Tensor:
    """``t`` on the device; ``misalign``: as a contiguous view one element into a larger buffer, so
    its storage starts off a 16-byte boundary."""
    if not misalign:
        return t.to(device)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def test_constants_follow_the_robust_geometry():
    assert _native.kernel_constant("mam_tile") == _native.kernel_constant("robust_tile")
    assert _native.kernel_constant("mam_lanes") == 64
    for code in DTYPES:
        ae = _native.kernel_constant(f"mam_ae_{code}")
        assert ae * DTYPES[code].itemsize == 16 and _native.kernel_constant("mam_tile") % (64 * ae) == 0
    with pytest.raises(_native.NativeError):
        _native.kernel_constant("mam_nope")


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_kernel_matches_restatement(hip_device, code, n):
    dtype = DTYPES[code]
    sizes = edge_sizes(code)
    gen = torch.Generator().manual_seed(1000 * n + len(code))
    host = [[draw(gen, s, dtype, INF if t % 2 == 0 else -INF) for t, s in enumerate(sizes)] for _ in range(n)]
    cols = [[f64(row[i]) for row in host] for i in range(len(sizes))]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    last = len(sizes) - 1  # the last segment's storage is misaligned for every client
    table = ClientTable(len(sizes))
    for row in host:
        table.add_client([place(t, hip_device, i == last) for i, t in enumerate(row)], [1.0] * len(sizes))
    try:
        for keep in keeps_for(n):
            for out_dtype in (torch.float64, torch.float32):
                outs = [torch.full((s,), 123.0, dtype=out_dtype, device=hip_device) for s in sizes]
                ctx.mean_around_median(table, dtype, keep, outs, out_dtype)
                ctx.raise_on_nan([(table, dtype)])
                for i, o in enumerate(outs):
                    want = ref.mean_around_median(cols[i], keep, NP_OUT[out_dtype])
                    assert np.array_equal(as_bits(o), as_bits(want)), (keep, out_dtype, sizes[i])
    finally:
        ctx.close()


def test_window_start_at_both_ends_in_one_pass(hip_device):
    """n = 8, keep = 5, the lower median is s_3. Even elements hold four 10s below four far larger
    values: nothing lies closer than the 10s, the window starts at a = 0. Odd elements hold three
    far smaller values below five 10s: the window is the five 10s, a = n - keep = 3. Neighbouring
    lanes of every pass take opposite ends."""
    tile = _native.kernel_constant("mam_tile")
    n, keep, numel = 8, 5, tile + 6
    low = np.asarray([10.0, 10.0, 10.0, 10.0, 100.0, 200.0, 300.0, 400.0])
    high = np.asarray([-400.0, -300.0, -200.0, 10.0, 10.0, 10.0, 10.0, 10.0])
    rng = np.random.default_rng(1)
    x = np.empty((n, numel))
    for e in range(numel):
        x[:, e] = rng.permutation(low if e % 2 == 0 else high)
    s = ref.sort_total_order(x)
    assert ref.window_by_shrinking(s, keep).tolist() == [0 if e % 2 == 0 else n - keep for e in range(numel)]
    ctx = FedAvgContext(layout_of([numel]), hip_device)
    try:
        for dtype in (torch.float32, torch.float64, torch.bfloat16):
            table = ClientTable(1)
            for r in x:
                table.add_client([torch.from_numpy(r).to(dtype).to(hip_device)], [1.0])
            out = [torch.empty(numel, dtype=torch.float64, device=hip_device)]
            ctx.mean_around_median(table, dtype, keep, out)
            ctx.raise_on_nan()
            want = [(10.0 * 4 + 100.0) / 5.0 if e % 2 == 0 else 10.0 for e in range(numel)]
            assert out[0].cpu().tolist() == want
            assert np.array_equal(as_bits(out[0]), as_bits(ref.mean_around_median(list(x), keep)))
    finally:
        ctx.close()


def test_misaligned_output_and_many_tiles(hip_device):
    tile = _native.kernel_constant("mam_tile")
    sizes = [3 * tile + 5, 7]
    gen = torch.Generator().manual_seed(3)
    host = [[draw(gen, s, torch.float32, INF) for s in sizes] for _ in range(5)]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    table = ClientTable(2)
    for row in host:
        table.add_client([t.to(hip_device) for t in row], [1.0, 1.0])
    try:
        for out_dtype in (torch.float64, torch.float32):
            outs = [place(torch.zeros(s, dtype=out_dtype), hip_device, True) for s in sizes]
            ctx.mean_around_median(table, torch.float32, [3, 2], outs, out_dtype)
            ctx.raise_on_nan()
            for i, (o, keep) in enumerate(zip(outs, (3, 2))):
                want = ref.mean_around_median([f64(row[i]) for row in host], keep, NP_OUT[out_dtype])
                assert np.array_equal(as_bits(o), as_bits(want))
    finally:
        ctx.close()


def test_one_call_mixes_client_counts_and_keeps(hip_device):
    """Segments of one launch differ in n_t (absent entries, compacted away) and in keep[t]; the
    launch's network is the widest segment's."""
    tile = _native.kernel_constant("mam_tile")
    sizes = [tile + 9, 40, 3, 2 * tile]
    n = 33
    absent = {1: set(range(0, 33, 2)),        # 16 clients left
              2: set(range(1, 33)),           # one client left
              3: {5, 6, 7}}                   # 30 left
    keeps = [17, 16, 1, 7]
    gen = torch.Generator().manual_seed(41)
    host = [[draw(gen, s, torch.float16, -INF) for s in sizes] for _ in range(n)]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    table = ClientTable(len(sizes))
    for c, row in enumerate(host):
        table.add_client([None if c in absent.get(i, ()) else t.to(hip_device) for i, t in enumerate(row)],
                         [1.0] * len(sizes))
    outs = [torch.empty(s, dtype=torch.float64, device=hip_device) for s in sizes]
    try:
        ctx.mean_around_median(table, torch.float16, keeps, outs)
        ctx.raise_on_nan([(table, torch.float16)])
        for i, o in enumerate(outs):
            col = [f64(row[i]) for c, row in enumerate(host) if c not in absent.get(i, ())]
            assert np.array_equal(as_bits(o), as_bits(ref.mean_around_median(col, keeps[i]))), i
        with pytest.raises(ValueError, match="keep 17"):
            ctx.mean_around_median(table, torch.float16, [17, 17, 1, 7], outs)   # segment 1 has 16 clients
        with pytest.raises(ValueError, match="entries"):
            ctx.mean_around_median(table, torch.float16, [1, 1], outs)
    finally:
        ctx.close()


def neg_nan(dtype: torch.dtype) -> torch.Tensor:
    t = torch.tensor([float("nan")], dtype=dtype)
    t.view(torch.int64 if dtype == torch.float64 else torch.int32)[0] |= -(2 ** 63) if dtype == torch.float64 else -(2 ** 31)
    return t


@pytest.mark.parametrize("sign", ["+", "-"])
def test_nan_input_latches_the_input_flag(hip_device, sign):
    tile = _native.kernel_constant("mam_tile")
    numel = tile + 70
    for dtype in (torch.float32, torch.float64):
        gen = torch.Generator().manual_seed(5)
        host = [draw(gen, numel, dtype, INF) for _ in range(6)]
        host[4][tile + 65] = float("nan") if sign == "+" else neg_nan(dtype)[0]
        ctx = FedAvgContext(layout_of([numel]), hip_device)
        table = ClientTable(1)
        for t in host:
            table.add_client([t.to(hip_device)], [1.0])
        out = [torch.empty(numel, dtype=torch.float64, device=hip_device)]
        try:
            ctx.mean_around_median(table, dtype, 3, out)
            assert ctx.flags() & _native.FLAG_INPUT_NAN
            with pytest.raises(NaNAggregationError) as e:
                ctx.raise_on_nan([(table, dtype)])
            assert e.value.stage == "input" and e.value.bad_clients == [4]
            # the flag was cleared with the error: the context is usable
            host[4][tile + 65] = 1.0
            clean = ClientTable(1)
            for t in host:
                clean.add_client([t.to(hip_device)], [1.0])
            ctx.mean_around_median(clean, dtype, 3, out)
            assert ctx.flags() == 0
            assert np.array_equal(as_bits(out[0]), as_bits(ref.mean_around_median([f64(t) for t in host], 3)))
        finally:
            ctx.close()


def test_both_infinities_in_a_window_latch_the_result_flag(hip_device):
    rows = [torch.tensor(v, dtype=torch.float32) for v in
            ([1.0, INF, 2.0], [1.0, -INF, 2.0], [1.0, 0.0, 2.0], [3.0, INF, 2.0], [1.0, -INF, 5.0])]
    ctx = FedAvgContext(layout_of([3]), hip_device)
    table = ClientTable(1)
    for t in rows:
        table.add_client([t.to(hip_device)], [1.0])
    out = [torch.empty(3, dtype=torch.float64, device=hip_device)]
    try:
        ctx.mean_around_median(table, torch.float32, 5, out)         # every value kept: +inf + -inf
        assert ctx.flags() == _native.FLAG_RESULT_NAN
        with pytest.raises(ref.BulyanNaN) as r:
            ref.mean_around_median([f64(t) for t in rows], 5)
        assert r.value.stage == "result"
        with pytest.raises(NaNAggregationError) as e:
            ctx.raise_on_nan([(table, torch.float32)])
        assert e.value.stage == "result"
        # the median alone (0.0 in element 1) keeps no infinity, and the context is usable
        ctx.mean_around_median(table, torch.float32, 1, out)
        assert ctx.flags() == 0
        assert np.array_equal(as_bits(out[0]), as_bits(ref.mean_around_median([f64(t) for t in rows], 1)))
        assert out[0].cpu().tolist() == [1.0, 0.0, 2.0]
    finally:
        ctx.close()


def test_refusals_launch_nothing(hip_device):
    lib = _native.load()
    n, sizes = 65, [8, 3]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    dev = [[torch.ones(s, device=hip_device) for s in sizes] for _ in range(n)]
    outs_t = [torch.full((s,), SENTINEL, dtype=torch.float64, device=hip_device) for s in sizes]
    outs = (ctypes.c_void_p * 2)(*[o.data_ptr() for o in outs_t])
    PP = ctypes.POINTER(ctypes.c_void_p)

    def ptrs(count, hole=None, offset=0):
        flat = [t.data_ptr() + offset for row in dev[:count] for t in row]
        arr = (ctypes.c_void_p * len(flat))(*flat)
        if hole is not None:
            arr[hole] = None
        return ctypes.cast(arr, PP), arr

    def call(p, dtype, count, keep, out=outs, out_dtype=_native.F64):
        return lib.fedavg_mean_around_median(ctx._h, p, dtype, count, keep, out, out_dtype, ctx.stream)

    def keep_of(*ks):
        return (ctypes.c_int32 * len(ks))(*ks)

    try:
        p65, hold65 = ptrs(65)
        p5, hold5 = ptrs(5)
        assert call(p65, _native.F32, 65, keep_of(1, 1)) == _native.ERR_INVALID and "64" in _native.last_error()
        cases = [
            (p5, _native.F32, 5, keep_of(0, 1)),            # keep 0
            (p5, _native.F32, 5, keep_of(5, 6)),            # keep n + 1
            (p5, _native.F32, 5, None),                     # NULL keep
            (p5, _native.QSGD_F32, 5, keep_of(1, 1)),       # a record dtype
            (p5, 99, 5, keep_of(1, 1)),                     # no dtype at all
            (None, _native.F32, 5, keep_of(1, 1)),          # NULL table
            (p5, _native.F32, 0, keep_of(1, 1)),            # num_clients < 1
            (ptrs(5, offset=2)[0], _native.F32, 5, keep_of(1, 1)),   # not aligned to the element
        ]
        for args in cases:
            assert call(*args) == _native.ERR_INVALID and _native.last_error(), args[1:3]
        assert call(p5, _native.F32, 5, keep_of(1, 1), None) == _native.ERR_INVALID
        assert call(p5, _native.F32, 5, keep_of(1, 1), outs, _native.F16) == _native.ERR_INVALID
        # keep is checked against the segment's own count: client 4 did not send segment 1
        p_hole, hold_hole = ptrs(5, hole=4 * 2 + 1)
        assert call(p_hole, _native.F32, 5, keep_of(5, 5)) == _native.ERR_INVALID and "keep 5" in _native.last_error()
        # a segment no client sent
        one, hold_one = ptrs(1, hole=1)
        assert call(one, _native.F32, 1, keep_of(1, 1)) == _native.ERR_STATE and _native.last_error()
        # the Python surface refuses the same before the call
        table = ClientTable(2)
        for row in dev:
            table.add_client(row, [1.0, 1.0])
        with pytest.raises(NotImplementedError, match="64"):
            ctx.mean_around_median(table, torch.float32, 1, outs_t)
        torch.cuda.synchronize(hip_device)
        for o in outs_t:
            assert o.cpu().unique().tolist() == [SENTINEL]    # nothing was launched
        # and the valid call on the same context writes
        assert call(p_hole, _native.F32, 5, keep_of(5, 4)) == _native.OK, _native.last_error()
        assert ctx.flags() == 0
        assert all(o.cpu().unique().tolist() == [1.0] for o in outs_t)
        del hold65, hold5, hold_hole, hold_one
    finally:
        ctx.close()


def test_open_dynamic_wave_refuses_with_err_state(hip_device):
    layout = ModelLayout.flat(10_000)
    ctx = FedAvgContext(layout, hip_device)
    g = torch.Generator().manual_seed(6)
    host = [torch.randn(10_000, generator=g) for _ in range(7)]
    dev = [x.to(hip_device) for x in host]
    table = NativeClientTable(1, hip_device.index or 0)
    plain = ClientTable(1)
    for x in dev:
        table.add_client([x], [1.0])
        plain.add_client([x], [1.0])
    out = torch.empty(10_000, dtype=torch.float64, device=hip_device)
    outs = OutputTable([out], layout, hip_device, torch.float64)
    res = torch.full((10_000,), SENTINEL, dtype=torch.float64, device=hip_device)
    try:
        ctx.dyn_open(torch.float32, 16)
        with pytest.raises(_native.NativeError) as e:
            ctx.mean_around_median(plain, torch.float32, 3, [res])       # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        torch.cuda.current_stream(hip_device).synchronize()
        assert res.cpu().unique().tolist() == [SENTINEL]
        assert ctx.dyn_publish(table) == 7
        assert ctx.dyn_close(outs, torch.float64) == (7, True)
        ctx.raise_on_nan()
        ctx.mean_around_median(plain, torch.float32, 3, [res])           # and accepted once it is closed
        ctx.raise_on_nan()
        assert np.array_equal(as_bits(res), as_bits(ref.mean_around_median([f64(x) for x in host], 3)))
    finally:
        ctx.close()


def test_accumulator_is_not_touched(hip_device):
    """A round folded in two waves gives the same bits with ``mean_around_median`` called between
    the waves; the accumulator tensor itself and the total weights do not change."""
    tile = _native.kernel_constant("mam_tile")
    sizes, n = [tile + 1, 33, 3], 6
    weights = [float(k + 1) for k in range(n)]
    gen = torch.Generator().manual_seed(56)
    host = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(n)]
    dev = [[t.to(hip_device) for t in row] for row in host]

    def table_of(rows, ws):
        table = ClientTable(len(sizes))
        for row, w in zip(rows, ws):
            table.add_client(row, [w] * len(sizes))
        return table

    first, last, everyone = table_of(dev[:3], weights[:3]), table_of(dev[3:], weights[3:]), table_of(dev, weights)

    def fresh_outs():
        return [torch.full((s,), 123.0, dtype=torch.float64, device=hip_device) for s in sizes]

    plain = FedAvgContext(layout_of(sizes), hip_device)
    try:
        plain.accumulate(first, torch.float32)
        want = fresh_outs()
        plain.aggregate(last, torch.float32, want, torch.float64)
        plain.raise_on_nan()
    finally:
        plain.close()
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        ctx.accumulate(first, torch.float32)
        assert ctx.flags() == 0                      # synchronises
        acc_before, totals_before = ctx.accumulator.clone(), ctx.total_weights()
        assert bool((acc_before != 0).any())
        mam = fresh_outs()
        ctx.mean_around_median(everyone, torch.float32, 4, mam)
        assert ctx.flags() == 0
        assert np.array_equal(as_bits(ctx.accumulator), as_bits(acc_before))
        assert ctx.total_weights() == totals_before
        got = fresh_outs()
        ctx.aggregate(last, torch.float32, got, torch.float64)
        ctx.raise_on_nan()
    finally:
        ctx.close()
    for g, w in zip(got, want):
        assert np.array_equal(as_bits(g), as_bits(w))
    for i, m in enumerate(mam):
        assert np.array_equal(as_bits(m), as_bits(ref.mean_around_median([f64(row[i]) for row in host], 4)))
