"""The fold about a point (csrc/clip_kernels.hip, ``fedavg_fold_about_point``) against DESIGN.md
§5j: bit for bit against the numpy restatement (``tests/clip_reference.fold_about_point``) through
``FedAvgContext.fold_about_point`` and through the C call; that an element's result depends on
nothing but its own values, the coefficients and the divisor; signed zeros; the three NaN flags; and
the refusals before any launch.

Client values are ``geomed_reference.order_sensitive_values`` (representable in the client format,
spread over binades) beside an N(0, 1) float64 point and coefficients between 0 and 3: every
difference, product and sum rounds. Sizes come from the build's own geometry
(``fedavg_kernel_constant``). A context holds no empty segment (the plugin class takes empty tensors
out before it builds one: tests/test_gpu_clip.py runs that layout). No input asks the kernel to read
or write past a tensor: every pointer is a whole torch tensor or a view that ends inside its buffer,
and the elements around an output view are checked to be untouched.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, _native
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import OutputTable
from distributed_learning_simulation_lib_amd.quantized import QSGD_F32
from tests import clip_reference as ref
from tests import geomed_reference as geo

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
SENTINEL = 12345.0
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
OUT_DTYPES = (torch.float64, torch.float32)
COUNTS = [1, 2, 9, 65]


def constant(name: str) -> int:
    return _native.kernel_constant(name)


def np_out(dtype: torch.dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def bits(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def assert_same_bits(got, want, what="") -> None:
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if not np.array_equal(g, w):
        at = int(np.argwhere(g != w)[0][0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} elements differ in bits; first at {at}: "
                             f"got {np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got).reshape(-1)[at]!r}, "
                             f"want {np.asarray(want).reshape(-1)[at]!r}")


def place(t: torch.Tensor, device, misalign: bool) -> torch.Tensor:
    """``t`` on the device; ``misalign``: a contiguous view one element into a larger buffer."""
    if not misalign:
        v = t.to(device)
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


class Outs:
    """One output view per segment inside a sentinel-filled buffer, with guard elements before it
    (16 bytes of them, or with ``misalign`` one element: the view then starts off a 16-byte
    boundary) and one after it; the guards are checked after the call."""

    def __init__(self, sizes, dtype, device, misalign: bool) -> None:
        per16 = 16 // dtype.itemsize
        lead = 1 if misalign else per16
        self.bufs = [torch.full((lead + s + 1,), SENTINEL, dtype=dtype, device=device) for s in sizes]
        self.views = [b[lead:lead + s] for b, s in zip(self.bufs, sizes)]
        self.lead = lead
        for v in self.views:
            assert (v.data_ptr() % 16 != 0) == misalign

    def guards_untouched(self) -> bool:
        return all(bool((b[:self.lead] == SENTINEL).all()) and b[-1].item() == SENTINEL for b in self.bufs)

    def untouched(self) -> bool:
        return all(bool((b == SENTINEL).all()) for b in self.bufs)


def table_of(dev_rows) -> ClientTable:
    T = len(dev_rows[0])
    table = ClientTable(T)
    for row in dev_rows:
        table.add_client(row, [1.0] * T)
    return table


def fold_once(device, dev_rows, dtype, sizes, coef, divisor, point, out_dtype, misalign_out=False, want_flags=0):
    ctx = FedAvgContext(layout_of(sizes), device)
    try:
        outs = Outs(sizes, out_dtype, device, misalign_out)
        ctx.fold_about_point(table_of(dev_rows), dtype, coef, divisor, point, outs.views, out_dtype)
        assert ctx.flags() == want_flags
        assert outs.guards_untouched()
        return [v.cpu().numpy() for v in outs.views]
    finally:
        ctx.close()


def coefficients(n: int, seed: int = 0) -> list[float]:
    """Between 0 and 3, some above 1; where there is room one exact 0.0 and one exact 1.0."""
    gen = torch.Generator().manual_seed(100 + n + seed)
    c = (3.0 * torch.rand(n, generator=gen, dtype=torch.float64)).tolist()
    if n >= 3:
        c[1], c[2] = 0.0, 1.0
    assert n < 3 or (0.0 in c and max(c) > 1.0)
    return c


# ---- 1. bit for bit against the restatement ----------------------------------------------------
def sizes_for() -> list[int]:
    return [constant("clip_tile") + 3, 5, 3 * 7, 1]


@functools.lru_cache(maxsize=None)
def case(code: str):
    """The largest client count's rows and a float64 point; every smaller count reads the leading
    rows. Computed once, left unchanged."""
    sizes = sizes_for()
    gen = torch.Generator().manual_seed(7000 + len(code) + ord(code[1]))
    rows = [[geo.order_sensitive_values(gen, s, DTYPES[code]) for s in sizes] for _ in range(max(COUNTS))]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    return sizes, rows, point


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_fold_equals_the_restatement(hip_device, code, n):
    dtype = DTYPES[code]
    sizes, rows, point = case(code)
    rows = rows[:n]
    coef = coefficients(n)
    divisor = 0.7 * n + 0.3
    # aligned: the vector paths; misaligned: client segment 0 (more than one tile) and segment 2 one
    # element into their buffers, the point's segment 0 only 8-byte aligned, every output one element in
    for misalign in (False, True):
        dev = [[place(t.to(dtype), hip_device, misalign and i in (0, 2)) for i, t in enumerate(r)] for r in rows]
        z = [place(p, hip_device, misalign and i == 0) for i, p in enumerate(point)]
        for out_dtype in OUT_DTYPES:
            want, flags = ref.fold_about_point(rows, coef, divisor, point, np_out(out_dtype))
            assert flags == 0
            got = fold_once(hip_device, dev, dtype, sizes, coef, divisor, z, out_dtype, misalign_out=misalign)
            for t, (g, w) in enumerate(zip(got, want)):
                assert_same_bits(g, w, f"{code} n={n} out={out_dtype} misaligned={misalign} segment {t}")


def test_1024_clients_of_8_elements(hip_device):
    n = _native.POINT_MAX_CLIENTS
    assert n == constant("clip_max_clients") == 1024
    gen = torch.Generator().manual_seed(5)
    rows = [[geo.order_sensitive_values(gen, 8, torch.float32)] for _ in range(n)]
    point = [torch.randn(8, generator=gen, dtype=torch.float64)]
    coef = coefficients(n)
    dev = [[t.to(torch.float32).to(hip_device) for t in r] for r in rows]
    want, _ = ref.fold_about_point(rows, coef, 1000.0, point)
    got = fold_once(hip_device, dev, torch.float32, [8], coef, 1000.0, [point[0].to(hip_device)], torch.float64)
    assert_same_bits(got[0], want[0], "1024 clients")


def test_signed_zeros(hip_device):
    """z = -0.0 with every x = -0.0: d = +0.0; positive coefficients give +0.0 products and
    -0.0 + +0.0 = +0.0; negative ones give -0.0 products whose sum stays -0.0 because no 0 + leads
    it, and -0.0 + -0.0 = -0.0."""
    sizes = [constant("clip_tile") + 3, 5]
    rows = [[torch.full((s,), -0.0, dtype=torch.float32) for s in sizes] for _ in range(3)]
    point = [torch.full((s,), -0.0, dtype=torch.float64) for s in sizes]
    dev = [[t.to(hip_device) for t in r] for r in rows]
    z = [p.to(hip_device) for p in point]
    for coef, sign in (([1.0, 0.5, 2.0], 1.0), ([-1.0, -0.5, -2.0], -1.0)):
        for out_dtype in OUT_DTYPES:
            want, _ = ref.fold_about_point(rows, coef, 3.0, point, np_out(out_dtype))
            got = fold_once(hip_device, dev, torch.float32, sizes, coef, 3.0, z, out_dtype)
            for g, w in zip(got, want):
                assert_same_bits(g, w, f"signed zeros {coef}")
                assert (g == 0).all() and (np.copysign(1.0, g) == sign).all()


# ---- 2. an element's result depends on nothing else ----------------------------------------------
def test_result_is_independent_of_earlier_calls_and_of_the_other_tensors(hip_device):
    code, dtype = "f32", torch.float32
    sizes, rows, point = case(code)
    n = 9
    rows = rows[:n]
    coef = coefficients(n)
    dev = [[t.to(dtype).to(hip_device) for t in r] for r in rows]
    z = [p.to(hip_device) for p in point]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        def run(table_rows, c, div, pt):
            outs = [torch.full((s,), SENTINEL, dtype=torch.float64, device=hip_device) for s in sizes]
            ctx.fold_about_point(table_of(table_rows), dtype, c, div, pt, outs)
            return [o.cpu().numpy() for o in outs]

        first = run(dev, coef, 4.0, z)
        run(dev[:2], [5.0, -1.0], 0.5, [p * 3.0 for p in z])          # another table, point and divisor
        ctx.aggregate(table_of(dev), dtype, [torch.empty(s, dtype=torch.float64, device=hip_device) for s in sizes],
                      torch.float64)                                # the fold's accumulator state
        again = run(dev, coef, 4.0, z)
        assert ctx.flags() == 0
        for a, b in zip(first, again):
            assert_same_bits(a, b, "two calls on one context")
    finally:
        ctx.close()
    # every tensor alone in a layout of its own (other tiles, other segment numbers)
    for t, s in enumerate(sizes):
        alone = fold_once(hip_device, [[r[t]] for r in dev], dtype, [s], coef, 4.0, [z[t]], torch.float64)
        assert_same_bits(alone[0], first[t], f"segment {t} alone")


# ---- 3. the flags ---------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan_client", "nan_point", "inf_point_times_zero", "inf_minus_inf", "result_only"])
def test_nan_flags(hip_device, what):
    tile = constant("clip_tile")
    sizes = [tile + 3, 5]
    gen = torch.Generator().manual_seed(8)
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64).to(torch.float32) for s in sizes] for _ in range(4)]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    coef = [1.0, 0.5, 2.0, 1.5]
    I, A, R = _native.FLAG_INPUT_NAN, _native.FLAG_ACC_NAN, _native.FLAG_RESULT_NAN
    at = tile + 2                                    # the guarded tail of the second tile
    if what == "nan_client":
        rows[2][0][at] = NAN
        want_flags = I | A | R
    elif what == "nan_point":
        point[1][3] = NAN
        want_flags, at = I | A | R, None
    elif what == "inf_point_times_zero":             # every distance is +inf, every coefficient 0: 0 * inf
        point[0][at] = INF
        coef = [0.0] * 4
        want_flags = A | R
    elif what == "inf_minus_inf":
        rows[0][0][at] = INF
        rows[3][0][at] = -INF
        want_flags = A | R
    else:                                            # acc = +inf is no NaN; -inf + inf is
        point[0][at] = -INF
        want_flags = R
    want, ref_flags = ref.fold_about_point(rows, coef, 4.0, point)
    assert (I, A, R) == (ref.FLAG_INPUT, ref.FLAG_ACC, ref.FLAG_RESULT) and ref_flags == want_flags
    dev = [[t.to(hip_device) for t in r] for r in rows]
    got = fold_once(hip_device, dev, torch.float32, sizes, coef, 4.0, [p.to(hip_device) for p in point],
                    torch.float64, want_flags=want_flags)
    for t, (g, w) in enumerate(zip(got, want)):     # NaN payloads aside, the same values everywhere
        assert np.array_equal(np.isnan(g), np.isnan(w)), t
        assert_same_bits(g[~np.isnan(g)], w[~np.isnan(w)], f"{what}: the elements beside the NaN, segment {t}")
    if at is not None:
        assert np.isnan(got[0][at]) and int(np.isnan(got[0]).sum()) == 1 and not np.isnan(got[1]).any()


# ---- 4. refusals before any launch ----------------------------------------------------------------
def test_c_abi_direct_call_and_refusals(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 5
    gen = torch.Generator().manual_seed(23)
    host = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(n)]
    zhost = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    dev = [[t.to(hip_device) for t in row] for row in host]
    zdev = [z.to(hip_device) for z in zhost]
    coef = [1.0, 0.0, 2.5, 0.25, 1.0]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        D = ctypes.c_double
        ptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        zptrs = (ctypes.c_void_p * 2)(*[z.data_ptr() for z in zdev])
        cs = (D * n)(*coef)
        outs = [torch.full((s,), SENTINEL, dtype=torch.float64, device=hip_device) for s in sizes]
        optrs = (ctypes.c_void_p * 2)(*[o.data_ptr() for o in outs])
        stream = ctypes.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)
        call = lib.fedavg_fold_about_point
        F32, F64 = _native.F32, _native.F64
        totals = (D * 2)()
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK
        before = bytes(totals)
        assert call(ctx, ptrs, F32, cs, n, 5.0, zptrs, optrs, F64, stream) == _native.OK, _native.last_error()
        flags = ctypes.c_uint32(99)
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        want, _ = ref.fold_about_point(host, coef, 5.0, zhost)
        for o, w in zip(outs, want):
            assert_same_bits(o, w, "C ABI")
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK and bytes(totals) == before   # state untouched
        # refused before any launch, each with a message
        for o in outs:
            o.fill_(SENTINEL)
        cap = _native.POINT_MAX_CLIENTS
        holed = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        holed[2 * 2 + 1] = None
        many = (ctypes.c_void_p * ((cap + 1) * 2))(*([dev[0][0].data_ptr(), dev[0][1].data_ptr()] * (cap + 1)))
        many_cs = (D * (cap + 1))(*([1.0] * (cap + 1)))
        odd = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        odd[0] = dev[0][0].data_ptr() + 2
        zholed = (ctypes.c_void_p * 2)(zdev[0].data_ptr(), None)
        zodd = (ctypes.c_void_p * 2)(zdev[0].data_ptr() + 4, zdev[1].data_ptr())
        oholed = (ctypes.c_void_p * 2)(outs[0].data_ptr(), None)
        oodd = (ctypes.c_void_p * 2)(outs[0].data_ptr() + 4, outs[1].data_ptr())
        inplace = (ctypes.c_void_p * 2)(outs[0].data_ptr(), zdev[1].data_ptr())
        cs_nan, cs_inf = (D * n)(1.0, NAN, 1.0, 1.0, 1.0), (D * n)(1.0, 1.0, 1.0, -INF, 1.0)
        for args in ((holed, F32, cs, n, 5.0, zptrs, optrs, F64), (many, F32, many_cs, cap + 1, 5.0, zptrs, optrs, F64),
                     (ptrs, _native.QSGD_F32, cs, n, 5.0, zptrs, optrs, F64), (ptrs, 99, cs, n, 5.0, zptrs, optrs, F64),
                     (ptrs, F32, cs, n, 5.0, zptrs, optrs, _native.F16), (ptrs, F32, cs, n, 5.0, zptrs, optrs, 99),
                     (None, F32, cs, n, 5.0, zptrs, optrs, F64), (ptrs, F32, None, n, 5.0, zptrs, optrs, F64),
                     (ptrs, F32, cs, n, 5.0, None, optrs, F64), (ptrs, F32, cs, n, 5.0, zptrs, None, F64),
                     (ptrs, F32, cs, 0, 5.0, zptrs, optrs, F64), (ptrs, F32, cs, -1, 5.0, zptrs, optrs, F64),
                     (odd, F32, cs, n, 5.0, zptrs, optrs, F64), (ptrs, F32, cs, n, 5.0, zholed, optrs, F64),
                     (ptrs, F32, cs, n, 5.0, zodd, optrs, F64), (ptrs, F32, cs, n, 5.0, zptrs, oholed, F64),
                     (ptrs, F32, cs, n, 5.0, zptrs, oodd, F64), (ptrs, F32, cs, n, 5.0, zptrs, inplace, F64),
                     (ptrs, F32, cs_nan, n, 5.0, zptrs, optrs, F64), (ptrs, F32, cs_inf, n, 5.0, zptrs, optrs, F64),
                     (ptrs, F32, cs, n, 0.0, zptrs, optrs, F64), (ptrs, F32, cs, n, -1.0, zptrs, optrs, F64),
                     (ptrs, F32, cs, n, INF, zptrs, optrs, F64), (ptrs, F32, cs, n, NAN, zptrs, optrs, F64)):
            assert call(ctx, *args, stream) == _native.ERR_INVALID, args
            assert _native.last_error()
        assert call(None, ptrs, F32, cs, n, 5.0, zptrs, optrs, F64, stream) == _native.ERR_INVALID
        torch.cuda.synchronize(hip_device)
        assert all(o.cpu().unique().tolist() == [SENTINEL] for o in outs)   # nothing was launched
        assert zdev[1].cpu().tolist() == zhost[1].tolist()                 # the in-place point is unchanged
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_python_refusals_without_a_launch(hip_device):
    sizes = [40, 3]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    x = [torch.ones(s, device=hip_device) for s in sizes]
    z = [torch.zeros(s, dtype=torch.float64, device=hip_device) for s in sizes]
    outs = Outs(sizes, torch.float64, hip_device, False)
    o = outs.views
    try:
        with pytest.raises(ValueError, match="no clients"):
            ctx.fold_about_point(ClientTable(2), torch.float32, [], 1.0, z, o)
        holed = ClientTable(2)
        holed.add_client(x, [1.0, 1.0])
        holed.add_client([x[0], None], [1.0, 1.0])
        with pytest.raises(ValueError, match="client 1 lacks tensor 1"):
            ctx.fold_about_point(holed, torch.float32, [1.0, 1.0], 1.0, z, o)
        with pytest.raises(NotImplementedError, match="dequantise"):
            ctx.fold_about_point(holed, QSGD_F32, [1.0, 1.0], 1.0, z, o)
        many = ClientTable(2)
        for _ in range(_native.POINT_MAX_CLIENTS + 1):
            many.add_client(x, [1.0, 1.0])
        with pytest.raises(NotImplementedError, match=str(_native.POINT_MAX_CLIENTS)):
            ctx.fold_about_point(many, torch.float32, [1.0] * (_native.POINT_MAX_CLIENTS + 1), 1.0, z, o)
        table = table_of([x, x])
        for coef in ([1.0], [1.0, NAN], [INF, 1.0]):
            with pytest.raises(ValueError, match="coefficient"):
                ctx.fold_about_point(table, torch.float32, coef, 1.0, z, o)
        for div in (0.0, -2.0, INF, NAN):
            with pytest.raises(ValueError, match="divisor"):
                ctx.fold_about_point(table, torch.float32, [1.0, 1.0], div, z, o)
        with pytest.raises(TypeError):
            ctx.fold_about_point(table, torch.float32, [1.0, 1.0], 1.0, z, o, torch.float16)
        for bad in ([z[0]], [z[0], z[1].float()], [z[0], z[1].cpu()],
                    [z[0], torch.zeros(4, dtype=torch.float64, device=hip_device)]):
            with pytest.raises(ValueError, match="point"):
                ctx.fold_about_point(table, torch.float32, [1.0, 1.0], 1.0, bad, o)
        for bad in ([o[0]], [o[0], o[1].float()], [o[0], torch.zeros(4, dtype=torch.float64, device=hip_device)]):
            with pytest.raises(ValueError, match="output"):
                ctx.fold_about_point(table, torch.float32, [1.0, 1.0], 1.0, z, bad)
        with pytest.raises(ValueError, match="in-place"):
            ctx.fold_about_point(table, torch.float32, [1.0, 1.0], 1.0, z, [o[0], z[1]])
        torch.cuda.synchronize(hip_device)
        assert outs.untouched() and ctx.flags() == 0
        ctx.fold_about_point(table, torch.float32, [1.0, 0.5], 3.0, z, o)     # 0 + (1 * 1 + 0.5 * 1) / 3
        assert ctx.flags() == 0 and all(v.cpu().unique().tolist() == [0.5] for v in o) and outs.guards_untouched()
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
    zhost = torch.randn(10_000, generator=g, dtype=torch.float64)
    z = zhost.to(hip_device)
    res = torch.full((10_000,), SENTINEL, dtype=torch.float64, device=hip_device)
    coef = coefficients(7)
    try:
        ctx.dyn_open(torch.float32, 16)
        with pytest.raises(_native.NativeError) as e:
            ctx.fold_about_point(plain, torch.float32, coef, 7.0, [z], [res])   # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        torch.cuda.current_stream(hip_device).synchronize()
        assert res.cpu().unique().tolist() == [SENTINEL]
        assert ctx.dyn_publish(table) == 7
        assert ctx.dyn_close(outs, torch.float64) == (7, True)
        ctx.raise_on_nan()
        ctx.fold_about_point(plain, torch.float32, coef, 7.0, [z], [res])       # and accepted once it is closed
        ctx.raise_on_nan()
        want, _ = ref.fold_about_point([[x] for x in host], coef, 7.0, [zhost])
        assert_same_bits(res, want[0], "after the wave has closed")
    finally:
        ctx.close()
