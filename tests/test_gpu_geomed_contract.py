"""The point-distance kernel (csrc/point_kernels.hip, ``fedavg_sqdist_to_point``) against DESIGN.md
§5i: the pinned summation order, bit for bit against the numpy restatement
(``tests/geomed_reference.distances_in_order``); the error bound against rational arithmetic; that a
client's entry depends on nothing but its own values, the point and the layout; the NaN / infinity
flags; and the refusals before any launch.

The order inputs are ``ref.order_sensitive_values`` (representable in the client format, squares
spread over more than 53 bits) and an N(0, 1) float64 point: every difference, square and sum rounds, so
another order gives other bits (tests/test_geomed_host.py shows that on the same generator).
Sizes come from the build's own geometry (``fedavg_kernel_constant``). No input asks the kernel to
read past a tensor: every pointer is a whole torch tensor or a view that ends inside its buffer.
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
from tests import geomed_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def constant(name: str) -> int:
    return _native.kernel_constant(name)


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    return ref.native_constants(_native.kernel_constant)


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def f64_bits(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def place(t: torch.Tensor, device, misalign: bool) -> torch.Tensor:
    """``t`` on the device; ``misalign``: a contiguous view one element into a larger buffer, so its
    storage starts off a 16-byte boundary (8 bytes off for float64: the point's guarded path)."""
    if not misalign:
        v = t.to(device)
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def on_device(device, rows, dtype, misalign_last=True):
    last = len(rows[0]) - 1
    return [[place(t.to(dtype), device, misalign_last and i == last) for i, t in enumerate(row)] for row in rows]


def point_on_device(device, point, misalign_middle=True):
    """The middle segment's point tensor 8 but not 16 bytes aligned."""
    return [place(z, device, misalign_middle and i == 1) for i, z in enumerate(point)]


def table_of(dev_rows) -> ClientTable:
    T = len(dev_rows[0])
    table = ClientTable(T)
    for row in dev_rows:
        table.add_client(row, [1.0] * T)
    return table


def distances_once(device, dev_rows, dtype, sizes, point=None, want_flags=0) -> np.ndarray:
    ctx = FedAvgContext(layout_of(sizes), device)
    try:
        D = ctx.sqdist_to_point(table_of(dev_rows), dtype, point)
        assert D.dtype == torch.float64 and D.shape == (len(dev_rows),) and D.device == device
        assert ctx.flags() == want_flags
        return D.cpu().numpy()
    finally:
        ctx.close()


def assert_same_bits(got, want, what="") -> None:
    g, w = f64_bits(got), f64_bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        at = int(np.argwhere(g != w)[0][0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} entries differ in bits; first at {at}: "
                             f"got {np.asarray(got)[at]!r}, want {np.asarray(want)[at]!r}")


# ---- 1. the pinned order ----------------------------------------------------------------------
def order_layouts(code: str) -> list[list[int]]:
    """Three segments each; between them 1, ae - 1, chunk - 1, chunk, chunk + 1 and 2 * chunk + 3."""
    chunk, ae = constant("point_chunk"), constant(f"point_ae_{code}")
    return [[1, chunk - 1, 2 * chunk + 3], [ae - 1, chunk, chunk + 1]]


def client_counts() -> list[int]:
    return [1, 2, 3, constant("point_batch") + 1]   # the last one crosses the kernel's client batch


@functools.lru_cache(maxsize=None)
def order_case(code: str, which: int):
    """The largest client count's rows (float64 values every format holds), a float64 point and the
    restatement's distances to the origin and to the point. A client's entry does not depend on the
    other clients, so every smaller count reads the leading rows. Computed once, left unchanged."""
    sizes = order_layouts(code)[which]
    n = max(client_counts())
    gen = torch.Generator().manual_seed(9000 + 10 * which + len(code))
    rows = [[ref.order_sensitive_values(gen, s, DTYPES[code]) for s in sizes] for _ in range(n)]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    c = constants()
    return sizes, rows, point, ref.distances_in_order(rows, None, c, code), ref.distances_in_order(rows, point, c, code)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 2, 3], ids=lambda i: f"count{i}")
@pytest.mark.parametrize("code", list(DTYPES))
def test_distances_follow_the_pinned_order(hip_device, code, n, which):
    n = client_counts()[n]
    dtype = DTYPES[code]
    sizes, rows, point, want_origin, want_point = order_case(code, which)
    rows = rows[:n]
    assert all(torch.equal(t.to(dtype).to(torch.float64), t) for r in rows for t in r)   # representable
    dev = on_device(hip_device, rows, dtype)                # the last segment's storage is misaligned
    assert_same_bits(distances_once(hip_device, dev, dtype, sizes), want_origin[:n], f"origin {code} n={n} {sizes}")
    z = point_on_device(hip_device, point)                  # the middle segment 8-byte aligned only
    assert z[1].data_ptr() % 16 == 8
    assert_same_bits(distances_once(hip_device, dev, dtype, sizes, z), want_point[:n], f"point {code} n={n} {sizes}")
    # the vector paths: everything 16-byte aligned
    dev = on_device(hip_device, rows, dtype, misalign_last=False)
    z = point_on_device(hip_device, point, misalign_middle=False)
    assert_same_bits(distances_once(hip_device, dev, dtype, sizes, z), want_point[:n], f"aligned {code} n={n} {sizes}")


# ---- 2. the error bound -------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(DTYPES))
def test_error_bound_against_rationals(hip_device, code):
    dtype = DTYPES[code]
    sizes = [1500, 7, 1493]
    P = sum(sizes)
    gen = torch.Generator().manual_seed(31)
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in sizes] for _ in range(3)]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    dev = on_device(hip_device, rows, dtype)
    for z_host in (None, point):
        z = None if z_host is None else point_on_device(hip_device, z_host)
        got = distances_once(hip_device, dev, dtype, sizes, z)
        for g, r in zip(got.tolist(), rows):
            exact = ref.exact_distance(r, z_host)
            rel = abs(ref.Fraction(g) - exact) / exact
            print(f"{code} {'origin' if z_host is None else 'point'}: relative error {float(rel):.3e}, "
                  f"bound {(P + 2) * 2.0 ** -53:.3e}")
            assert rel <= ref.Fraction(P + 2, 2 ** 53)


# ---- 3. a client's entry depends on nothing else ------------------------------------------------
def test_entry_is_independent_of_the_table_and_of_earlier_calls(hip_device):
    code, dtype = "f32", torch.float32
    chunk, batch = constant("point_chunk"), constant("point_batch")
    sizes = [chunk + 5, 3, 2 * chunk + 1]
    n = batch + 3
    gen = torch.Generator().manual_seed(77)
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in sizes] for _ in range(n)]
    point = point_on_device(hip_device, [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes])
    dev = on_device(hip_device, rows, dtype)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        i = 2
        alone = ctx.sqdist_to_point(table_of([dev[i]]), dtype, point).cpu().numpy()      # the workspace holds 1 client
        small = ctx.sqdist_to_point(table_of(dev[:5]), dtype, point).cpu().numpy()        # grown
        full = ctx.sqdist_to_point(table_of(dev), dtype, point).cpu().numpy()             # grown again
        again = ctx.sqdist_to_point(table_of(dev), dtype, point).cpu().numpy()
        moved = ctx.sqdist_to_point(table_of(dev[batch:] + dev[:batch]), dtype, point).cpu().numpy()  # other rows
        after = ctx.sqdist_to_point(table_of([dev[i]]), dtype, point).cpu().numpy()       # after the growth
        assert ctx.flags() == 0
        assert_same_bits(again, full, "two calls on one context")
        assert_same_bits(alone, full[i:i + 1], "alone against a table of n")
        assert_same_bits(small, full[:5], "a table of 5 against a table of n")
        assert_same_bits(after, alone, "after the workspace has grown")
        assert_same_bits(moved, np.concatenate([full[batch:], full[:batch]]), "at another row")
    finally:
        ctx.close()
    assert_same_bits(distances_once(hip_device, dev, dtype, sizes, point), full, "another context")


# ---- 4. NaN and infinities -------------------------------------------------------------------
def flag_rows(gen, sizes, n=4):
    return [[torch.randn(s, generator=gen, dtype=torch.float64).to(torch.float32) for s in sizes] for _ in range(n)]


@pytest.mark.parametrize("where", ["first", "tail", "misaligned"])
def test_nan_latches_the_input_flag(hip_device, where):
    chunk = constant("point_chunk")
    sizes = [chunk + 3, 5, 2 * chunk + 1]
    seg, pos = {"first": (0, 0), "tail": (0, chunk + 2), "misaligned": (2, 2 * chunk)}[where]
    gen = torch.Generator().manual_seed(5)
    rows = flag_rows(gen, sizes)
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    bad = [[t.clone() for t in r] for r in rows]
    bad[1][seg][pos] = float("nan")
    dev = on_device(hip_device, bad, torch.float32)
    for z in (None, point_on_device(hip_device, point)):
        D = distances_once(hip_device, dev, torch.float32, sizes, z,
                           want_flags=_native.FLAG_INPUT_NAN | _native.FLAG_ACC_NAN)
        assert np.isnan(D[1]) and np.isfinite(np.delete(D, 1)).all()
    # a NaN in the point: the input flag too
    zbad = [z.clone() for z in point]
    zbad[1 if where == "first" else seg][min(pos, 4) if where == "first" else pos] = float("nan")
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        ctx.sqdist_to_point(table_of(on_device(hip_device, rows, torch.float32)), torch.float32,
                            point_on_device(hip_device, zbad))
        assert ctx.flags() & _native.FLAG_INPUT_NAN
    finally:
        ctx.close()


def test_infinities(hip_device):
    chunk = constant("point_chunk")
    sizes = [chunk + 3, 5, 2 * chunk + 1]
    gen = torch.Generator().manual_seed(6)
    rows = flag_rows(gen, sizes)
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    want = ref.distances_in_order(rows, point, constants(), "f32")
    rows[0][0][chunk + 1] = INF
    rows[2][2][7] = -INF
    dev = on_device(hip_device, rows, torch.float32)
    for z_host in (None, point):
        z = None if z_host is None else point_on_device(hip_device, z_host)
        D = distances_once(hip_device, dev, torch.float32, sizes, z)      # no flag
        assert D[0] == INF and D[2] == INF and np.isfinite(D[[1, 3]]).all()
        if z_host is not None:
            assert_same_bits(D[[1, 3]], want[[1, 3]], "the finite clients beside the infinite ones")
    # an infinite point element against the same infinity: inf - inf
    zinf = [z.clone() for z in point]
    zinf[0][chunk + 1] = INF
    D = distances_once(hip_device, dev, torch.float32, sizes, point_on_device(hip_device, zinf),
                       want_flags=_native.FLAG_ACC_NAN)
    assert np.isnan(D[0]) and (D[1:] == INF).all()


# ---- 5. refusals before any launch ----------------------------------------------------------------
def test_c_abi_direct_call_and_refusals(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 5
    gen = torch.Generator().manual_seed(23)
    host = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(n)]
    zhost = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    dev = [[t.to(hip_device) for t in row] for row in host]
    zdev = [z.to(hip_device) for z in zhost]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        ptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        zptrs = (ctypes.c_void_p * 2)(*[z.data_ptr() for z in zdev])
        out = torch.full((n,), 123.0, dtype=torch.float64, device=hip_device)
        optr = ctypes.c_void_p(out.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)
        call = lib.fedavg_sqdist_to_point
        assert call(ctx, ptrs, _native.F32, n, zptrs, optr, stream) == _native.OK, _native.last_error()
        flags = ctypes.c_uint32(99)
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        assert_same_bits(out, ref.distances_in_order(host, zhost, constants(), "f32"), "C ABI, point")
        assert call(ctx, ptrs, _native.F32, n, None, optr, stream) == _native.OK, _native.last_error()
        assert lib.fedavg_check(ctx, stream, None) == _native.OK
        assert_same_bits(out, ref.distances_in_order(host, None, constants(), "f32"), "C ABI, origin")
        # refused before any launch, each with a message
        out.fill_(5.0)
        holed = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        holed[2 * 2 + 1] = None
        cap = _native.POINT_MAX_CLIENTS
        assert cap == constant("point_max_clients")
        many = (ctypes.c_void_p * ((cap + 1) * 2))(*([dev[0][0].data_ptr(), dev[0][1].data_ptr()] * (cap + 1)))
        zholed = (ctypes.c_void_p * 2)(zdev[0].data_ptr(), None)
        zodd = (ctypes.c_void_p * 2)(zdev[0].data_ptr() + 4, zdev[1].data_ptr())
        odd = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        odd[0] = dev[0][0].data_ptr() + 2
        for args in ((holed, _native.F32, n, zptrs, optr), (many, _native.F32, cap + 1, zptrs, optr),
                     (ptrs, _native.QSGD_F32, n, zptrs, optr), (ptrs, 99, n, zptrs, optr),
                     (None, _native.F32, n, zptrs, optr), (ptrs, _native.F32, 0, zptrs, optr),
                     (ptrs, _native.F32, n, zptrs, None), (ptrs, _native.F32, n, zholed, optr),
                     (ptrs, _native.F32, n, zodd, optr), (odd, _native.F32, n, zptrs, optr)):
            assert call(ctx, *args, stream) == _native.ERR_INVALID
            assert _native.last_error()
        assert call(None, ptrs, _native.F32, n, zptrs, optr, stream) == _native.ERR_INVALID
        torch.cuda.synchronize(hip_device)
        assert out.cpu().unique().tolist() == [5.0]   # nothing was launched
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_python_refusals_without_a_launch(hip_device):
    sizes = [40, 3]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    x = [torch.ones(s, device=hip_device) for s in sizes]
    try:
        with pytest.raises(ValueError, match="no clients"):
            ctx.sqdist_to_point(ClientTable(2), torch.float32)
        holed = ClientTable(2)
        holed.add_client(x, [1.0, 1.0])
        holed.add_client([x[0], None], [1.0, 1.0])
        with pytest.raises(ValueError, match="client 1 lacks tensor 1"):
            ctx.sqdist_to_point(holed, torch.float32)
        with pytest.raises(NotImplementedError, match="dequantise"):
            ctx.sqdist_to_point(holed, QSGD_F32)
        many = ClientTable(2)
        for _ in range(_native.POINT_MAX_CLIENTS + 1):
            many.add_client(x, [1.0, 1.0])
        with pytest.raises(NotImplementedError, match=str(_native.POINT_MAX_CLIENTS)):
            ctx.sqdist_to_point(many, torch.float32)
        table = table_of([x])
        z = [torch.zeros(s, dtype=torch.float64, device=hip_device) for s in sizes]
        for bad in ([z[0]], [z[0], z[1].float()], [z[0], z[1].cpu()], [z[0], torch.zeros(4, dtype=torch.float64,
                                                                                       device=hip_device)]):
            with pytest.raises(ValueError, match="point"):
                ctx.sqdist_to_point(table, torch.float32, bad)
        assert ctx.sqdist_to_point(table, torch.float32, z).tolist() == [43.0]
        assert ctx.flags() == 0
    finally:
        ctx.close()


def test_open_dynamic_wave_refuses_with_err_state(hip_device):
    layout = ModelLayout.flat(10_000)
    ctx = FedAvgContext(layout, hip_device)
    g = torch.Generator().manual_seed(6)
    dev = [torch.randn(10_000, generator=g).to(hip_device) for _ in range(7)]
    table = NativeClientTable(1, hip_device.index or 0)
    plain = ClientTable(1)
    for x in dev:
        table.add_client([x], [1.0])
        plain.add_client([x], [1.0])
    out = torch.empty(10_000, dtype=torch.float64, device=hip_device)
    outs = OutputTable([out], layout, hip_device, torch.float64)
    try:
        ctx.dyn_open(torch.float32, 16)
        with pytest.raises(_native.NativeError) as e:
            ctx.sqdist_to_point(plain, torch.float32)   # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        torch.cuda.current_stream(hip_device).synchronize()
        assert ctx.dyn_publish(table) == 7
        assert ctx.dyn_close(outs, torch.float64) == (7, True)
        ctx.raise_on_nan()
        D = ctx.sqdist_to_point(plain, torch.float32)    # and accepted once it is closed
        ctx.raise_on_nan()
        want = ref.distances_in_order([[x.cpu()] for x in dev], None, constants(), "f32")
        assert_same_bits(D, want, "after the wave has closed")
    finally:
        ctx.close()
