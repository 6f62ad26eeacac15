"""The moments about a point (csrc/trust_kernels.hip, ``fedavg_moments_about_point``) against
DESIGN.md §5l: dots and squared norms bit for bit against the numpy restatement
(``tests/trust_reference.moments_in_order``) through ``FedAvgContext.moments_about_point`` and
through the C call; the squared norms bit for bit ``sqdist_to_point``; that a client's two entries
depend on nothing but its own values; the dot's error bound in rational arithmetic; the NaN flags;
and the refusals before any launch.

Client and direction values are ``geomed_reference.order_sensitive_values`` (representable in their
format, spread over binades, both signs) beside an N(0, 1) float64 centre: every difference, product
and sum rounds, and tests/test_trust_host.py shows that another order gives other bits. Sizes come
from the build's own geometry (``fedavg_kernel_constant``). No input asks the kernel to read past a
tensor: every pointer is a whole torch tensor or a view that ends inside its buffer.
"""

from __future__ import annotations

import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, _native
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import OutputTable
from distributed_learning_simulation_lib_amd.quantized import QSGD_F32
from tests import trust_reference as ref
from tests import geomed_reference as geo

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
SENTINEL = 12345.0
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def constant(name: str) -> int:
    return _native.kernel_constant(name)


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    return ref.native_constants(_native.kernel_constant)


def counts() -> list[int]:
    return [1, 2, 3, constant("trust_batch") + 1]


def layouts(code: str) -> dict[str, list[int]]:
    """Every edge of the chunk, three sizes per layout; the middle segment is the one whose centre and
    direction are placed 8-byte aligned only, the last one the client segment placed one element in."""
    chunk, ae = constant("trust_chunk"), constant(f"trust_ae_{code}")
    return {"a": [chunk + 1, ae - 1, 2 * chunk + 3], "b": [1, chunk, chunk - 1]}


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def fbits(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).reshape(-1).view(np.int64)


def assert_same_bits(got, want, what="") -> None:
    g, w = fbits(got), fbits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        at = int(np.argwhere(g != w)[0][0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} entries differ in bits; first at {at}: "
                             f"got {g.view(np.float64)[at]!r}, want {w.view(np.float64)[at]!r}")


def place(t: torch.Tensor, device, misalign: bool) -> torch.Tensor:
    """``t`` on the device; ``misalign``: a contiguous view one element into a larger buffer."""
    if not misalign:
        v = t.to(device)
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.data_ptr() % t.element_size() == 0 and v.is_contiguous()
    return v


def table_of(dev_rows) -> ClientTable:
    T = len(dev_rows[0])
    table = ClientTable(T)
    for row in dev_rows:
        table.add_client(row, [1.0] * T)
    return table


@functools.lru_cache(maxsize=None)
def case(code: str, which: str):
    """The largest client count's rows, a float64 centre and direction, and the restatement's dots
    and squared norms about the centre and about the origin: a client's entries do not depend on the
    count, so every smaller count reads the leading entries. Computed once, left unchanged."""
    sizes = layouts(code)[which]
    dtype = DTYPES[code]
    gen = torch.Generator().manual_seed(9000 + 10 * len(code) + ord(code[1]) + ord(which))
    rows = [[geo.order_sensitive_values(gen, s, dtype).to(dtype) for s in sizes] for _ in range(max(counts()))]
    centre = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    direction = [geo.order_sensitive_values(gen, s, torch.float64) for s in sizes]
    about = ref.moments_in_order(rows, centre, direction, constants(), dtype)
    origin = ref.moments_in_order(rows, None, direction, constants(), dtype)
    return sizes, rows, centre, direction, about, origin


# ---- 1. bit for bit against the restatement and the distance kernel ---------------------------------
def test_the_geometry_is_the_point_kernels():
    assert constant("trust_chunk") == constant("point_chunk") and constant("trust_threads") == constant("point_threads")
    for code in DTYPES:
        assert constant(f"trust_ae_{code}") == constant(f"point_ae_{code}")
    assert constant("trust_max_clients") == _native.POINT_MAX_CLIENTS


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_moments_equal_the_restatement_and_the_distances(hip_device, code, which):
    dtype = DTYPES[code]
    sizes, rows, centre, direction, about, origin = case(code, which)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        for misalign in (False, True):
            # misaligned: every client's last segment one element into its buffer, the centre's and the
            # direction's middle segment 8-byte aligned only
            dev = [[place(t, hip_device, misalign and i == 2) for i, t in enumerate(r)] for r in rows]
            v = [place(p, hip_device, misalign and i == 1) for i, p in enumerate(centre)]
            g = [place(p, hip_device, misalign and i == 1) for i, p in enumerate(direction)]
            for n in counts():
                table = table_of(dev[:n])
                for z, (wT, wS) in ((v, about), (None, origin)):
                    T, S = ctx.moments_about_point(table, dtype, z, g)
                    D = ctx.sqdist_to_point(table, dtype, z)
                    assert T.shape == S.shape == (n,) and T.dtype == S.dtype == torch.float64
                    what = f"{code} layout {which} n={n} misaligned={misalign} centre={'yes' if z is not None else 'NULL'}"
                    assert_same_bits(T, wT[:n], "dots, " + what)
                    assert_same_bits(S, wS[:n], "squared norms, " + what)
                    assert_same_bits(S, D, "squared norms against sqdist_to_point, " + what)
        assert ctx.flags() == 0
    finally:
        ctx.close()


def test_1024_clients_of_8_elements(hip_device):
    n = _native.POINT_MAX_CLIENTS
    gen = torch.Generator().manual_seed(5)
    X = geo.order_sensitive_values(gen, 8 * n, torch.float32).to(torch.float32).reshape(n, 8)
    rows = [[X[i]] for i in range(n)]
    centre = [torch.randn(8, generator=gen, dtype=torch.float64)]
    direction = [geo.order_sensitive_values(gen, 8, torch.float64)]
    Xd = X.to(hip_device)
    ctx = FedAvgContext(layout_of([8]), hip_device)
    try:
        T, S = ctx.moments_about_point(table_of([[Xd[i]] for i in range(n)]), torch.float32,
                                       [centre[0].to(hip_device)], [direction[0].to(hip_device)])
        wT, wS = ref.moments_in_order(rows, centre, direction, constants(), torch.float32)
        assert_same_bits(T, wT, "1024 clients: dots")
        assert_same_bits(S, wS, "1024 clients: squared norms")
        assert ctx.flags() == 0
    finally:
        ctx.close()


# ---- 2. a client's entries depend on nothing but its own values ---------------------------------------
def test_entries_are_independent_of_the_other_clients_the_row_and_the_count(hip_device):
    code, dtype = "bf16", torch.bfloat16
    sizes, rows, centre, direction, about, _ = case(code, "a")
    big = max(counts())
    dev = [[t.to(hip_device) for t in r] for r in rows]
    v = [p.to(hip_device) for p in centre]
    g = [p.to(hip_device) for p in direction]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    other = FedAvgContext(layout_of(sizes), hip_device)      # a second context with its own state
    try:
        alone = ctx.moments_about_point(table_of([dev[7]]), dtype, v, g)
        last = ctx.moments_about_point(table_of(dev[8:] + dev[:8]), dtype, v, g)        # row big - 1, other neighbours
        pair = other.moments_about_point(table_of([dev[3], dev[7]]), dtype, v, g)
        again = ctx.moments_about_point(table_of([dev[7]]), dtype, v, g)                # back to back, state reused
        scaled = other.moments_about_point(table_of([[t * 2 for t in dev[0]], dev[7]]), dtype, v, g)
        for k in range(2):                                     # 0: the dot, 1: the squared norm
            want = about[k][7:8]
            assert_same_bits(alone[k], want, "alone")
            assert_same_bits(last[k][big - 1:], want, "last row of the largest table")
            assert_same_bits(pair[k][1:], want, "second of two, second context")
            assert_same_bits(again[k], want, "again")
            assert_same_bits(scaled[k][1:], want, "beside another neighbour")
        assert ctx.flags() == 0 and other.flags() == 0
    finally:
        ctx.close()
        other.close()


# ---- 3. the dot's error bound ----------------------------------------------------------------------
@pytest.mark.parametrize("code", ["f32", "bf16"])
def test_dot_is_within_the_bound_of_the_exact_value(hip_device, code):
    """|T - exact| <= (P + 2) * 2^-53 * sum |(x - v) * g|, P the layout's element count."""
    dtype = DTYPES[code]
    sizes, rows, centre, direction, _, _ = case(code, "b")
    P = sum(sizes)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        dev = [[t.to(hip_device) for t in r] for r in rows[:2]]
        for z in (centre, None):
            T, _ = ctx.moments_about_point(table_of(dev), dtype, None if z is None else [p.to(hip_device) for p in z],
                                           [p.to(hip_device) for p in direction])
            for i, t in enumerate(T.cpu().tolist()):
                exact, mass = ref.exact_dot(rows[i], z, direction)
                err, bound = abs(Fraction(t) - exact), (P + 2) * Fraction(2) ** -53 * mass
                print(f"{code} client {i} centre={'yes' if z is not None else 'NULL'}: error / bound = {float(err / bound):.3g}")
                assert err <= bound
    finally:
        ctx.close()


# ---- 4. the flags -----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan_client", "nan_centre", "nan_direction", "zero_times_inf", "inf_minus_inf"])
def test_nan_flags(hip_device, what):
    chunk = constant("trust_chunk")
    sizes = [chunk + 3, 5]
    gen = torch.Generator().manual_seed(8)
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64).to(torch.float32) for s in sizes] for _ in range(4)]
    centre = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    direction = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    I, A = _native.FLAG_INPUT_NAN, _native.FLAG_ACC_NAN
    at = chunk + 2                                   # the guarded tail of the second chunk
    if what == "nan_client":
        rows[2][0][at] = NAN
        want_flags, nan_dots, nan_sqs = I | A, [2], [2]
    elif what == "nan_centre":
        centre[1][3] = NAN
        want_flags, nan_dots, nan_sqs = I | A, [0, 1, 2, 3], [0, 1, 2, 3]
    elif what == "nan_direction":
        direction[0][at] = NAN
        want_flags, nan_dots, nan_sqs = I | A, [0, 1, 2, 3], []
    elif what == "zero_times_inf":                   # d = 0 exactly for client 1, g = inf: 0 * inf in its dot alone
        centre[0][at] = 0.75
        rows[1][0][at] = 0.75
        direction[0][at] = INF
        want_flags, nan_dots, nan_sqs = A, [1], []
    else:                                            # inf - inf in client 3's difference
        centre[0][at] = INF
        rows[3][0][at] = INF
        want_flags, nan_dots, nan_sqs = A, [3], [3]
    wT, wS = ref.moments_in_order(rows, centre, direction, constants(), torch.float32, check=False)
    assert np.flatnonzero(np.isnan(wT)).tolist() == nan_dots and np.flatnonzero(np.isnan(wS)).tolist() == nan_sqs
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        dev = [[t.to(hip_device) for t in r] for r in rows]
        T, S = ctx.moments_about_point(table_of(dev), torch.float32, [p.to(hip_device) for p in centre],
                                       [p.to(hip_device) for p in direction])
        T, S = T.cpu().numpy(), S.cpu().numpy()
        assert ctx.flags() == want_flags
        for got, want in ((T, wT), (S, wS)):           # NaN payloads aside, the same values everywhere
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert_same_bits(got[~np.isnan(got)], want[~np.isnan(want)], what)
    finally:
        ctx.close()


def test_opposite_infinities_in_a_dot(hip_device):
    """+inf + -inf between two products of one dot: a NaN dot beside a +inf squared norm."""
    sizes = [40]
    x = torch.ones(40)
    x[3], x[17] = INF, INF
    g = torch.ones(40, dtype=torch.float64)
    g[17] = -1.0
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        T, S = ctx.moments_about_point(table_of([[x.to(hip_device)]]), torch.float32, None, [g.to(hip_device)])
        assert np.isnan(T.item()) and S.item() == INF and ctx.flags() == _native.FLAG_ACC_NAN
    finally:
        ctx.close()


# ---- 5. refusals before any launch ------------------------------------------------------------------
def test_c_abi_direct_call_and_refusals(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 5
    gen = torch.Generator().manual_seed(23)
    host = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(n)]
    vhost = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    ghost = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    dev = [[t.to(hip_device) for t in row] for row in host]
    vdev = [z.to(hip_device) for z in vhost]
    gdev = [z.to(hip_device) for z in ghost]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        ptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        vptrs = (ctypes.c_void_p * 2)(*[z.data_ptr() for z in vdev])
        gptrs = (ctypes.c_void_p * 2)(*[z.data_ptr() for z in gdev])
        out = torch.full((2 * n + 1,), SENTINEL, dtype=torch.float64, device=hip_device)
        optr = ctypes.c_void_p(out.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)
        call = lib.fedavg_moments_about_point
        F32 = _native.F32
        totals = (ctypes.c_double * 2)()
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK
        before = bytes(totals)
        assert call(ctx, ptrs, F32, n, vptrs, gptrs, optr, stream) == _native.OK, _native.last_error()
        flags = ctypes.c_uint32(99)
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        wT, wS = ref.moments_in_order(host, vhost, ghost, constants(), torch.float32)
        got = out.cpu().numpy()
        assert_same_bits(got[:n], wT, "C ABI dots")
        assert_same_bits(got[n:2 * n], wS, "C ABI squared norms")
        assert got[2 * n] == SENTINEL                                     # nothing past 2n doubles is written
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK and bytes(totals) == before   # state untouched
        # a NaN latches the input flag; the refusals below must leave it and the outputs as they are
        poisoned = dev[0][1].clone()
        poisoned[1] = NAN
        nanptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        nanptrs[1] = poisoned.data_ptr()
        assert call(ctx, nanptrs, F32, n, vptrs, gptrs, optr, stream) == _native.OK
        torch.cuda.synchronize(hip_device)
        out.fill_(SENTINEL)
        torch.cuda.synchronize(hip_device)
        cap = _native.POINT_MAX_CLIENTS
        holed = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        holed[2 * 2 + 1] = None
        many = (ctypes.c_void_p * ((cap + 1) * 2))(*([dev[0][0].data_ptr(), dev[0][1].data_ptr()] * (cap + 1)))
        odd = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        odd[0] = dev[0][0].data_ptr() + 2
        vholed = (ctypes.c_void_p * 2)(vdev[0].data_ptr(), None)
        vodd = (ctypes.c_void_p * 2)(vdev[0].data_ptr() + 4, vdev[1].data_ptr())
        gholed = (ctypes.c_void_p * 2)(None, gdev[1].data_ptr())
        godd = (ctypes.c_void_p * 2)(gdev[0].data_ptr(), gdev[1].data_ptr() + 4)
        oodd = ctypes.c_void_p(out.data_ptr() + 4)
        for args in ((holed, F32, n, vptrs, gptrs, optr), (many, F32, cap + 1, vptrs, gptrs, optr),
                     (ptrs, _native.QSGD_F32, n, vptrs, gptrs, optr), (ptrs, 99, n, vptrs, gptrs, optr),
                     (None, F32, n, vptrs, gptrs, optr), (ptrs, F32, n, vptrs, None, optr),
                     (ptrs, F32, n, vptrs, gptrs, None), (ptrs, F32, 0, vptrs, gptrs, optr),
                     (ptrs, F32, -1, vptrs, gptrs, optr), (odd, F32, n, vptrs, gptrs, optr),
                     (ptrs, F32, n, vholed, gptrs, optr), (ptrs, F32, n, vodd, gptrs, optr),
                     (ptrs, F32, n, vptrs, gholed, optr), (ptrs, F32, n, vptrs, godd, optr),
                     (ptrs, F32, n, vptrs, gptrs, oodd)):
            assert call(ctx, *args, stream) == _native.ERR_INVALID, args
            assert _native.last_error()
        assert call(None, ptrs, F32, n, vptrs, gptrs, optr, stream) == _native.ERR_INVALID
        torch.cuda.synchronize(hip_device)
        assert out.cpu().unique().tolist() == [SENTINEL]                   # nothing was launched
        rc = lib.fedavg_check(ctx, stream, ctypes.byref(flags))            # the latched flags are still there
        assert rc != _native.OK and flags.value == _native.FLAG_INPUT_NAN | _native.FLAG_ACC_NAN
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_python_refusals_without_a_launch(hip_device):
    sizes = [40, 3]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    x = [torch.ones(s, device=hip_device) for s in sizes]
    z = [torch.zeros(s, dtype=torch.float64, device=hip_device) for s in sizes]
    g = [torch.ones(s, dtype=torch.float64, device=hip_device) for s in sizes]
    try:
        with pytest.raises(ValueError, match="no clients"):
            ctx.moments_about_point(ClientTable(2), torch.float32, z, g)
        holed = ClientTable(2)
        holed.add_client(x, [1.0, 1.0])
        holed.add_client([x[0], None], [1.0, 1.0])
        with pytest.raises(ValueError, match="client 1 lacks tensor 1"):
            ctx.moments_about_point(holed, torch.float32, z, g)
        with pytest.raises(NotImplementedError, match="dequantise"):
            ctx.moments_about_point(holed, QSGD_F32, z, g)
        many = ClientTable(2)
        for _ in range(_native.POINT_MAX_CLIENTS + 1):
            many.add_client(x, [1.0, 1.0])
        with pytest.raises(NotImplementedError, match=str(_native.POINT_MAX_CLIENTS)):
            ctx.moments_about_point(many, torch.float32, z, g)
        table = table_of([x, x])
        with pytest.raises(ValueError, match="direction"):
            ctx.moments_about_point(table, torch.float32, z, None)
        for bad in ([z[0]], [z[0], z[1].float()], [z[0], z[1].cpu()],
                    [z[0], torch.zeros(4, dtype=torch.float64, device=hip_device)]):
            with pytest.raises(ValueError, match="centre"):
                ctx.moments_about_point(table, torch.float32, bad, g)
            with pytest.raises(ValueError, match="direction"):
                ctx.moments_about_point(table, torch.float32, z, bad)
        assert ctx.flags() == 0
        T, S = ctx.moments_about_point(table, torch.float32, z, g)      # 43 elements of (1 - 0) * 1 and (1 - 0)^2
        assert T.tolist() == [43.0, 43.0] and S.tolist() == [43.0, 43.0] and ctx.flags() == 0
    finally:
        ctx.close()


def test_open_dynamic_wave_refuses_with_err_state(hip_device):
    layout = ModelLayout.flat(10_000)
    ctx = FedAvgContext(layout, hip_device)
    gen = torch.Generator().manual_seed(6)
    host = [torch.randn(10_000, generator=gen) for _ in range(7)]
    dev = [x.to(hip_device) for x in host]
    table = NativeClientTable(1, hip_device.index or 0)
    plain = ClientTable(1)
    for x in dev:
        table.add_client([x], [1.0])
        plain.add_client([x], [1.0])
    out = torch.empty(10_000, dtype=torch.float64, device=hip_device)
    outs = OutputTable([out], layout, hip_device, torch.float64)
    vhost = torch.randn(10_000, generator=gen, dtype=torch.float64)
    ghost = torch.randn(10_000, generator=gen, dtype=torch.float64)
    v, g = vhost.to(hip_device), ghost.to(hip_device)
    try:
        ctx.dyn_open(torch.float32, 16)
        with pytest.raises(_native.NativeError) as e:
            ctx.moments_about_point(plain, torch.float32, [v], [g])       # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        assert ctx.dyn_publish(table) == 7
        assert ctx.dyn_close(outs, torch.float64) == (7, True)
        ctx.raise_on_nan()
        T, S = ctx.moments_about_point(plain, torch.float32, [v], [g])    # and accepted once it is closed
        ctx.raise_on_nan()
        wT, wS = ref.moments_in_order([[x] for x in host], [vhost], [ghost], constants(), torch.float32)
        assert_same_bits(T, wT, "after the wave has closed")
        assert_same_bits(S, wS, "after the wave has closed")
    finally:
        ctx.close()
