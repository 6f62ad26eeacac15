"""The server optimiser step (csrc/opt_kernels.hip, ``fedavg_server_opt_step``) against DESIGN.md
§5m: ``out``, ``m'`` and ``v'`` bit for bit against the numpy restatement (``tests/opt_reference.step``)
through ``FedAvgContext.server_opt_step`` and through the C call; the square root and the division on
an edge set built in rational arithmetic; Yogi's three sign branches; that an element's results
depend on nothing but its own values; the NaN flags with the inputs left as they were; the refusals
before any launch; and the relation to the fold about a point.

Client values are ``geomed_reference.order_sensitive_values`` beside an N(0, 1) float64 point, as in
tests/test_gpu_clip_contract.py. Sizes come from the build's own geometry
(``fedavg_kernel_constant``). No input asks the kernel to read or write past a tensor: every pointer
is a whole torch tensor or a view that ends inside its buffer, and the elements around every output
view are checked to be untouched.
"""

from __future__ import annotations

import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, _native
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import OutputTable
from distributed_learning_simulation_lib_amd.quantized import QSGD_F32
from tests import geomed_reference as geo
from tests import opt_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
SENTINEL = 12345.0
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
OUT_DTYPES = (torch.float64, torch.float32)
COUNTS = [1, 2, 9, 65]
MODES = ref.MODES
HYPER = {"lr": 0.03, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
I, A, R = _native.FLAG_INPUT_NAN, _native.FLAG_ACC_NAN, _native.FLAG_RESULT_NAN


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
    """``t`` on the device; ``misalign``: a contiguous view one element into a larger buffer (for
    float64: 8-byte aligned only)."""
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

    def numpy(self):
        return [v.cpu().numpy() for v in self.views]


def table_of(dev_rows) -> ClientTable:
    T = len(dev_rows[0])
    table = ClientTable(T)
    for row in dev_rows:
        table.add_client(row, [1.0] * T)
    return table


def step_once(device, dev_rows, dtype, sizes, coef, divisor, z, m, v, mode, out_dtype=torch.float64, misalign_out=False,
              want_flags=0, hyper=HYPER):
    """One call on a fresh context. ``z``, ``m``, ``v`` are device tensors; they must come back bit
    for bit as they went in. Returns (outs, m_new, v_new) as numpy arrays per segment."""
    ctx = FedAvgContext(layout_of(sizes), device)
    try:
        before = [[bits(t).copy() for t in g] for g in (z, m, v)]
        outs = Outs(sizes, out_dtype, device, misalign_out)
        mo = Outs(sizes, torch.float64, device, misalign_out)
        vo = Outs(sizes, torch.float64, device, misalign_out)
        ctx.server_opt_step(table_of(dev_rows), dtype, coef, divisor, z, m, v, mo.views, vo.views, outs.views, out_dtype,
                            mode=mode, **hyper)
        assert ctx.flags() == want_flags
        assert outs.guards_untouched() and mo.guards_untouched() and vo.guards_untouched()
        if mode == "avgm":
            assert vo.untouched()
        for g, b in zip((z, m, v), before):
            for t, w in zip(g, b):
                assert np.array_equal(bits(t), w), "an input buffer changed"
        return outs.numpy(), mo.numpy(), (None if mode == "avgm" else vo.numpy())
    finally:
        ctx.close()


def coefficients(n: int, seed: int = 0) -> list[float]:
    """Between 0 and 3, some above 1; where there is room one exact 0.0 and one exact 1.0."""
    gen = torch.Generator().manual_seed(100 + n + seed)
    c = (3.0 * torch.rand(n, generator=gen, dtype=torch.float64)).tolist()
    if n >= 3:
        c[1], c[2] = 0.0, 1.0
    return c


def compare(got, want, what):
    (outs, ms, vs), (wo, wm, wv) = got, want
    for t in range(len(wo)):
        assert_same_bits(outs[t], wo[t], f"{what} out, segment {t}")
        assert_same_bits(ms[t], wm[t], f"{what} m', segment {t}")
        if wv is not None:
            assert_same_bits(vs[t], wv[t], f"{what} v', segment {t}")
    assert (vs is None) == (wv is None)


# ---- 1. bit for bit against the restatement ----------------------------------------------------
def sizes_for(code: str) -> list[int]:
    ae, tile = constant(f"opt_ae_{code}"), constant("opt_tile")
    assert tile == constant("clip_tile") and constant("opt_threads") == 256
    return [1, max(ae - 1, 1), ae + 1, tile - 1, tile, tile + 1, 2 * tile + 3]


def thinned(ci: int, ni: int) -> tuple[str, torch.dtype]:
    """The mode and the out dtype of case (client dtype ci, client count ni): a Latin square, so every
    pair of (dtype, count, mode, out dtype) values meets in some case."""
    return MODES[(ci + ni) % 4], OUT_DTYPES[(ci + ni // 2) % 2]


def test_the_thinning_is_pairwise():
    cases = [(ci, ni, *thinned(ci, ni)) for ci in range(4) for ni in range(4)]
    for a in range(4):
        for b in range(a + 1, 4):
            seen = {(c[a], c[b]) for c in cases}
            assert len(seen) == len({c[a] for c in cases}) * len({c[b] for c in cases}), (a, b)


@functools.lru_cache(maxsize=None)
def case(code: str):
    """The largest client count's rows, a float64 point and moments; every smaller count reads the
    leading rows. Computed once, left unchanged."""
    sizes = sizes_for(code)
    gen = torch.Generator().manual_seed(9000 + len(code) + ord(code[1]))
    rows = [[geo.order_sensitive_values(gen, s, DTYPES[code]) for s in sizes] for _ in range(max(COUNTS))]
    point = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    m = [0.1 * torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    # second moments on both sides of delta^2 (Yogi's branches), spread over binades
    v = [torch.rand(s, generator=gen, dtype=torch.float64) * geo.order_sensitive_values(gen, s, torch.float64) ** 2
         for s in sizes]
    return sizes, rows, point, m, v


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_step_equals_the_restatement(hip_device, code, n):
    dtype = DTYPES[code]
    mode, out_dtype = thinned(list(DTYPES).index(code), COUNTS.index(n))
    sizes, rows, point, m, v = case(code)
    rows = rows[:n]
    coef = coefficients(n)
    divisor = 0.7 * n + 0.3
    want = ref.step(rows, coef, divisor, point, m, v, mode, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["tau"],
                    np_out(out_dtype))
    assert want[3] == 0
    # aligned: the vector paths. Misaligned: the clients' segments 3, 4 and 6 one element into their
    # buffers, the same segments of z, m_in and v_in only 8-byte aligned, every output one element in
    for misalign in (False, True):
        off = (3, 4, 6) if misalign else ()
        dev = [[place(t.to(dtype), hip_device, i in off) for i, t in enumerate(r)] for r in rows]
        z, md, vd = ([place(p, hip_device, i in off) for i, p in enumerate(g)] for g in (point, m, v))
        got = step_once(hip_device, dev, dtype, sizes, coef, divisor, z, md, vd, mode, out_dtype, misalign_out=misalign)
        compare(got, want[:3], f"{code} n={n} {mode} out={out_dtype} misaligned={misalign}")


# ---- 2. the square root and the division ---------------------------------------------------------
def ulp_steps(x: float, k: int) -> float:
    for _ in range(abs(k)):
        x = math.nextafter(x, INF if k > 0 else -INF)
    return x


@functools.lru_cache(maxsize=None)
def sqrt_edge_set() -> np.ndarray:
    tiny, dbl_min, dbl_max = 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308
    vals = [0.0, tiny, ulp_steps(dbl_min, -1), dbl_min, ulp_steps(dbl_min, 1), dbl_max, ulp_steps(dbl_max, -1), 1.0, 2.0,
            4.0, 0.25]
    rng = np.random.default_rng(12)
    # k^2 (exact: k below 2^26, scaled by an even power of two) and its two neighbours, across binades
    for e in range(-1060, 961, 20):
        k = int(rng.integers(2 ** 25, 2 ** 26)) | 1
        sq = math.ldexp(float(k * k), 2 * (e // 2))
        if 0.0 < sq < INF:
            vals += [ulp_steps(sq, -1), sq, ulp_steps(sq, 1)]
    # values whose root lies within a few ulp of a rounding midpoint: the midpoint of two neighbouring
    # doubles squared in rational arithmetic, rounded to a double (float(Fraction) rounds correctly),
    # and that double's neighbours
    for e in list(range(-1020, 1021, 12)) + [-1, 0, 1]:
        r = math.ldexp(float(rng.uniform(1.0, 2.0)), e // 2)
        mid = (Fraction(r) + Fraction(math.nextafter(r, INF))) / 2
        sq = float(mid * mid)
        if 0.0 < sq < INF:
            vals += [ulp_steps(sq, d) for d in (-2, -1, 0, 1, 2)]
    # and subnormal arguments
    for _ in range(40):
        vals.append(float(rng.integers(1, 2 ** 52)) * tiny)
    out = np.array(vals, dtype=np.float64)
    assert (out >= 0).all() and np.isfinite(out).all()
    return out


def test_square_root_and_division_edge_set(hip_device):
    """Adagrad with every client equal to z: delta = 0, v' = v exactly, r = sqrt(v); m and lr over
    binades so that num / den rounds. Bit for bit numpy's sqrt and division."""
    v = sqrt_edge_set()
    s = int(v.size)
    assert s > constant("opt_tile") // 4
    rng = np.random.default_rng(13)
    m = rng.uniform(1.0, 2.0, s) * np.exp2(rng.integers(-40, 40, s)) * rng.choice([-1.0, 1.0], s)
    z = np.zeros(s)
    rows = [[torch.zeros(s, dtype=torch.float64)] for _ in range(2)]
    dev = [[t.to(hip_device) for t in r] for r in rows]
    zd, md, vd = ([torch.from_numpy(a).to(hip_device)] for a in (z, m, v))
    for lr, tau in ((1.1 * 2.0 ** -7, 1e-3), (1.0, 2.0 ** -600), (3.0e5, 1e-8)):
        hyper = {"lr": lr, "beta1": 0.9, "beta2": 0.99, "tau": tau}
        outs, ms, vs = step_once(hip_device, dev, torch.float64, [s], [1.0, 2.0], 3.0, zd, md, vd, "adagrad", hyper=hyper)
        with np.errstate(over="ignore", under="ignore"):
            m_new = np.float64(0.9) * m + np.float64(ref.one_minus(0.9)) * np.zeros(s)
            want = (np.float64(lr) * m_new) / (np.sqrt(v) + np.float64(tau))
        assert_same_bits(vs[0], v, "v' = v + 0")
        assert_same_bits(ms[0], m_new, "m'")
        assert_same_bits(outs[0], z + want, f"lr {lr} tau {tau}: (lr m') / (sqrt(v) + tau)")
        compare((outs, ms, vs), ref.step(rows, [1.0, 2.0], 3.0, [z], [m], [v], "adagrad", lr, 0.9, 0.99, tau)[:3], "edge set")


# ---- 3. Yogi's sign branches ---------------------------------------------------------------------
def test_yogi_sign_branches_in_one_launch(hip_device):
    """One client with c = 1, W = 1 and z = 0: delta = x exactly. v above, below and equal to delta^2,
    v = 0, delta = 0 and delta = -0.0 in one launch."""
    x = np.array([3.0, 3.0, 3.0, 0.5, 0.0, -0.0, 0.0, -0.0, 1.5, -2.0, 2.0 ** -30, 7.0], dtype=np.float64)
    v = np.array([10.0, 2.0, 9.0, 0.0, 0.0, 0.0, 4.0, 4.0, 1.0, 4.0, 2.0 ** -60, 50.0], dtype=np.float64)
    m = np.linspace(-1.0, 1.0, x.size)
    z = np.zeros(x.size)
    rows = [[torch.from_numpy(x)]]
    dev = [[rows[0][0].to(hip_device)]]
    zd, md, vd = ([torch.from_numpy(a).to(hip_device)] for a in (z, m, v))
    got = step_once(hip_device, dev, torch.float64, [x.size], [1.0], 1.0, zd, md, vd, "yogi")
    want = ref.step(rows, [1.0], 1.0, [z], [m], [v], "yogi", **HYPER)
    assert want[3] == 0
    compare(got, want[:3], "yogi")
    f = np.float64(ref.one_minus(HYPER["beta2"])) * (x * x)
    g = v - x * x
    assert (g > 0).sum() >= 3 and (g < 0).sum() >= 3 and (g == 0).sum() >= 4
    assert_same_bits(got[2][0], np.where(g > 0, v - f, np.where(g < 0, v + f, v)), "v - f sign(v - delta^2)")


# ---- 4. an element's results depend on nothing else -----------------------------------------------
def test_changing_one_element_of_one_client_changes_that_element_alone(hip_device):
    code, dtype, n = "f32", torch.float32, 9
    tile = constant("opt_tile")
    sizes = [tile + 3, 5]
    gen = torch.Generator().manual_seed(31)
    rows = [[geo.order_sensitive_values(gen, s, dtype).to(dtype) for s in sizes] for _ in range(n)]
    z, m = ([torch.randn(s, generator=gen, dtype=torch.float64).to(hip_device) for s in sizes] for _ in range(2))
    v = [torch.rand(s, generator=gen, dtype=torch.float64).to(hip_device) for s in sizes]
    coef = coefficients(n)

    def run(rs):
        dev = [[t.to(hip_device) for t in r] for r in rs]
        return step_once(hip_device, dev, dtype, sizes, coef, 4.0, z, m, v, "adam")

    base = run(rows)
    at = tile + 1                                  # the guarded tail of the second tile
    changed = [[t.clone() for t in r] for r in rows]
    changed[4][0][at] += 0.75
    other = run(changed)
    for b, o in zip(base, other):
        differs = bits(b[0]) != bits(o[0])
        assert differs[at] and int(differs.sum()) == 1
        assert_same_bits(b[1], o[1], "the other segment")


# ---- 5. the flags ---------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan_client", "nan_point", "nan_m", "nan_v", "inf_client"])
def test_nan_flags_leave_the_inputs_unchanged(hip_device, what):
    tile = constant("opt_tile")
    sizes = [tile + 3, 5]
    gen = torch.Generator().manual_seed(8)
    rows = [[torch.randn(s, generator=gen, dtype=torch.float64).to(torch.float32) for s in sizes] for _ in range(4)]
    z, m = ([torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes] for _ in range(2))
    v = [torch.rand(s, generator=gen, dtype=torch.float64) for s in sizes]
    coef = [1.0, 0.5, 2.0, 1.5]
    at = tile + 2
    mode = "adagrad"
    if what == "nan_client":
        rows[2][0][at] = NAN
        want_flags = I | A | R
    elif what == "nan_point":
        z[1][3] = NAN
        want_flags = I | A | R
    elif what == "nan_m":                           # the sum is clean: m enters after it
        m[0][at] = NAN
        want_flags = I | R
    elif what == "nan_v":
        v[1][0] = NAN
        want_flags = I | R
    else:                                           # acc = delta = m' = v' = +inf are no NaN; u = inf / inf is
        rows[1][0][at] = INF
        want_flags = R
    want = ref.step(rows, coef, 4.0, z, m, v, mode, **HYPER)
    assert (I, A, R) == (ref.FLAG_INPUT, ref.FLAG_ACC, ref.FLAG_RESULT) and want[3] == want_flags
    dev = [[t.to(hip_device) for t in r] for r in rows]
    zd, md, vd = ([t.to(hip_device) for t in g] for g in (z, m, v))
    got = step_once(hip_device, dev, torch.float32, sizes, coef, 4.0, zd, md, vd, mode, want_flags=want_flags)
    for g, w in zip(got, want[:3]):                 # NaN payloads aside, the same values everywhere
        for t in range(len(sizes)):
            assert np.array_equal(np.isnan(g[t]), np.isnan(w[t])), (what, t)
            assert_same_bits(g[t][~np.isnan(g[t])], w[t][~np.isnan(w[t])], f"{what}: beside the NaN, segment {t}")
    assert int(sum(np.isnan(o).sum() for o in got[0])) == 1      # one element's model is lost, no other


# ---- 6. refusals before any launch ----------------------------------------------------------------
def test_c_abi_direct_call_and_refusals(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 5
    gen = torch.Generator().manual_seed(23)
    host = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(n)]
    zhost, mhost = ([torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes] for _ in range(2))
    vhost = [torch.rand(s, generator=gen, dtype=torch.float64) for s in sizes]
    dev = [[t.to(hip_device) for t in row] for row in host]
    zdev, mdev, vdev = ([t.to(hip_device) for t in g] for g in (zhost, mhost, vhost))
    coef = [1.0, 0.0, 2.5, 0.25, 1.0]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        D = ctypes.c_double
        P2 = ctypes.c_void_p * 2

        def table(ts):
            return P2(*[t.data_ptr() for t in ts])

        ptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        z, mi, vi = table(zdev), table(mdev), table(vdev)
        cs = (D * n)(*coef)
        results = [[torch.full((s,), SENTINEL, dtype=torch.float64, device=hip_device) for s in sizes] for _ in range(3)]
        outs, mouts, vouts = results
        o, mo, vo = table(outs), table(mouts), table(vouts)
        stream = ctypes.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)
        F32, F64 = _native.F32, _native.F64
        lr, b1, b2, tau = 0.03, 0.9, 0.99, 1e-3
        ob1, ob2 = 1.0 - b1, 1.0 - b2

        def call(c=ctx, p=ptrs, idt=F32, co=cs, k=n, div=5.0, zz=z, m_in=mi, v_in=vi, m_out=mo, v_out=vo,
                 mode=_native.OPT_ADAM, lr=lr, b1=b1, b2=b2, tau=tau, oo=o, odt=F64):
            return lib.fedavg_server_opt_step(c, p, idt, co, k, div, zz, m_in, v_in, m_out, v_out, mode, lr, b1, ob1, b2,
                                              ob2, tau, oo, odt, stream)

        totals = (D * 2)()
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK
        before = bytes(totals)
        for mode_name, mode_code in (("adam", _native.OPT_ADAM), ("avgm", _native.OPT_AVGM)):
            for g in results:
                for t in g:
                    t.fill_(SENTINEL)
            avgm = mode_name == "avgm"        # avgm: the second-moment tables may be NULL
            assert call(mode=mode_code, v_in=None if avgm else vi, v_out=None if avgm else vo) == _native.OK, \
                _native.last_error()
            flags = ctypes.c_uint32(99)
            assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
            want = ref.step(host, coef, 5.0, zhost, mhost, vhost, mode_name, lr, b1, b2, tau)
            for t in range(2):
                assert_same_bits(outs[t], want[0][t], "C ABI out")
                assert_same_bits(mouts[t], want[1][t], "C ABI m'")
                if avgm:
                    assert vouts[t].cpu().unique().tolist() == [SENTINEL]
                else:
                    assert_same_bits(vouts[t], want[2][t], "C ABI v'")
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK and bytes(totals) == before   # state untouched
        # refused before any launch, each with a message
        for g in results:
            for t in g:
                t.fill_(SENTINEL)
        cap = _native.POINT_MAX_CLIENTS
        holed = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        holed[2 * 2 + 1] = None
        many = (ctypes.c_void_p * ((cap + 1) * 2))(*([dev[0][0].data_ptr(), dev[0][1].data_ptr()] * (cap + 1)))
        many_cs = (D * (cap + 1))(*([1.0] * (cap + 1)))
        odd = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        odd[0] = dev[0][0].data_ptr() + 2

        def hole(ts):
            return P2(ts[0].data_ptr(), None)

        def skew(ts):
            return P2(ts[0].data_ptr() + 4, ts[1].data_ptr())

        cs_nan, cs_inf = (D * n)(1.0, NAN, 1.0, 1.0, 1.0), (D * n)(1.0, 1.0, 1.0, -INF, 1.0)
        refused = [dict(p=holed), dict(p=many, co=many_cs, k=cap + 1), dict(idt=_native.QSGD_F32), dict(idt=99),
                   dict(odt=_native.F16), dict(odt=99), dict(p=None), dict(co=None), dict(zz=None), dict(oo=None),
                   dict(k=0), dict(k=-1), dict(p=odd), dict(zz=hole(zdev)), dict(zz=skew(zdev)), dict(oo=hole(outs)),
                   dict(oo=skew(outs)), dict(co=cs_nan), dict(co=cs_inf), dict(div=0.0), dict(div=-1.0), dict(div=INF),
                   dict(div=NAN),
                   # the optimiser's own
                   dict(mode=4), dict(mode=-1), dict(lr=0.0), dict(lr=-1.0), dict(lr=INF), dict(lr=NAN),
                   dict(b1=-0.1), dict(b1=1.0), dict(b1=NAN), dict(b2=-0.1), dict(b2=1.0), dict(b2=NAN),
                   dict(tau=0.0), dict(tau=-1.0), dict(tau=INF), dict(tau=NAN),
                   dict(mode=_native.OPT_YOGI, tau=0.0), dict(mode=_native.OPT_ADAGRAD, tau=NAN),
                   dict(m_in=None), dict(m_out=None), dict(v_in=None), dict(v_out=None),
                   dict(mode=_native.OPT_AVGM, m_in=None), dict(mode=_native.OPT_AVGM, m_out=None),
                   dict(m_in=hole(mdev)), dict(m_out=hole(mouts)), dict(v_in=hole(vdev)), dict(v_out=hole(vouts)),
                   dict(m_in=skew(mdev)), dict(m_out=skew(mouts)), dict(v_in=skew(vdev)), dict(v_out=skew(vouts)),
                   # not in-place
                   dict(oo=P2(outs[0].data_ptr(), zdev[1].data_ptr())),
                   dict(m_out=P2(mouts[0].data_ptr(), mdev[1].data_ptr())),
                   dict(v_out=P2(vdev[0].data_ptr(), vouts[1].data_ptr())),
                   dict(mode=_native.OPT_AVGM, m_out=P2(mdev[0].data_ptr(), mouts[1].data_ptr()))]
        for kw in refused:
            assert call(**kw) == _native.ERR_INVALID, kw
            assert _native.last_error()
        assert call(c=None) == _native.ERR_INVALID
        assert call(mode=_native.OPT_AVGM, tau=NAN, v_in=None, v_out=None) == _native.OK     # avgm ignores tau and v
        torch.cuda.synchronize(hip_device)
        for t in vouts:
            assert t.cpu().unique().tolist() == [SENTINEL]
        for g in (outs, mouts):
            for t in g:
                t.fill_(SENTINEL)
        for kw in refused[:4] + refused[-4:]:
            assert call(**kw) == _native.ERR_INVALID
        torch.cuda.synchronize(hip_device)
        assert all(t.cpu().unique().tolist() == [SENTINEL] for g in results for t in g)   # nothing was launched
        for dev_g, host_g in ((zdev, zhost), (mdev, mhost), (vdev, vhost)):                 # the inputs are unchanged
            for d, h in zip(dev_g, host_g):
                assert_same_bits(d, h.numpy(), "an input")
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_python_refusals_without_a_launch(hip_device):
    sizes = [40, 3]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    x = [torch.ones(s, device=hip_device) for s in sizes]
    z, m, v = ([torch.zeros(s, dtype=torch.float64, device=hip_device) for s in sizes] for _ in range(3))
    outs, mo, vo = (Outs(sizes, torch.float64, hip_device, False) for _ in range(3))
    o = outs.views
    table = table_of([x, x])

    def step(tb=table, dt=torch.float32, coef=(1.0, 1.0), div=1.0, zz=z, mi=m, vi=v, mm=mo.views, vv=vo.views, oo=o,
             odt=torch.float64, mode="adam", **hyper):
        ctx.server_opt_step(tb, dt, list(coef), div, zz, mi, vi, mm, vv, oo, odt, mode=mode, **{**HYPER, **hyper})

    try:
        with pytest.raises(ValueError, match="no clients"):
            step(tb=ClientTable(2), coef=())
        holed = ClientTable(2)
        holed.add_client(x, [1.0, 1.0])
        holed.add_client([x[0], None], [1.0, 1.0])
        with pytest.raises(ValueError, match="client 1 lacks tensor 1"):
            step(tb=holed)
        with pytest.raises(NotImplementedError, match="dequantise"):
            step(tb=holed, dt=QSGD_F32)
        for coef in ([1.0], [1.0, NAN], [INF, 1.0]):
            with pytest.raises(ValueError, match="coefficient"):
                step(coef=coef)
        for div in (0.0, -2.0, INF, NAN):
            with pytest.raises(ValueError, match="divisor"):
                step(div=div)
        with pytest.raises(TypeError):
            step(odt=torch.float16)
        with pytest.raises(ValueError, match="mode"):
            step(mode="sgd")
        for kw, match in ((dict(lr=0.0), "learning rate"), (dict(beta1=1.0), "beta1"), (dict(beta2=-1.0), "beta2"),
                          (dict(tau=0.0), "tau")):
            with pytest.raises(ValueError, match=match):
                step(**kw)
        with pytest.raises(ValueError, match="second-moment"):
            step(vi=None)
        for name in ("zz", "mi", "vi", "mm", "vv"):
            for bad in ([z[0]], [z[0], z[1].float()], [z[0], z[1].cpu()],
                        [z[0], torch.zeros(4, dtype=torch.float64, device=hip_device)]):
                with pytest.raises(ValueError, match="tensor|per segment"):
                    step(**{name: bad})
        with pytest.raises(ValueError, match="output"):
            step(oo=[o[0], o[1].float()])
        with pytest.raises(ValueError, match="in-place"):
            step(oo=[o[0], z[1]])
        with pytest.raises(ValueError, match="in-place"):
            step(mm=[mo.views[0], m[1]])
        with pytest.raises(ValueError, match="in-place"):
            step(vv=[v[0], vo.views[1]])
        torch.cuda.synchronize(hip_device)
        assert outs.untouched() and mo.untouched() and vo.untouched() and ctx.flags() == 0
        step(mode="avgm", coef=(1.0, 0.5), div=3.0, vi=None, vv=None, lr=2.0, beta1=0.5)   # m' = 0.5, u = 1.0
        assert ctx.flags() == 0 and all(t.cpu().unique().tolist() == [1.0] for t in o)
        assert all(t.cpu().unique().tolist() == [0.5] for t in mo.views) and vo.untouched()
        assert outs.guards_untouched() and mo.guards_untouched()
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
    zhost, mhost = (torch.randn(10_000, generator=g, dtype=torch.float64) for _ in range(2))
    z, m = zhost.to(hip_device), mhost.to(hip_device)
    res, mres = (torch.full((10_000,), SENTINEL, dtype=torch.float64, device=hip_device) for _ in range(2))
    coef = coefficients(7)

    def step():
        ctx.server_opt_step(plain, torch.float32, coef, 7.0, [z], [m], None, [mres], None, [res], mode="avgm", **HYPER)

    try:
        ctx.dyn_open(torch.float32, 16)
        with pytest.raises(_native.NativeError) as e:
            step()                                                   # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        torch.cuda.current_stream(hip_device).synchronize()
        assert res.cpu().unique().tolist() == [SENTINEL] and mres.cpu().unique().tolist() == [SENTINEL]
        assert ctx.dyn_publish(table) == 7
        assert ctx.dyn_close(outs, torch.float64) == (7, True)
        ctx.raise_on_nan()
        step()                                                       # and accepted once it is closed
        ctx.raise_on_nan()
        want = ref.step([[x] for x in host], coef, 7.0, [zhost], [mhost], None, "avgm", **HYPER)
        assert_same_bits(res, want[0][0], "after the wave has closed")
        assert_same_bits(mres, want[1][0], "m' after the wave has closed")
    finally:
        ctx.close()


# ---- 7. the relation to the fold about a point ------------------------------------------------------
def test_avgm_without_momentum_is_the_fold_about_the_point(hip_device):
    code, dtype, n = "bf16", torch.bfloat16, 9
    sizes, rows, point, m, _ = case(code)
    rows = rows[:n]
    coef = coefficients(n)
    dev = [[t.to(dtype).to(hip_device) for t in r] for r in rows]
    z = [p.to(hip_device) for p in point]
    zero = [torch.zeros(s, dtype=torch.float64, device=hip_device) for s in sizes]
    hyper = {"lr": 1.0, "beta1": 0.0, "beta2": 0.0, "tau": 1.0}
    outs, ms, _ = step_once(hip_device, dev, dtype, sizes, coef, 6.5, z, zero, zero, "avgm", hyper=hyper)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        fold = [torch.empty(s, dtype=torch.float64, device=hip_device) for s in sizes]
        ctx.fold_about_point(table_of(dev), dtype, coef, 6.5, z, fold)
        assert ctx.flags() == 0
        for t in range(len(sizes)):
            assert_same_bits(outs[t], fold[t], f"segment {t}")
            # and m' is the pseudo-gradient itself: out = z + m'
            assert_same_bits(point[t].numpy() + ms[t], fold[t], f"z + m', segment {t}")
    finally:
        ctx.close()
