"""The clip-and-noise pass on the GPU (fedavg_dp_noise): outputs byte-identical to the
numpy restatement (tests/dp_reference.py) for every dtype in whole-list and row mode, repeatable,
indexed by the draw, in place as out of place, written between guard bytes that stay untouched; the
input flag, and the package's GPU path against its CPU path through the endpoints."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    DifferentialPrivacyEmbeddingEndpoint,
    DifferentialPrivacyParameterEndpoint,
    FeatureMessage,
    ParameterMessage,
    _native,
    dp,
)
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout
from tests import dp_cases as cases
from tests import dp_reference as ref

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes before and after every tensor


class Guarded:
    """A device tensor between two guard areas of 0xA5, ``offset`` elements past 16-byte alignment."""

    def __init__(self, x: torch.Tensor, device, offset: int = 0) -> None:
        nbytes = x.numel() * x.element_size()
        self.lo = GUARD + offset * x.element_size()
        self.buf = torch.full((self.lo + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.hi = self.lo + nbytes
        self.tensor = self.buf[self.lo : self.hi].view(x.dtype) if nbytes else torch.empty(0, dtype=x.dtype, device=device)
        self.tensor.copy_(x)

    def fill(self, x: torch.Tensor) -> None:
        self.tensor.copy_(x)

    def bytes(self) -> bytes:
        return self.buf[self.lo : self.hi].cpu().numpy().tobytes()

    def guards_intact(self) -> bool:
        b = self.buf.cpu().numpy()
        return bool((b[: self.lo] == 0xA5).all() and (b[self.hi :] == 0xA5).all())


@pytest.fixture(scope="module")
def ctx(hip_device):
    c = FedAvgContext(ModelLayout.flat(1, "dp"), hip_device)
    yield c
    c.close()


def _check(ctx, device, xs, offsets, want, row_len, c, ids, redraw_want):
    ins = [Guarded(x, device, o) for x, o in zip(xs, offsets)]
    outs = [Guarded(torch.zeros_like(x), device, o) for x, o in zip(xs, offsets)]
    args = (c, cases.SIGMA * c, cases.SEED)

    def run(dst, draw):
        ctx.dp_noise([g.tensor for g in ins], [g.tensor for g in dst], *args, draw, ids, row_len)
        assert ctx.flags() == 0

    run(outs, cases.DRAW)
    got = [g.bytes() for g in outs]
    for t, (g, w) in enumerate(zip(got, want)):
        if g != w:
            a, b = np.frombuffer(g, dtype=np.uint8), np.frombuffer(w, dtype=np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"tensor {t}: {bad.size} bytes differ from the restatement, first at {bad[:8]}")
    assert all(g.guards_intact() for g in ins + outs)
    assert [g.bytes() for g in ins] == [cases.raw(x) for x in xs]  # out of place: the inputs stay
    run(outs, cases.DRAW)
    assert [g.bytes() for g in outs] == got  # the same arguments, the same bytes
    run(outs, cases.DRAW + 1)
    again = [g.bytes() for g in outs]
    assert again == redraw_want and any(a != g for a, g in zip(again, got) if g)  # another draw, other bytes
    run(ins, cases.DRAW)  # in place
    assert [g.bytes() for g in ins] == got
    assert all(g.guards_intact() for g in ins + outs)


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("name", list(cases.list_cases()))
def test_whole_list_matches_restatement(ctx, hip_device, name, dtype):
    xs, c, want = cases.list_case(name, dtype)
    _, _, redraw = cases.list_case(name, dtype, cases.DRAW + 1)
    offsets = [0, 1, 0] if name == "three" else [0] * len(xs)
    _check(ctx, hip_device, xs, offsets, want, 0, c, None, redraw)


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("rows,length", cases.row_cases())
def test_rows_match_restatement(ctx, hip_device, rows, length, dtype):
    x, want = cases.row_case(rows, length, dtype)
    _, redraw = cases.row_case(rows, length, dtype, cases.DRAW + 1)
    _check(ctx, hip_device, [x], [0], [want], length, cases.C, [5], [redraw])


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_shifted_groups_cover_an_even_misalignment(ctx, hip_device, dtype):
    """A tensor two elements (fp64: none: its group is two) past 16 bytes: the apply pass shifts its
    groups; and an output that is aligned differently from its input goes element by element."""
    tl = ref.tile()
    x = cases.values(tl + 11, dtype, 77)
    want = ref.expected([cases.widen(x)], dtype, 0, cases.C, cases.SIGMA * cases.C, cases.SEED, cases.DRAW)
    off = 2 if ref.group(dtype) > 2 else 0
    for in_off, out_off in ((off, off), (off, 0), (0, 1)):
        src, dst = Guarded(x, hip_device, in_off), Guarded(torch.zeros_like(x), hip_device, out_off)
        ctx.dp_noise([src.tensor], [dst.tensor], cases.C, cases.SIGMA * cases.C, cases.SEED, cases.DRAW)
        assert ctx.flags() == 0
        assert [dst.bytes()] == want and src.guards_intact() and dst.guards_intact(), (in_off, out_off)


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_zero_noise_below_the_norm_returns_the_input(ctx, hip_device, dtype):
    """s = 1 and n = z * 0: a row with norm <= C comes back unchanged; a zero comes back as a zero,
    -0.0 only where the input is -0.0 and z < 0 (-0.0 + -0.0 in the contract's last line)."""
    rows, length = 6, 40
    x = (cases.values(rows * length, dtype, 5) * 2.0**-5).reshape(rows, length)
    x[1] = 0
    x[1, 3] = cases.C  # norm = C exactly
    x[2, :8] = torch.tensor([-0.0, 0.0] * 4).to(x.dtype)
    assert (torch.linalg.vector_norm(x.double(), dim=1) <= cases.C).all()
    src = x.reshape(-1).to(hip_device)
    out = torch.empty_like(src)
    ctx.dp_noise([src], [out], cases.C, 0.0, cases.SEED, 0, [0], length)
    assert ctx.flags() == 0
    got = out.cpu()
    assert torch.equal(got.double(), x.reshape(-1).double())  # by value
    nz = (x.reshape(-1) != 0).numpy()
    a = np.frombuffer(cases.raw(got), dtype=np.uint8).reshape(x.numel(), -1)
    b = np.frombuffer(cases.raw(x), dtype=np.uint8).reshape(x.numel(), -1)
    assert np.array_equal(a[nz], b[nz])
    z = dp.normal_stream(cases.SEED, 0, 0, x.numel())
    for i in range(2 * length, 2 * length + 8):
        neg_in = math.copysign(1.0, float(x.reshape(-1)[i])) < 0
        assert (math.copysign(1.0, float(got[i])) < 0) == (neg_in and z[i] < 0), i


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_non_finite_input_raises_and_the_context_stays_usable(ctx, hip_device, bad):
    tl = ref.tile()
    x = cases.values(tl + 5, "f32", 3)
    y = x.clone()
    y[tl + 2] = bad
    out = torch.empty(tl + 5, device=hip_device)
    ctx.dp_noise([y.to(hip_device)], [out], cases.C, 1.0, cases.SEED)
    assert ctx.flags() & _native.FLAG_INPUT_NAN
    ctx.reset()
    with pytest.raises(ValueError):
        dp.add_dp_noise(y.to(hip_device), C=cases.C, sigma=1.0, seed=cases.SEED)
    with pytest.raises(ValueError):
        dp.add_dp_noise_to_parameter({"x": x.to(hip_device), "y": y.to(hip_device)}, C=cases.C, sigma=1.0, seed=1)
    # both contexts answer the next call
    good = dp.add_dp_noise(x.to(hip_device), C=cases.C, sigma=1.0, seed=cases.SEED)
    assert torch.equal(good.cpu(), dp.add_dp_noise(x, C=cases.C, sigma=1.0, seed=cases.SEED))
    ctx.dp_noise([x.to(hip_device)], [out], cases.C, 1.0, cases.SEED)
    assert ctx.flags() == 0


def test_native_refusals(ctx, hip_device):
    x = torch.zeros(12, device=hip_device)
    o = torch.empty_like(x)
    for kw in (dict(row_len=5), dict(row_len=-1), dict(C=0.0), dict(C=math.inf), dict(noise_scale=-1.0),
               dict(noise_scale=math.nan)):
        args = dict(C=1.0, noise_scale=1.0, row_len=0)
        args.update(kw)
        with pytest.raises(_native.NativeError) as e:
            ctx.dp_noise([x], [o], args["C"], args["noise_scale"], 1, 0, None, args["row_len"])
        assert e.value.status == _native.ERR_INVALID
    with pytest.raises(_native.NativeError) as e:
        ctx.dp_noise([x, x], [o, o], 1.0, 1.0, 1, 0, None, 4)  # row mode takes one tensor
    assert e.value.status == _native.ERR_INVALID
    lib = _native.load()
    ptr, n = np.array([x.data_ptr()], dtype=np.uint64), np.array([12], dtype=np.int64)
    null = np.zeros(1, dtype=np.uint64)
    call = lambda dtype, p, cnt, T, q: lib.fedavg_dp_noise(  # noqa: E731
        ctx._h, dtype, p.ctypes.data, cnt.ctypes.data, None, T, q.ctypes.data, 0, 1.0, 1.0, 1, 0, ctx.stream)
    assert call(_native.QSGD_F32, ptr, n, 1, ptr) == _native.ERR_INVALID
    assert call(_native.F32, ptr, n, 0, ptr) == _native.ERR_INVALID
    assert call(_native.F32, ptr, np.array([-1], dtype=np.int64), 1, ptr) == _native.ERR_INVALID
    assert call(_native.F32, null, n, 1, ptr) == _native.ERR_INVALID
    assert call(_native.F32, ptr, n, 1, null) == _native.ERR_INVALID
    assert call(_native.F32, null, np.zeros(1, dtype=np.int64), 1, null) == _native.OK  # NULL where numel == 0
    assert ctx.flags() == 0


def test_endpoints_give_the_cpu_bytes_on_the_gpu(hip_device):
    class Sink:
        def __init__(self):
            self.sent = []

        def send(self, data):
            self.sent.append(data)

    tl = ref.tile()
    p = {"w": cases.values(tl + 70, "f32", 1).reshape(-1, 2), "b": cases.values(9, "f32", 2),
         "s": cases.values(1, "f32", 3).reshape(())}
    f = cases.values(33 * 24, "f16", 4).reshape(33, 24)
    for cls, make in ((DifferentialPrivacyParameterEndpoint, lambda dev: ParameterMessage(
            parameter={k: v.to(dev) for k, v in p.items()})),
            (DifferentialPrivacyEmbeddingEndpoint, lambda dev: FeatureMessage(feature=f.to(dev)))):
        gpu, cpu = Sink(), Sink()
        cls(gpu, C=0.75, seed=99).send(make(hip_device))
        cls(cpu, C=0.75, seed=99).send(make("cpu"))
        a, b = gpu.sent[0], cpu.sent[0]
        if cls is DifferentialPrivacyEmbeddingEndpoint:
            assert a.feature.device == hip_device and a.feature.shape == f.shape
            assert cases.raw(a.feature) == cases.raw(b.feature)
        else:
            for k in p:
                assert a.parameter[k].device == hip_device and a.parameter[k].shape == p[k].shape
                assert cases.raw(a.parameter[k]) == cases.raw(b.parameter[k]), k
