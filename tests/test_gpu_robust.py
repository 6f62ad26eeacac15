"""The trimmed-mean / median kernel (csrc/robust_kernels.hip) on the MI355X against the torch-CPU
restatement of the rules (tests/robust_reference.py; NOT a reference algorithm). Tolerance: none —
every result is compared bit for bit, as integer views.

Sizes come from the build's own geometry (``fedavg_kernel_constant``): 1, one element short of a
16-byte vector, tile - 1 / tile / tile + 1, and a segment whose storage starts off a 16-byte
boundary. Client counts sit on both sides of every network width (2, 4, ..., 64). Values are drawn
from a small pool so that ties, signed zeros, subnormals and infinities are frequent; a segment
holds infinities of one sign only (both kept would be the result-NaN error, tested separately).
No input asks the kernel to read past a tensor.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from distributed_learning_simulation_lib_amd import (
    ClientTable,
    FedAvgContext,
    ModelLayout,
    NaNAggregationError,
    ParameterMessage,
    RobustFedAVGAlgorithm,
    _native,
)
from tests import robust_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
RULES = [("median", 0.0), ("trimmed_mean", 0.0), ("trimmed_mean", 0.1), ("trimmed_mean", 0.25), ("trimmed_mean", 0.49)]
COUNTS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]
# finite pool: zeros of both signs, ties, a subnormal of every input format (2^-24: fp16; 2^-130:
# fp32 / bf16; 2^-1030: fp64), large magnitudes; the segment's infinity is appended
POOL = [0.0, -0.0, 1.0, 1.0, -1.0, 1.5, 0.1, -7.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -130, -(2.0 ** -130),
        2.0 ** -1030, 6.0e4, -6.0e4, 3.0e38]


def as_bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def draw(gen: torch.Generator, numel: int, dtype: torch.dtype, inf: float) -> torch.Tensor:
    # 3e38 would round to +inf in fp16, beside a segment's -inf
    finite = [6.0e4 if (dtype == torch.float16 and v == 3.0e38) else v for v in POOL]
    pool = torch.tensor(finite + [inf, inf], dtype=torch.float64)
    return pool[torch.randint(0, len(pool), (numel,), generator=gen)].to(dtype)


def edge_sizes(code: str) -> list[int]:
    tile = _native.kernel_constant("robust_tile")
    ae = _native.kernel_constant(f"robust_ae_{code}")
    return [1, ae - 1, tile - 1, tile, tile + 1, 2 * ae + 1]


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


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_kernel_matches_restatement(hip_device, code, n):
    dtype = DTYPES[code]
    sizes = edge_sizes(code)
    gen = torch.Generator().manual_seed(1000 * n + len(code))
    host = [[draw(gen, s, dtype, INF if t % 2 == 0 else -INF) for t, s in enumerate(sizes)] for _ in range(n)]
    layout = ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))
    ctx = FedAvgContext(layout, hip_device)
    last = len(sizes) - 1  # the last segment's storage is misaligned for every client
    table = ClientTable(len(sizes))
    for row in host:
        table.add_client([place(t, hip_device, i == last) for i, t in enumerate(row)], [1.0] * len(sizes))
    try:
        for mode, trim in RULES:
            for out_dtype in (torch.float64, torch.float32):
                want = [ref.reduce_tensor([row[i] for row in host], mode, trim, out_dtype) for i in range(len(sizes))]
                outs = [torch.full((s,), 123.0, dtype=out_dtype, device=hip_device) for s in sizes]
                ctx.robust_aggregate(table, dtype, mode, trim, outs, out_dtype)
                ctx.raise_on_nan([(table, dtype)])
                for i, (o, w) in enumerate(zip(outs, want)):
                    assert np.array_equal(as_bits(o), as_bits(w)), (mode, trim, out_dtype, sizes[i])
    finally:
        ctx.close()


def test_misaligned_output_and_many_tiles(hip_device):
    tile = _native.kernel_constant("robust_tile")
    sizes = [3 * tile + 5, 7]
    gen = torch.Generator().manual_seed(3)
    host = [[draw(gen, s, torch.float32, INF) for s in sizes] for _ in range(5)]
    layout = ModelLayout(names=("a", "b"), shapes=tuple((s,) for s in sizes))
    ctx = FedAvgContext(layout, hip_device)
    table = ClientTable(2)
    for row in host:
        table.add_client([t.to(hip_device) for t in row], [1.0, 1.0])
    outs = [place(torch.zeros(s, dtype=torch.float64), hip_device, True) for s in sizes]
    ctx.robust_aggregate(table, torch.float32, "trimmed_mean", 0.25, outs, torch.float64)
    ctx.raise_on_nan()
    for i, o in enumerate(outs):
        want = ref.reduce_tensor([row[i] for row in host], "trimmed_mean", 0.25)
        assert np.array_equal(as_bits(o), as_bits(want))
    ctx.close()


def _round(hip_device, clients, mode, trim, out_dtype=torch.float64, on_device=True):
    algo = RobustFedAVGAlgorithm(mode=mode, trim=trim, device=hip_device, out_dtype=out_dtype)
    for wid, c in enumerate(clients):
        if c is None:
            algo.process_worker_data(wid, None)
        else:
            p = {k: (v.to(hip_device) if on_device else v) for k, v in c.items()}
            algo.process_worker_data(wid, ParameterMessage(parameter=p, aggregation_weight=wid + 1))
    return algo.aggregate_worker_data()


@pytest.mark.parametrize("on_device", [True, False])
def test_algorithm_round_with_missing_tensor_and_skipped_client(hip_device, on_device):
    tile = _native.kernel_constant("robust_tile")
    gen = torch.Generator().manual_seed(17)
    shapes = {"w": (tile + 3,), "b": (5,), "m": (3, 7), "scalar": ()}
    clients = [{k: draw(gen, int(np.prod(s, dtype=np.int64)), torch.float32, INF).reshape(s) for k, s in shapes.items()}
               for _ in range(9)]
    clients[3] = None
    del clients[1]["b"]      # n differs per segment: 8 for most, 6 for "b"
    del clients[6]["b"]
    for mode, trim in (("median", 0.0), ("trimmed_mean", 0.25)):
        for out_dtype in (torch.float64, torch.float32):
            msg = _round(hip_device, clients, mode, trim, out_dtype, on_device)
            want = ref.reduce_round(clients, mode, trim, out_dtype)
            assert list(msg.parameter) == list(want)
            for name, w in want.items():
                got = msg.parameter[name]
                assert got.device.type == "cuda" and got.shape == w.shape and got.dtype == out_dtype
                assert np.array_equal(as_bits(got), as_bits(w)), (name, mode, out_dtype)


def test_c_abi_direct_call(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 5
    gen = torch.Generator().manual_seed(23)
    host = [[draw(gen, s, torch.float32, INF) for s in sizes] for _ in range(n)]
    dev = [[t.to(hip_device) for t in row] for row in host]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        ptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        ptrs[2 * 2 + 1] = None  # client 2 did not send segment 1
        outs_t = [torch.empty(s, dtype=torch.float64, device=hip_device) for s in sizes]
        outs = (ctypes.c_void_p * 2)(*[o.data_ptr() for o in outs_t])
        ks = (ctypes.c_int32 * 2)(1, 1)
        stream = ctypes.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)
        st = lib.fedavg_robust_aggregate(ctx, ptrs, _native.F32, n, _native.ROBUST_TRIMMED_MEAN, ks, outs,
                                         _native.F64, stream)
        assert st == _native.OK, _native.last_error()
        flags = ctypes.c_uint32(99)
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        cols = [[row[0] for row in host], [row[1] for i, row in enumerate(host) if i != 2]]
        for o, col in zip(outs_t, cols):
            k = 1
            x = ref.sort_total_order(torch.stack([c.to(torch.float64) for c in col]))
            total = x[k].clone()
            for j in range(k + 1, len(col) - k):
                total = total + x[j]
            assert np.array_equal(as_bits(o), as_bits(total / float(len(col) - 2 * k)))
        # median ignores trim_k (NULL); invalid arguments are FEDAVG_ERR_INVALID with a message
        assert lib.fedavg_robust_aggregate(ctx, ptrs, _native.F32, n, _native.ROBUST_MEDIAN, None, outs,
                                           _native.F64, stream) == _native.OK
        assert lib.fedavg_check(ctx, stream, None) == _native.OK
        want = ref.reduce_tensor(cols[1], "median")
        assert np.array_equal(as_bits(outs_t[1]), as_bits(want))
        bad_k = (ctypes.c_int32 * 2)(1, 2)  # segment 1 has 4 clients: 2k = 4 keeps nothing
        for args in ((ptrs, _native.F32, n, 7, ks), (ptrs, _native.QSGD_F32, n, 0, ks), (ptrs, _native.F32, n, 0, bad_k),
                     (ptrs, _native.F32, n, 0, None), (None, _native.F32, n, 0, ks), (ptrs, _native.F32, 0, 0, ks)):
            st = lib.fedavg_robust_aggregate(ctx, args[0], args[1], args[2], args[3], args[4], outs, _native.F64, stream)
            assert st == _native.ERR_INVALID and _native.last_error()
        assert lib.fedavg_robust_aggregate(ctx, ptrs, _native.F32, n, 0, ks, outs, _native.F16, stream) == _native.ERR_INVALID
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_nan_input_raises_input_stage(hip_device):
    gen = torch.Generator().manual_seed(29)
    clients = [{"a": draw(gen, 600, torch.float16, INF)} for _ in range(4)]
    clients[2]["a"][577] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        _round(hip_device, clients, "median", 0.0)
    assert e.value.stage == "input" and e.value.bad_clients == [2]
    # a negative-signed NaN sorts to the other end: found as well
    neg = [{"a": torch.tensor([1.0, 2.0], dtype=torch.float64)} for _ in range(3)]
    neg[0]["a"] = torch.tensor([1.0, -float("nan")], dtype=torch.float64)
    neg[0]["a"].view(torch.int64)[1] |= -(2 ** 63)
    with pytest.raises(NaNAggregationError) as e:
        _round(hip_device, neg, "trimmed_mean", 0.34)
    assert e.value.stage == "input"


def test_both_infinities_kept_raises_result_stage(hip_device):
    a = torch.tensor([1.0, INF, 2.0], dtype=torch.float32)
    b = torch.tensor([1.0, -INF, 2.0], dtype=torch.float32)
    with pytest.raises(NaNAggregationError) as e:
        _round(hip_device, [{"a": a}, {"a": b}], "median", 0.0)
    assert e.value.stage == "result"
    with pytest.raises(NaNAggregationError) as e:
        _round(hip_device, [{"a": a}, {"a": b}, {"a": a}], "trimmed_mean", 0.0)
    assert e.value.stage == "result"
    # trimmed away, they are harmless — and the context is usable after the errors
    c = torch.tensor([3.0, 5.0, 6.0], dtype=torch.float32)
    d = torch.tensor([0.0, 7.0, 1.0], dtype=torch.float32)
    msg = _round(hip_device, [{"a": a}, {"a": b}, {"a": c}, {"a": d}], "trimmed_mean", 0.25)
    want = ref.reduce_tensor([a, b, c, d], "trimmed_mean", 0.25)
    assert np.array_equal(as_bits(msg.parameter["a"]), as_bits(want))


def test_65_clients_refused_without_a_launch(hip_device):
    layout = ModelLayout(names=("a",), shapes=((8,),))
    ctx = FedAvgContext(layout, hip_device)
    table = ClientTable(1)
    for _ in range(65):
        table.add_client([torch.ones(8, device=hip_device)], [1.0])
    out = [torch.full((8,), 5.0, dtype=torch.float64, device=hip_device)]
    with pytest.raises(NotImplementedError, match="64"):
        ctx.robust_aggregate(table, torch.float32, "median", 0.0, out)
    # the C ABI refuses it too, naming the limit
    p, _ = table.arrays()
    st = ctx._lib.fedavg_robust_aggregate(ctx._h, p.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)), _native.F32, 65,
                                          _native.ROBUST_MEDIAN, None, (ctypes.c_void_p * 1)(out[0].data_ptr()),
                                          _native.F64, ctx.stream)
    assert st == _native.ERR_INVALID and "64" in _native.last_error()
    with pytest.raises(ValueError, match="0 <= trim < 0.5"):
        ctx.robust_aggregate(table, torch.float32, "trimmed_mean", 0.5, out)
    torch.cuda.synchronize(hip_device)
    assert out[0].cpu().tolist() == [5.0] * 8  # nothing was launched
    ctx.close()


@settings(max_examples=25, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(n=st.integers(1, 64), sizes=st.lists(st.integers(1, 1300), min_size=1, max_size=4),
       code=st.sampled_from(list(DTYPES)), rule=st.sampled_from(RULES + [("trimmed_mean", 0.37)]),
       out32=st.booleans(), seed=st.integers(0, 2 ** 31 - 1), skip_every=st.integers(0, 6), drop_key=st.booleans(),
       poison=st.sampled_from(["none", "none", "none", "nan", "both_inf"]))
def test_random_rounds_match_restatement(hip_device, n, sizes, code, rule, out32, seed, skip_every, drop_key, poison):
    dtype, (mode, trim) = DTYPES[code], rule
    out_dtype = torch.float32 if out32 else torch.float64
    gen = torch.Generator().manual_seed(seed)
    clients: list = []
    for c in range(n):
        if skip_every and c % skip_every == skip_every - 1 and c != 0:
            clients.append(None)
            continue
        clients.append({f"t{i}": draw(gen, s, dtype, INF if (i + seed) % 2 else -INF) for i, s in enumerate(sizes)})
        if drop_key and len(sizes) > 1 and c % 3 == 1:
            del clients[-1]["t1"]
    if poison == "nan":
        clients[0]["t0"][sizes[0] // 2] = float("nan")
    elif poison == "both_inf":
        for c in clients:
            if c is not None:
                c["t0"][0] = INF
        clients[0]["t0"][0] = -INF
    try:
        want = ref.reduce_round(clients, mode, trim, out_dtype)
    except ref.RobustNaN as err:
        with pytest.raises(NaNAggregationError) as e:
            _round(hip_device, clients, mode, trim, out_dtype)
        assert e.value.stage == err.stage
        return
    msg = _round(hip_device, clients, mode, trim, out_dtype)
    assert list(msg.parameter) == list(want)
    for name, w in want.items():
        assert np.array_equal(as_bits(msg.parameter[name]), as_bits(w)), name
