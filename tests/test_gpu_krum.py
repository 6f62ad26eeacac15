"""The pairwise-distance kernel (csrc/krum_kernels.hip) and ``KrumFedAVGAlgorithm`` on the MI355X
against the torch-CPU restatement (tests/krum_reference.py; NOT a reference algorithm) and the
FedAvg oracle.

Sizes come from the build's own geometry (``fedavg_kernel_constant``): 1, one element short of a
16-byte vector, tile - 1 / tile / tile + 1, chunk + 1, and a segment whose storage starts one
element off a 16-byte boundary, all in one layout. Client counts sit on the register-block edges
(4, 15, 16, 17) and the 64-client block edges (63, 64, 65, 130, 256).

Tolerances. Integer inputs in [-32, 32] are exact in every input format and every difference,
square and partial sum is an exact integer below 2^53, so ``D`` is compared bit for bit. For
N(0, 1) inputs both the kernel and the restatement are within (P + 2) * 2^-53 relative of the
exact value (all terms are non-negative), so they differ by at most 2 * (P + 2) * 2^-53 * D_ref.
No input asks the kernel to read past a tensor.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from distributed_learning_simulation_lib_amd import (
    ClientTable,
    FedAvgContext,
    KrumFedAVGAlgorithm,
    ModelLayout,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import OutputTable
from oracle.fedavg_oracle import OracleFedAvg, OracleMessage
from tests import krum_reference as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
COUNTS = [1, 2, 3, 5, 4, 15, 16, 17, 63, 64, 65, 130]


def as_bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def edge_sizes(code: str) -> list[int]:
    """The last segment is the one stored misaligned."""
    tile = _native.kernel_constant("krum_tile")
    chunk = _native.kernel_constant("krum_chunk")
    ae = _native.kernel_constant(f"krum_ae_{code}")
    return [1, ae - 1, tile - 1, tile, tile + 1, chunk + 1, 2 * ae + 1]


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


def integers(gen, numel, dtype):
    return torch.randint(-32, 33, (numel,), generator=gen).to(dtype)


def gpu_distances(device, host, dtype, sizes, misalign_last=True, calls=1):
    layout = ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))
    ctx = FedAvgContext(layout, device)
    last = len(sizes) - 1
    table = ClientTable(len(sizes))
    for row in host:
        table.add_client([place(t, device, misalign_last and i == last) for i, t in enumerate(row)], [1.0] * len(sizes))
    try:
        outs = []
        for _ in range(calls):
            outs.append(ctx.pairwise_sqdist(table, dtype))
            ctx.raise_on_nan([(table, dtype)])
        return [o.cpu() for o in outs]
    finally:
        ctx.close()


def check_shape_of_d(D: torch.Tensor, n: int):
    assert D.dtype == torch.float64 and D.shape == (n, n)
    assert np.array_equal(as_bits(D), as_bits(D.t()))             # exactly symmetric
    assert not as_bits(torch.diagonal(D)).any()                   # +0.0, not -0.0


# ---- bit-exact on integers ------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_integer_inputs_are_bit_exact(hip_device, code, n):
    dtype, sizes = DTYPES[code], edge_sizes(code)
    gen = torch.Generator().manual_seed(1000 * n + len(code))
    host = [[integers(gen, s, dtype) for s in sizes] for _ in range(n)]
    (D,) = gpu_distances(hip_device, host, dtype, sizes)
    check_shape_of_d(D, n)
    assert np.array_equal(as_bits(D), as_bits(ref.distances(host)))


def test_256_clients_one_tiny_segment(hip_device):
    gen = torch.Generator().manual_seed(256)
    host = [[integers(gen, 5, torch.float32)] for _ in range(256)]
    (D,) = gpu_distances(hip_device, host, torch.float32, [5], misalign_last=False)
    check_shape_of_d(D, 256)
    assert np.array_equal(as_bits(D), as_bits(ref.distances(host)))


# ---- bounded on N(0, 1), and the same bits on every run ---------------------------------------
@pytest.mark.parametrize("n", [5, 17, 65])
@pytest.mark.parametrize("code", list(DTYPES))
def test_normal_inputs_within_the_contract_bound(hip_device, code, n):
    dtype, sizes = DTYPES[code], edge_sizes(code)
    gen = torch.Generator().manual_seed(77 * n + len(code))
    host = [[torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in sizes] for _ in range(n)]
    first, second = gpu_distances(hip_device, host, dtype, sizes, calls=2)
    check_shape_of_d(first, n)
    assert np.array_equal(as_bits(first), as_bits(second))
    want = ref.distances(host)
    bound = 2 * (sum(sizes) + 2) * 2.0 ** -53
    err = (first - want).abs()
    print("largest |D_gpu - D_ref| / D_ref:", (err / want.clamp_min(1e-300)).max().item(), "bound", bound)
    assert bool((err <= bound * want).all())


# ---- end to end ---------------------------------------------------------------------------
def _round(device, clients, f, m, weighted=False, out_dtype=torch.float64, on_device=True):
    algo = KrumFedAVGAlgorithm(f, m, weighted=weighted, device=device, out_dtype=out_dtype)
    for wid, c in enumerate(clients):
        if c is None:
            algo.process_worker_data(wid, None)
        else:
            p = {k: (v.to(device) if on_device else v) for k, v in c.items()}
            algo.process_worker_data(wid, ParameterMessage(parameter=p, aggregation_weight=wid + 1))
    return algo, algo.aggregate_worker_data()


def oracle_over(clients, rows, weights, out_dtype):
    o = OracleFedAvg()
    for r in rows:
        o.process_worker_data(r, OracleMessage(parameter={k: v.numpy() for k, v in clients[r].items()},
                                               aggregation_weight=weights[r]))
    np_dtype = np.float32 if out_dtype == torch.float32 else np.float64
    return {k: torch.from_numpy(np.asarray(v).astype(np_dtype)) for k, v in o.aggregate_parameter().items()}


@functools.lru_cache(maxsize=None)
def planted_round():
    """12 clients: 9 honest ones (a common model plus small noise) and f = 3 planted far away; one
    skipped worker in between. Computed once and left unchanged."""
    chunk = _native.kernel_constant("krum_chunk")
    shapes = {"w": (chunk + 3,), "b": (5,), "m": (3, 7), "scalar": ()}
    gen = torch.Generator().manual_seed(41)
    base = {k: torch.randn(s, generator=gen) for k, s in shapes.items()}
    clients: list = []
    for c in range(12):
        far = 3.0 if c in (1, 6, 10) else 0.0
        clients.append({k: base[k] + 0.01 * torch.randn(s, generator=gen) + far for k, s in shapes.items()})
    clients.insert(4, None)
    counted = [c for c in clients if c is not None]
    D = ref.distances([list(c.values()) for c in counted])
    P = sum(int(np.prod(s, dtype=np.int64)) for s in shapes.values())
    return clients, counted, D, P


@pytest.mark.parametrize("m", [1, 4, 9])
def test_algorithm_round_against_restatement_and_oracle(hip_device, m):
    clients, counted, D, P = planted_round()
    n, f = len(counted), 3
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    want_scores, want_rows = ref.select(D, f, m)
    # a condition on the inputs: the gap between the m-th and the (m + 1)-th score is larger than
    # what the distance bound can move a score by, so the bound cannot change the choice
    ranked = sorted(want_scores)
    finite = max(s for s in want_scores if s != INF)
    assert ranked[m] - ranked[m - 1] > 4 * n * (P + 2) * 2.0 ** -53 * finite
    for weighted in (False, True):
        for out_dtype in (torch.float64, torch.float32):
            algo, msg = _round(hip_device, clients, f, m, weighted, out_dtype)
            assert algo.last_selection.worker_ids == ids
            assert algo.last_selection.chosen == [ids[r] for r in want_rows]
            assert algo.skipped_workers == {4}
            ws = [float(ids[r] + 1) if weighted else 1.0 for r in range(n)]
            want = oracle_over(counted, want_rows, ws, out_dtype)
            assert list(msg.parameter) == list(want)
            for name, w in want.items():
                got = msg.parameter[name]
                assert got.device.type == "cuda" and got.dtype == out_dtype and got.shape == counted[0][name].shape
                assert np.array_equal(as_bits(got).reshape(-1), as_bits(w).reshape(-1)), (name, weighted, out_dtype)


def test_host_resident_updates_and_multi_krum_default(hip_device):
    clients, counted, D, _ = planted_round()
    algo, msg = _round(hip_device, clients, 3, None, on_device=False)   # m = n - f = 9
    ids = [wid for wid, c in enumerate(clients) if c is not None]
    assert algo.last_selection.chosen == [ids[r] for r in ref.select(D, 3, 9)[1]]
    assert set(algo.last_selection.chosen).isdisjoint({ids[1], ids[6], ids[10]})
    assert msg.parameter["w"].device.type == "cuda"


def test_duplicate_clients_tie_goes_to_the_earlier_arrival(hip_device):
    # five clients on a line at 5, 0, 0, 1, 9 (constant tensors of 40 integers): rows 1 and 2 tie
    clients = [{"a": torch.full((40,), x, dtype=torch.bfloat16)} for x in (5.0, 0.0, 0.0, 1.0, 9.0)]
    algo, msg = _round(hip_device, clients, 1, 1)
    assert algo.last_selection.scores == [40.0 * s for s in (16 + 16, 0 + 1, 0 + 1, 1 + 1, 16 + 64)]
    assert algo.last_selection.chosen == [1]
    assert not as_bits(msg.parameter["a"]).any()
    algo, _ = _round(hip_device, clients, 1, 2)
    assert algo.last_selection.chosen == [1, 2]


# ---- C ABI and errors -----------------------------------------------------------------------
def test_c_abi_direct_call_and_refusals(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 5
    gen = torch.Generator().manual_seed(23)
    host = [[integers(gen, s, torch.float32) for s in sizes] for _ in range(n)]
    dev = [[t.to(hip_device) for t in row] for row in host]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        ptrs = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        out = torch.full((n, n), 123.0, dtype=torch.float64, device=hip_device)
        optr = ctypes.c_void_p(out.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)
        assert lib.fedavg_pairwise_sqdist(ctx, ptrs, _native.F32, n, optr, stream) == _native.OK, _native.last_error()
        flags = ctypes.c_uint32(99)
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        assert np.array_equal(as_bits(out), as_bits(ref.distances(host)))
        # one client: a single +0.0
        one = torch.full((1,), 123.0, dtype=torch.float64, device=hip_device)
        assert lib.fedavg_pairwise_sqdist(ctx, ptrs, _native.F32, 1, ctypes.c_void_p(one.data_ptr()), stream) == _native.OK
        assert lib.fedavg_check(ctx, stream, None) == _native.OK
        assert as_bits(one).tolist() == [0]
        # refused before any launch, each with a message
        out.fill_(5.0)
        holed = (ctypes.c_void_p * (n * 2))(*[t.data_ptr() for row in dev for t in row])
        holed[2 * 2 + 1] = None
        many = (ctypes.c_void_p * (257 * 2))(*([dev[0][0].data_ptr(), dev[0][1].data_ptr()] * 257))
        for args in ((holed, _native.F32, n, optr), (many, _native.F32, 257, optr), (ptrs, _native.QSGD_F32, n, optr),
                     (ptrs, 99, n, optr), (None, _native.F32, n, optr), (ptrs, _native.F32, 0, optr),
                     (ptrs, _native.F32, n, None)):
            assert lib.fedavg_pairwise_sqdist(ctx, args[0], args[1], args[2], args[3], stream) == _native.ERR_INVALID
            assert _native.last_error()
        assert lib.fedavg_pairwise_sqdist(None, ptrs, _native.F32, n, optr, stream) == _native.ERR_INVALID
        torch.cuda.synchronize(hip_device)
        assert out.cpu().unique().tolist() == [5.0]  # nothing was launched
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_python_refusals_without_a_launch(hip_device):
    layout = ModelLayout(names=("a", "b"), shapes=((8,), (3,)))
    ctx = FedAvgContext(layout, hip_device)
    try:
        table = ClientTable(2)
        for _ in range(257):
            table.add_client([torch.ones(8, device=hip_device), torch.ones(3, device=hip_device)], [1.0, 1.0])
        with pytest.raises(NotImplementedError, match="256"):
            ctx.pairwise_sqdist(table, torch.float32)
        holed = ClientTable(2)
        holed.add_client([torch.ones(8, device=hip_device), torch.ones(3, device=hip_device)], [1.0, 1.0])
        holed.add_client([torch.ones(8, device=hip_device), None], [1.0, 0.0])
        with pytest.raises(ValueError, match="client 1 lacks tensor 1"):
            ctx.pairwise_sqdist(holed, torch.float32)
        with pytest.raises(ValueError):
            ctx.pairwise_sqdist(ClientTable(2), torch.float32)
        from distributed_learning_simulation_lib_amd.quantized import QSGD_F32

        with pytest.raises(NotImplementedError, match="dequantise"):
            ctx.pairwise_sqdist(holed, QSGD_F32)
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
            ctx.pairwise_sqdist(plain, torch.float32)   # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        torch.cuda.current_stream(hip_device).synchronize()
        assert ctx.dyn_publish(table) == 7
        assert ctx.dyn_close(outs, torch.float64) == (7, True)
        ctx.raise_on_nan()
        D = ctx.pairwise_sqdist(plain, torch.float32)    # and accepted once it is closed
        ctx.raise_on_nan()
        check_shape_of_d(D.cpu(), 7)
    finally:
        ctx.close()


def test_nan_and_infinity_flag_paths(hip_device):
    tile = _native.kernel_constant("krum_tile")
    gen = torch.Generator().manual_seed(29)

    def fresh():
        return [{"a": integers(gen, 3 * tile + 5, torch.float16), "b": integers(gen, 3, torch.float16)} for _ in range(5)]

    clients = fresh()
    clients[2]["a"][2 * tile + 1] = float("nan")
    with pytest.raises(NaNAggregationError) as e:
        _round(hip_device, clients, 1, 1)
    assert e.value.stage == "input" and e.value.bad_clients == [2]
    # a lone infinity is legal: that client's distances are +inf and it is never chosen
    clients = fresh()
    clients[3]["b"][1] = -INF
    algo, msg = _round(hip_device, clients, 1, 4)
    D = ref.distances([list(c.values()) for c in clients])
    assert D[3].tolist() == [INF, INF, INF, 0.0, INF]
    assert algo.last_selection.scores == ref.select(D, 1, 4)[0] and algo.last_selection.scores[3] == INF
    assert algo.last_selection.chosen == [0, 1, 2, 4]
    assert bool(torch.isfinite(msg.parameter["b"]).all())
    # the same infinity in the same element of two clients: inf - inf
    clients[0]["b"][1] = -INF
    with pytest.raises(NaNAggregationError) as e:
        _round(hip_device, clients, 1, 1)
    assert e.value.stage == "accumulator"
    # opposite signs are a distance of +inf; and the context is usable after the errors
    clients[0]["b"][1] = INF
    algo, _ = _round(hip_device, clients, 1, 1)
    D = ref.distances([list(c.values()) for c in clients])
    assert algo.last_selection.scores == ref.select(D, 1, 1)[0]
    assert algo.last_selection.chosen == ref.select(D, 1, 1)[1]


# ---- property test ---------------------------------------------------------------------------
@settings(max_examples=20, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(n=st.integers(1, 80), sizes=st.lists(st.integers(1, 1300), min_size=1, max_size=4),
       big=st.booleans(), code=st.sampled_from(list(DTYPES)), seed=st.integers(0, 2 ** 31 - 1), misalign=st.booleans())
def test_random_layouts_are_bit_exact(hip_device, n, sizes, big, code, seed, misalign):
    if big:  # one segment of more than a chunk
        sizes = sizes + [_native.kernel_constant("krum_chunk") + sizes[0]]
    dtype = DTYPES[code]
    gen = torch.Generator().manual_seed(seed)
    host = [[integers(gen, s, dtype) for s in sizes] for _ in range(n)]
    (D,) = gpu_distances(hip_device, host, dtype, sizes, misalign_last=misalign)
    check_shape_of_d(D, n)
    assert np.array_equal(as_bits(D), as_bits(ref.distances(host)))
