"""The sparse delta fold (csrc/sparse_kernels.hip, ``fedavg_sparse_aggregate_delta``) against
DESIGN.md §5n: bit for bit against the numpy restatement (``tests/sparse_reference.fold``) and
against ``fedavg_aggregate_delta`` on the densified tensors; entry placement around every tile edge;
storage that is only element-aligned; signed zeros; the client order; the surroundings of every
output; reuse of one context with launches in flight on both table slots; the NaN flags; index
violations; and the refusals before any launch.

Sizes come from the build's own geometry (``fedavg_kernel_constant``: T = sparse_tile, B =
sparse_batch). The index-violation tests hand the kernel well-formed device buffers whose *contents*
break the ordering rule: the kernel's range check is what they exercise, every pointer is a whole
torch tensor or a view that ends inside its buffer, and 64 canary elements on both sides of every
output are checked to be untouched.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, SparseDelta, _native
from distributed_learning_simulation_lib_amd._staging import NativeClientTable
from distributed_learning_simulation_lib_amd.fedavg import OutputTable
from tests import robust_values
from tests import sparse_reference as ref
from tests.sparse_cases import assert_same_bits, random_sparse

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SENTINEL = 12345.0
CANARY = 64
OUT_DTYPES = (torch.float64, torch.float32)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def constant(name: str) -> int:
    return _native.kernel_constant(name)


def np_out(dtype: torch.dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def edge_sizes() -> list[int]:
    T = constant("sparse_tile")
    return [1, T - 1, T, T + 1, 2 * T + 3]


def client_counts() -> list[int]:
    B = constant("sparse_batch")
    return [1, 2, B, B + 1, 2 * B + 1]


def view_at(t: torch.Tensor, device, lead: int) -> torch.Tensor:
    """``t`` on the device as a contiguous view ``lead`` elements into a larger buffer."""
    buf = torch.empty(t.numel() + lead, dtype=t.dtype, device=device)
    buf[lead:].copy_(t)
    return buf[lead:]


def on_device(d: SparseDelta, device, misalign: bool = False) -> SparseDelta:
    if not misalign:
        return d.to(device)
    out = SparseDelta(view_at(d.indices, device, 1), view_at(d.values, device, 1), d.shape)
    assert d.nnz == 0 or (out.indices.data_ptr() % 16 != 0 and out.values.data_ptr() % 16 != 0)
    return out


class Outs:
    """One output view per segment inside a sentinel-filled buffer with CANARY elements before and
    after it; ``misalign``: the view starts at an odd element."""

    def __init__(self, sizes, dtype, device, misalign: bool = False) -> None:
        self.lead = CANARY + (1 if misalign else 0)
        self.bufs = [torch.full((self.lead + s + CANARY,), SENTINEL, dtype=dtype, device=device) for s in sizes]
        self.views = [b[self.lead:self.lead + s] for b, s in zip(self.bufs, sizes)]

    def canaries_untouched(self) -> bool:
        return all(bool((b[:self.lead] == SENTINEL).all()) and bool((b[-CANARY:] == SENTINEL).all())
                   for b in self.bufs)

    def numpy(self):
        return [v.cpu().numpy() for v in self.views]


def as_reference(rows):
    return [[(d.indices, d.values) for d in row] for row in rows]


def total(weights) -> float:
    return float(ref.total_weight(list(weights)))


def sparse_once(device, rows, weights, base, out_dtype, misalign=False, want_flags=0):
    """One sparse fold of host ``rows`` on a context of its own; the outputs as numpy."""
    sizes = [b.numel() for b in base]
    ctx = FedAvgContext(layout_of(sizes), device)
    try:
        dev = [[on_device(d, device, misalign) for d in row] for row in rows]
        z = [view_at(b, device, 1) if misalign else b.to(device) for b in base]
        outs = Outs(sizes, out_dtype, device, misalign)
        ctx.sparse_aggregate_delta(dev, weights, total(weights), z, outs.views, out_dtype)
        assert ctx.flags() == want_flags
        assert outs.canaries_untouched()
        return outs.numpy()
    finally:
        ctx.close()


def dense_once(device, rows, weights, base, out_dtype):
    """``fedavg_aggregate_delta`` on the densified tensors."""
    sizes = [b.numel() for b in base]
    ctx = FedAvgContext(layout_of(sizes), device)
    try:
        table = ClientTable(len(sizes))
        for row, w in zip(rows, weights):
            table.add_client([d.to_dense().reshape(-1).to(device) for d in row], [float(w)] * len(sizes))
        outs = [torch.empty(s, dtype=out_dtype, device=device) for s in sizes]
        ctx.aggregate_delta(table, rows[0][0].dtype, [b.to(device) for b in base], outs, out_dtype)
        assert ctx.flags() == 0
        return [o.cpu().numpy() for o in outs]
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def case(code: str):
    """The largest client count's rows over the edge sizes (about 5 % of the entries, at least one)
    and a float64 base; every smaller count reads the leading rows. Computed once, left unchanged."""
    sizes = edge_sizes()
    gen = torch.Generator().manual_seed(9000 + len(code) + ord(code[1]))
    rows = [[random_sparse(gen, s, max(1, s // 20), DTYPES[code]) for s in sizes] for _ in range(max(client_counts()))]
    base = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    weights = [float(w) for w in torch.rand(len(rows), generator=gen, dtype=torch.float64) * 9 + 0.5]
    return rows, weights, base


def check_all(device, rows, weights, base, what, misalign=False, dense=True):
    for out_dtype in OUT_DTYPES:
        want, flags = ref.fold(as_reference(rows), weights, total(weights), base, np_out(out_dtype))
        assert flags == 0
        got = sparse_once(device, rows, weights, base, out_dtype, misalign)
        for t, (g, w) in enumerate(zip(got, want)):
            assert_same_bits(g, w, f"{what} out={out_dtype} segment {t}: restatement")
        if dense:
            for t, (g, w) in enumerate(zip(got, dense_once(device, rows, weights, base, out_dtype))):
                assert_same_bits(g, w, f"{what} out={out_dtype} segment {t}: fedavg_aggregate_delta")


# ---- 1. bit for bit against the restatement and the dense delta fold ------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_equals_the_restatement_and_the_dense_delta_fold(hip_device, n):
    n = client_counts()[n]
    rows, weights, base = case("f32")
    check_all(hip_device, rows[:n], weights[:n], base, f"f32 n={n}")


@pytest.mark.parametrize("code", ["f16", "bf16", "f64"])
def test_every_value_dtype(hip_device, code):
    rows, weights, base = case(code)
    n = constant("sparse_batch") + 1
    check_all(hip_device, rows[:n], weights[:n], base, f"{code} n={n}")


def test_1024_clients_of_few_elements(hip_device):
    n = constant("sparse_max_clients")
    assert n == _native.POINT_MAX_CLIENTS == 1024
    gen = torch.Generator().manual_seed(5)
    rows = [[random_sparse(gen, 9, 2, torch.float32)] for _ in range(n)]
    base = [torch.randn(9, generator=gen, dtype=torch.float64)]
    weights = [float(1 + (i % 7)) for i in range(n)]
    check_all(hip_device, rows, weights, base, "1024 clients", dense=False)


# ---- 2. entry placement -----------------------------------------------------------------------------
def entries(numel: int, idx, gen) -> SparseDelta:
    idx = torch.tensor(sorted(idx), dtype=torch.int32)
    return SparseDelta(idx, torch.randn(idx.numel(), generator=gen) * 0.1, (numel,))


def test_entry_placement_around_the_tile_edges(hip_device):
    T = constant("sparse_tile")
    numel = 2 * T + 3
    gen = torch.Generator().manual_seed(31)
    base = [torch.randn(numel, generator=gen, dtype=torch.float64)]
    rows = [
        [entries(numel, [], gen)],                                      # nnz = 0 for one client
        [SparseDelta.dense(torch.randn(numel, generator=gen) * 0.1)],   # nnz = numel
        [entries(numel, [0, numel - 1], gen)],                          # the first and the last element only
        [entries(numel, [T - 1, T, 2 * T - 1, 2 * T], gen)],            # a tile's last element and the next one's first
        [entries(numel, range(T + 5, T + 400, 3), gen)],                # all inside one tile
        [entries(numel, [2 * T + 2], gen)],                             # the last, short tile only
    ]
    weights = [3.0, 0.25, 7.0, 1.5, 2.0, 0.125]
    check_all(hip_device, rows, weights, base, "placement")
    for k in range(len(rows)):                                          # and each of them alone
        check_all(hip_device, [rows[k]], [weights[k]], base, f"placement client {k} alone", dense=False)


def test_no_entries_at_all_is_the_weighted_base_not_the_base(hip_device):
    sizes = [constant("sparse_tile") + 7, 3]
    gen = torch.Generator().manual_seed(32)
    base = [robust_values.wide_values(gen, s, torch.float64) for s in sizes]
    rows = [[entries(s, [], gen) for s in sizes] for _ in range(3)]
    weights = [0.1, 0.7, 1 / 3]
    check_all(hip_device, rows, weights, base, "no entries")
    got = sparse_once(hip_device, rows, weights, base, torch.float64)
    assert any((g != b.numpy()).any() for g, b in zip(got, base))       # (b*w0 + b*w1 + b*w2) / W rounds


# ---- 3. storage that is only element-aligned ----------------------------------------------------------
@pytest.mark.parametrize("code", list(DTYPES))
def test_unaligned_storage(hip_device, code):
    """Index and value arrays one element into their buffers, base and outputs at an odd element."""
    rows, weights, base = case(code)
    n = constant("sparse_batch") + 1
    check_all(hip_device, rows[:n], weights[:n], base, f"unaligned {code}", misalign=True, dense=False)


# ---- 4. signed zeros -----------------------------------------------------------------------------------
def test_signed_zeros(hip_device):
    T = constant("sparse_tile")
    numel = T + 5
    base = [torch.full((numel,), -0.0, dtype=torch.float64)]
    at = [0, T - 1, T, numel - 1]
    neg = SparseDelta(torch.tensor(at, dtype=torch.int32), torch.full((4,), -0.0), (numel,))
    rows = [[neg], [neg], [neg]]
    weights = [1.0, 0.5, 2.0]
    for out_dtype in OUT_DTYPES:
        want, _ = ref.fold(as_reference(rows), weights, total(weights), base, np_out(out_dtype))
        got = sparse_once(hip_device, rows, weights, base, out_dtype)[0]
        assert_same_bits(got, want[0], "signed zeros")
        assert (got == 0).all()
        assert np.signbit(got[at]).all()                                 # -0.0 + -0.0 = -0.0 for every client
        rest = np.ones(numel, dtype=bool)
        rest[at] = False
        assert not np.signbit(got[rest]).any()                           # -0.0 + +0.0 = +0.0: no entry, no sign


# ---- 5. the client order ---------------------------------------------------------------------------------
def test_the_client_order_enters_the_result(hip_device):
    T = constant("sparse_tile")
    sizes = [T + 9]
    n = 2 * constant("sparse_batch") + 1
    gen = torch.Generator().manual_seed(33)
    base = [robust_values.wide_values(gen, sizes[0], torch.float64) * 1e-3]
    rows = []
    for _ in range(n):
        d = random_sparse(gen, sizes[0], sizes[0] // 2, torch.float32)
        rows.append([SparseDelta(d.indices, robust_values.wide_values(gen, d.nnz, torch.float32).to(torch.float32),
                                 d.shape)])
    weights = [float(w) for w in torch.rand(n, generator=gen, dtype=torch.float64) * 9 + 0.5]
    fwd = sparse_once(hip_device, rows, weights, base, torch.float64)[0]
    rev = sparse_once(hip_device, rows[::-1], weights[::-1], base, torch.float64)[0]
    want_fwd, _ = ref.fold(as_reference(rows), weights, total(weights), base)
    want_rev, _ = ref.fold(as_reference(rows[::-1]), weights[::-1], total(weights[::-1]), base)
    assert_same_bits(fwd, want_fwd[0], "arrival order")
    assert_same_bits(rev, want_rev[0], "reversed order")
    assert (fwd.view(np.int64) != rev.view(np.int64)).any()


# ---- 6. one context, many calls ----------------------------------------------------------------------------
def test_second_call_with_sparser_data_and_launches_in_flight_on_both_slots(hip_device):
    """The planes are left clean, and a call waits for the launch that still reads its table slot."""
    T, B = constant("sparse_tile"), constant("sparse_batch")
    sizes = [T + 3, 2 * T, 5]
    gen = torch.Generator().manual_seed(34)
    base = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    z = [b.to(hip_device) for b in base]
    calls = []
    for call, (n, frac) in enumerate([(B + 2, 2), (B + 2, 50), (3, 7), (2 * B, 3), (1, 1), (B, 400)]):
        rows = [[random_sparse(gen, s, max(1, s // frac), torch.float32) for s in sizes] for _ in range(n)]
        weights = [float(w) for w in torch.rand(n, generator=gen, dtype=torch.float64) + 0.5]
        calls.append((rows, weights))
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        # one after the other: a dense-ish call, then a sparser one
        for rows, weights in calls[:2]:
            outs = Outs(sizes, torch.float64, hip_device)
            ctx.sparse_aggregate_delta([[d.to(hip_device) for d in r] for r in rows], weights, total(weights), z,
                                       outs.views)
            want, _ = ref.fold(as_reference(rows), weights, total(weights), base)
            assert ctx.flags() == 0 and outs.canaries_untouched()
            for g, w in zip(outs.numpy(), want):
                assert_same_bits(g, w, "second call on one context")
        # back to back without a wait in between: both table slots have a launch in flight
        dev = [[[d.to(hip_device) for d in r] for r in rows] for rows, _ in calls]
        results = [Outs(sizes, torch.float64, hip_device) for _ in calls]
        for (rows, weights), d, outs in zip(calls, dev, results):
            ctx.sparse_aggregate_delta(d, weights, total(weights), z, outs.views, check_indices=False)
        assert not ctx.sparse_index_errors() and ctx.flags() == 0
        for k, ((rows, weights), outs) in enumerate(zip(calls, results)):
            want, _ = ref.fold(as_reference(rows), weights, total(weights), base)
            assert outs.canaries_untouched()
            for g, w in zip(outs.numpy(), want):
                assert_same_bits(g, w, f"call {k} of a burst")
    finally:
        ctx.close()


# ---- 7. the NaN flags -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan_value", "nan_base", "inf_minus_inf_in_x", "inf_and_minus_inf_clients"])
def test_nan_flags(hip_device, what):
    T = constant("sparse_tile")
    sizes = [T + 3, 5]
    gen = torch.Generator().manual_seed(35)
    rows = [[random_sparse(gen, s, max(2, s // 10), torch.float32) for s in sizes] for _ in range(3)]
    base = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    weights = [1.0, 0.5, 2.0]
    I, A, R = _native.FLAG_INPUT_NAN, _native.FLAG_ACC_NAN, _native.FLAG_RESULT_NAN
    assert (I, A, R) == (ref.FLAG_INPUT, ref.FLAG_ACC, ref.FLAG_RESULT)
    if what == "nan_value":
        rows[1][0].values[-1] = NAN
        want_flags = I | A | R
    elif what == "nan_base":
        base[1][2] = NAN
        want_flags = I | A | R
    elif what == "inf_minus_inf_in_x":
        base[0][int(rows[2][0].indices[0])] = INF
        rows[2][0].values[0] = -INF
        want_flags = I | A | R
    else:
        at = T + 1
        for k, v in ((0, INF), (2, -INF)):
            keep = rows[k][0].indices != at
            rows[k][0] = SparseDelta(torch.cat([rows[k][0].indices[keep], torch.tensor([at], dtype=torch.int32)]),
                                     torch.cat([rows[k][0].values[keep], torch.tensor([v])]), (sizes[0],))
            order = torch.argsort(rows[k][0].indices)
            rows[k][0] = SparseDelta(rows[k][0].indices[order], rows[k][0].values[order], (sizes[0],))
        want_flags = A | R
    want, ref_flags = ref.fold(as_reference(rows), weights, total(weights), base)
    assert ref_flags == want_flags
    got = sparse_once(hip_device, rows, weights, base, torch.float64, want_flags=want_flags)
    for t, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.isnan(g), np.isnan(w)), t
        assert_same_bits(g[~np.isnan(g)], w[~np.isnan(w)], f"{what}: the elements beside the NaN, segment {t}")
    assert sum(int(np.isnan(g).sum()) for g in got) == 1


# ---- 8. index violations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["duplicate", "descending", "negative", "numel", "far_outside"])
def test_index_violations_raise_and_write_nothing_outside_the_outputs(hip_device, what):
    T = constant("sparse_tile")
    sizes = [T + 3, 40]
    gen = torch.Generator().manual_seed(36)
    rows = [[random_sparse(gen, s, max(2, s // 10), torch.float32) for s in sizes] for _ in range(3)]
    base = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    weights = [1.0, 0.5, 2.0]
    good = [[d.to(hip_device) for d in r] for r in rows]
    bad_idx = rows[1][0].indices.clone()
    mid = bad_idx.numel() // 2
    if what == "duplicate":
        bad_idx[mid] = bad_idx[mid - 1]
    elif what == "descending":
        bad_idx[mid - 1], bad_idx[mid] = bad_idx[mid].item(), bad_idx[mid - 1].item()
    elif what == "negative":
        bad_idx[0] = -1
    elif what == "numel":
        bad_idx[-1] = sizes[0]
    else:
        bad_idx[0], bad_idx[-1] = -2**31, 2**31 - 1
    bad = [list(r) for r in good]
    bad[1][0] = SparseDelta(bad_idx.to(hip_device), rows[1][0].values.to(hip_device), (sizes[0],))
    z = [b.to(hip_device) for b in base]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        outs = Outs(sizes, torch.float64, hip_device)
        with pytest.raises(ValueError, match="strictly increasing"):
            ctx.sparse_aggregate_delta(bad, weights, total(weights), z, outs.views)
        torch.cuda.synchronize(hip_device)
        assert outs.canaries_untouched() and ctx.flags() == 0
        # the report cleared the word: the context folds well-formed deltas as before
        outs = Outs(sizes, torch.float64, hip_device)
        ctx.sparse_aggregate_delta(good, weights, total(weights), z, outs.views)
        want, _ = ref.fold(as_reference(rows), weights, total(weights), base)
        assert ctx.flags() == 0 and outs.canaries_untouched()
        for g, w in zip(outs.numpy(), want):
            assert_same_bits(g, w, f"after a refused call ({what})")
    finally:
        ctx.close()


# ---- 9. refusals before any launch -----------------------------------------------------------------------------------
def test_c_abi_direct_call_and_refusals(hip_device):
    lib = _native.load()
    sizes = [700, 3]
    n = 3
    gen = torch.Generator().manual_seed(37)
    rows = [[random_sparse(gen, s, max(1, s // 10), torch.float32) for s in sizes] for _ in range(n)]
    base = [torch.randn(s, generator=gen, dtype=torch.float64) for s in sizes]
    dev = [[d.to(hip_device) for d in r] for r in rows]
    z = [b.to(hip_device) for b in base]
    weights = [1.0, 0.0, 2.5]
    seg = (ctypes.c_int64 * 2)(*sizes)
    ctx = ctypes.c_void_p()
    assert lib.fedavg_ctx_create(ctypes.byref(ctx), hip_device.index, seg, 2, None) == _native.OK
    try:
        D, L, P = ctypes.c_double, ctypes.c_int64, ctypes.c_void_p
        iptr = (P * (n * 2))(*[d.indices.data_ptr() for r in dev for d in r])
        vptr = (P * (n * 2))(*[d.values.data_ptr() for r in dev for d in r])
        nnz = (L * (n * 2))(*[d.nnz for r in dev for d in r])
        ws = (D * n)(*weights)
        zptr = (P * 2)(*[t.data_ptr() for t in z])
        outs = [torch.full((s,), SENTINEL, dtype=torch.float64, device=hip_device) for s in sizes]
        optr = (P * 2)(*[o.data_ptr() for o in outs])
        stream = P(torch.cuda.current_stream(hip_device).cuda_stream)
        call, F32, F64 = lib.fedavg_sparse_aggregate_delta, _native.F32, _native.F64
        totals = (D * 2)()
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK
        before = bytes(totals)
        err = ctypes.c_int32(7)
        assert lib.fedavg_sparse_index_errors(ctx, stream, ctypes.byref(err)) == _native.OK and err.value == 0
        assert call(ctx, iptr, vptr, nnz, F32, ws, n, 3.5, zptr, optr, F64, stream) == _native.OK, _native.last_error()
        flags = ctypes.c_uint32(99)
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        assert lib.fedavg_sparse_index_errors(ctx, stream, ctypes.byref(err)) == _native.OK and err.value == 0
        want, _ = ref.fold(as_reference(rows), weights, 3.5, base)
        for o, w in zip(outs, want):
            assert_same_bits(o, w, "C ABI")
        assert lib.fedavg_total_weights(ctx, totals) == _native.OK and bytes(totals) == before   # state untouched
        for o in outs:
            o.fill_(SENTINEL)
        cap = _native.POINT_MAX_CLIENTS

        def table(src, at, value):
            t = (type(src))(*src)
            t[at] = value
            return t

        many_i = (P * ((cap + 1) * 2))(*([iptr[0], iptr[1]] * (cap + 1)))
        many_v = (P * ((cap + 1) * 2))(*([vptr[0], vptr[1]] * (cap + 1)))
        many_n = (L * ((cap + 1) * 2))(*([nnz[0], nnz[1]] * (cap + 1)))
        many_w = (D * (cap + 1))(*([1.0] * (cap + 1)))
        good = dict(i=iptr, v=vptr, z=nnz, dt=F32, w=ws, n=n, div=3.5, b=zptr, o=optr, ot=F64)
        bad = [dict(i=None), dict(v=None), dict(z=None), dict(w=None), dict(b=None), dict(o=None),
               dict(dt=_native.QSGD_F32), dict(dt=99), dict(ot=_native.F16), dict(ot=99),
               dict(n=0), dict(n=-1), dict(i=many_i, v=many_v, z=many_n, w=many_w, n=cap + 1),
               dict(i=table(iptr, 2, None)), dict(v=table(vptr, 3, None)),
               dict(i=table(iptr, 0, iptr[0] + 2)), dict(v=table(vptr, 0, vptr[0] + 2)),
               dict(z=table(nnz, 1, -1)), dict(z=table(nnz, 1, sizes[1] + 1)),
               dict(w=(D * n)(1.0, NAN, 1.0)), dict(w=(D * n)(1.0, 1.0, -INF)),
               dict(div=0.0), dict(div=-1.0), dict(div=INF), dict(div=NAN),
               dict(b=(P * 2)(zptr[0], None)), dict(b=(P * 2)(zptr[0] + 4, zptr[1])),
               dict(o=(P * 2)(optr[0], None)), dict(o=(P * 2)(optr[0] + 4, optr[1])),
               dict(o=(P * 2)(optr[0], zptr[1]))]
        for change in bad:
            a = {**good, **change}
            assert call(ctx, a["i"], a["v"], a["z"], a["dt"], a["w"], a["n"], a["div"], a["b"], a["o"], a["ot"],
                        stream) == _native.ERR_INVALID, change
            assert _native.last_error()
        assert call(None, iptr, vptr, nnz, F32, ws, n, 3.5, zptr, optr, F64, stream) == _native.ERR_INVALID
        assert lib.fedavg_sparse_index_errors(None, stream, ctypes.byref(err)) == _native.ERR_INVALID
        assert lib.fedavg_sparse_index_errors(ctx, stream, None) == _native.ERR_INVALID
        # NULL arrays are allowed where nnz == 0
        holed_i, holed_v, holed_n = table(iptr, 2, None), table(vptr, 2, None), table(nnz, 2, 0)
        torch.cuda.synchronize(hip_device)
        assert all(o.cpu().unique().tolist() == [SENTINEL] for o in outs)   # nothing was launched
        assert call(ctx, holed_i, holed_v, holed_n, F32, ws, n, 3.5, zptr, optr, F64, stream) == _native.OK
        assert lib.fedavg_check(ctx, stream, ctypes.byref(flags)) == _native.OK and flags.value == 0
        holed = [list(r) for r in rows]
        holed[1][0] = SparseDelta(torch.zeros(0, dtype=torch.int32), torch.zeros(0), (sizes[0],))
        want, _ = ref.fold(as_reference(holed), weights, 3.5, base)
        for o, w in zip(outs, want):
            assert_same_bits(o, w, "a NULL array with nnz = 0")
    finally:
        torch.cuda.synchronize(hip_device)
        lib.fedavg_ctx_destroy(ctx)


def test_python_refusals_without_a_launch(hip_device):
    sizes = [40, 3]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    gen = torch.Generator().manual_seed(38)
    row = [random_sparse(gen, s, 2, torch.float32).to(hip_device) for s in sizes]
    z = [torch.zeros(s, dtype=torch.float64, device=hip_device) for s in sizes]
    outs = Outs(sizes, torch.float64, hip_device)
    o = outs.views
    try:
        with pytest.raises(ValueError, match="no clients"):
            ctx.sparse_aggregate_delta([], [], 1.0, z, o)
        with pytest.raises(NotImplementedError, match="1024"):
            ctx.sparse_aggregate_delta([row] * 1025, [1.0] * 1025, 1.0, z, o)
        with pytest.raises(ValueError, match="client 0"):
            ctx.sparse_aggregate_delta([row[:1]], [1.0], 1.0, z, o)
        with pytest.raises(TypeError, match="SparseDelta"):
            ctx.sparse_aggregate_delta([[row[0], z[1]]], [1.0], 1.0, z, o)
        with pytest.raises(ValueError, match="client 0, tensor 1"):
            ctx.sparse_aggregate_delta([[row[0], row[0]]], [1.0], 1.0, z, o)
        with pytest.raises(ValueError, match="client 1, tensor 0"):
            ctx.sparse_aggregate_delta([row, [row[0].to("cpu"), row[1]]], [1.0, 1.0], 2.0, z, o)
        other = SparseDelta(row[1].indices, row[1].values.double(), row[1].shape)
        with pytest.raises(ValueError, match="one value dtype"):
            ctx.sparse_aggregate_delta([[row[0], other]], [1.0], 1.0, z, o)
        for w in ([1.0, 2.0], [NAN], [INF]):
            with pytest.raises(ValueError, match="weight"):
                ctx.sparse_aggregate_delta([row], w, 1.0, z, o)
        for div in (0.0, -2.0, INF, NAN):
            with pytest.raises(ValueError, match="divisor"):
                ctx.sparse_aggregate_delta([row], [1.0], div, z, o)
        with pytest.raises(TypeError):
            ctx.sparse_aggregate_delta([row], [1.0], 1.0, z, o, torch.float16)
        for bad in ([z[0]], [z[0], z[1].float()], [z[0], z[1].cpu()]):
            with pytest.raises(ValueError, match="base"):
                ctx.sparse_aggregate_delta([row], [1.0], 1.0, bad, o)
        for bad in ([o[0]], [o[0], o[1].float()]):
            with pytest.raises(ValueError, match="output"):
                ctx.sparse_aggregate_delta([row], [1.0], 1.0, z, bad)
        with pytest.raises(ValueError, match="in-place"):
            ctx.sparse_aggregate_delta([row], [1.0], 1.0, z, [o[0], z[1]])
        torch.cuda.synchronize(hip_device)
        assert all(bool((b == SENTINEL).all()) for b in outs.bufs) and ctx.flags() == 0
    finally:
        ctx.close()


def test_open_dynamic_wave_refuses_with_err_state(hip_device):
    layout = ModelLayout.flat(10_000)
    ctx = FedAvgContext(layout, hip_device)
    g = torch.Generator().manual_seed(6)
    host = [torch.randn(10_000, generator=g) for _ in range(3)]
    dev = [x.to(hip_device) for x in host]
    table = NativeClientTable(1, hip_device.index or 0)
    for x in dev:
        table.add_client([x], [1.0])
    out = torch.empty(10_000, dtype=torch.float64, device=hip_device)
    outs = OutputTable([out], layout, hip_device, torch.float64)
    rows = [[random_sparse(g, 10_000, 300, torch.float32)] for _ in range(3)]
    drows = [[d.to(hip_device) for d in r] for r in rows]
    zhost = torch.randn(10_000, generator=g, dtype=torch.float64)
    z = zhost.to(hip_device)
    res = torch.full((10_000,), SENTINEL, dtype=torch.float64, device=hip_device)
    weights = [1.0, 2.0, 3.0]
    try:
        ctx.dyn_open(torch.float32, 16)
        with pytest.raises(_native.NativeError) as e:
            ctx.sparse_aggregate_delta(drows, weights, 6.0, [z], [res])     # refused while the wave is open
        assert e.value.status == _native.ERR_STATE
        torch.cuda.current_stream(hip_device).synchronize()
        assert res.cpu().unique().tolist() == [SENTINEL]
        assert ctx.dyn_publish(table) == 3
        assert ctx.dyn_close(outs, torch.float64) == (3, True)
        ctx.raise_on_nan()
        ctx.sparse_aggregate_delta(drows, weights, 6.0, [z], [res])         # and accepted once it is closed
        ctx.raise_on_nan()
        want, _ = ref.fold(as_reference(rows), weights, 6.0, [zhost])
        assert_same_bits(res, want[0], "after the wave has closed")
    finally:
        ctx.close()
