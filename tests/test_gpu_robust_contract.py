"""The trimmed-mean / median kernel (csrc/robust_kernels.hip, ``robust_tile_kernel``) and the host
half it shares with ``mam_tile_kernel`` against DESIGN.md §5g: the order of the kept sum, every rank
of the sorting network, every bit pattern of the 16-bit input formats through the key map, that
nothing but the output elements is written, and the rotation of the two table slots with launches
in flight. Every comparison is bit for bit with tests/robust_reference.py (tests/bulyan_reference.py
where the shared slots serve the mean around the median); no tolerance anywhere.

The order cases and their values are ``tests/robust_values``'; tests/test_robust_values_host.py
shows on the CPU that a descending or a pairwise sum of the same kept values differs from the
contract's ascending sum in at least a tenth of the elements — except for fp16 inputs, whose sums are
exact in any order: the fp16 cases here run for completeness and say nothing about the order.

Sizes come from the build's own geometry (``fedavg_kernel_constant``). No input asks the kernel to
read or write past a tensor: every pointer is a whole torch tensor or a view that ends inside its
buffer, and the elements around every output view are checked to be untouched.
"""

from __future__ import annotations

import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, _native
from tests import bulyan_reference as bref
from tests import robust_reference as rref
from tests import robust_values as rv
from tests.robust_values import SENTINEL, Outs, assert_same_bits, bits, place

pytestmark = pytest.mark.gpu

DTYPES = rv.DTYPES
OUT_DTYPES = (torch.float64, torch.float32)
NP_OUT = {torch.float64: np.float64, torch.float32: np.float32}
RANK_COUNTS = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]
CODES = {"f32": _native.F32, "f16": _native.F16, "bf16": _native.BF16, "f64": _native.F64}


def constant(name: str) -> int:
    return _native.kernel_constant(name)


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def table_of(dev_rows) -> ClientTable:
    T = len(dev_rows[0])
    table = ClientTable(T)
    for row in dev_rows:
        table.add_client(row, [1.0] * T)
    return table


# ---- C1. the kept sum is added ascending ----------------------------------------------------------
@pytest.mark.parametrize("code,n", rv.ORDER_CASES)
def test_kept_sum_is_added_ascending(hip_device, code, n):
    dtype = DTYPES[code]
    sizes = rv.order_sizes(code, constant("robust_tile"), constant(f"robust_ae_{code}"))
    rows = rv.order_rows(code, n, sizes)
    last = len(sizes) - 1  # the last segment's storage is misaligned for every client
    dev = [[place(t.to(dtype), hip_device, i == last) for i, t in enumerate(r)] for r in rows]
    table = table_of(dev)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        for mode, trim in rv.ORDER_RULES:
            for out_dtype in OUT_DTYPES:
                outs = [torch.full((s,), SENTINEL, dtype=out_dtype, device=hip_device) for s in sizes]
                ctx.robust_aggregate(table, dtype, mode, trim, outs, out_dtype)
                assert ctx.flags() == 0
                for i, o in enumerate(outs):
                    want = rref.reduce_tensor([r[i] for r in rows], mode, trim, out_dtype)
                    assert_same_bits(o, want, f"{code} n={n} {mode} {trim} out={out_dtype} segment {i}")
    finally:
        ctx.close()


# ---- C2. every rank of the network ----------------------------------------------------------------
def rank_case(device, code: str, n: int, tile: int):
    """One buffer per client cut into ``(n - 1) // 2 + 1`` segments of ``tile + 1`` elements (so
    the segments' alignment varies), every element a permutation of 1, 4, 9, ..., n^2."""
    numel, S = tile + 1, (n - 1) // 2 + 1
    x = rv.distinct_columns(np.random.default_rng(100 * n + len(code)), n, S * numel)
    dev = [torch.from_numpy(x[c]).to(DTYPES[code]).to(device) for c in range(n)]
    views = [[d[t * numel:(t + 1) * numel] for t in range(S)] for d in dev]
    for row in views:
        assert all(v.is_contiguous() and v.numel() == numel for v in row)
    return x.reshape(n, S, numel), dev, views, numel, S


class CContext:
    """A context of the C ABI over ``S`` segments of ``numel`` elements."""

    def __init__(self, device, sizes) -> None:
        self.lib = _native.load()
        self.h = ctypes.c_void_p()
        seg = (ctypes.c_int64 * len(sizes))(*sizes)
        assert self.lib.fedavg_ctx_create(ctypes.byref(self.h), device.index, seg, len(sizes), None) == _native.OK
        self.device = device
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def flags(self) -> int:
        f = ctypes.c_uint32(99)
        assert self.lib.fedavg_check(self.h, self.stream, ctypes.byref(f)) == _native.OK, _native.last_error()
        return f.value

    def close(self) -> None:
        torch.cuda.synchronize(self.device)
        self.lib.fedavg_ctx_destroy(self.h)


def pointer_table(views):
    return (ctypes.c_void_p * (len(views) * len(views[0])))(*[v.data_ptr() for row in views for v in row])


@pytest.mark.parametrize("n", RANK_COUNTS)
@pytest.mark.parametrize("code", ["f32", "f64"])
def test_every_rank_with_every_trim_in_one_launch(hip_device, code, n):
    """Segment t drops t values at each end, so one launch carries every legal k. The kept values
    are (k + 1)^2 .. (n - k)^2 whatever the permutation: the result is their exact sum divided once.
    Successive segments differ by s_k + s_{n-k-1}, so a value sorted to a wrong rank shows."""
    x, dev, views, numel, S = rank_case(hip_device, code, n, constant("robust_tile"))
    out = torch.full((S * numel,), SENTINEL, dtype=torch.float64, device=hip_device)
    out_views = [out[t * numel:(t + 1) * numel] for t in range(S)]
    c = CContext(hip_device, [numel] * S)
    try:
        ks = (ctypes.c_int32 * S)(*range(S))
        outs = (ctypes.c_void_p * S)(*[v.data_ptr() for v in out_views])
        st = c.lib.fedavg_robust_aggregate(c.h, pointer_table(views), CODES[code], n, _native.ROBUST_TRIMMED_MEAN, ks, outs,
                                           _native.F64, c.stream)
        assert st == _native.OK, _native.last_error()
        assert c.flags() == 0
        got = out.cpu().numpy().reshape(S, numel)
        for t in range(S):
            closed = float(Fraction(sum(j * j for j in range(t + 1, n - t + 1)), n - 2 * t))
            assert (got[t] == closed).all(), (n, t, closed, got[t][got[t] != closed][:4])
            trim = (t + 0.25) / n
            assert rref.trim_count(trim, n) == t
            want = rref.reduce_tensor([torch.from_numpy(x[r, t]) for r in range(n)], "trimmed_mean", trim)
            assert_same_bits(got[t], want.numpy(), f"{code} n={n} k={t}")
        # the median is the same kernel with k = (n - 1) // 2 in every segment
        out.fill_(SENTINEL)
        st = c.lib.fedavg_robust_aggregate(c.h, pointer_table(views), CODES[code], n, _native.ROBUST_MEDIAN, None, outs,
                                           _native.F64, c.stream)
        assert st == _native.OK, _native.last_error()
        assert c.flags() == 0
        mid = (n // 2 + 1) ** 2 if n % 2 else ((n // 2) ** 2 + (n // 2 + 1) ** 2) / 2.0
        assert (out.cpu().numpy() == float(mid)).all()
    finally:
        c.close()


# ---- C3. every bit pattern through the key map ----------------------------------------------------
def pattern_tensor(code: str) -> torch.Tensor:
    if code in ("f16", "bf16"):
        t, replaced = rv.all_patterns_16(DTYPES[code])
        assert replaced == {"f16": 2046, "bf16": 254}[code]
    else:
        t, _ = rv.random_patterns(torch.Generator().manual_seed(77), 8192, DTYPES[code])
    return t


def pattern_trio(t: torch.Tensor) -> list[torch.Tensor]:
    """The patterns, the same reversed and the same rolled: every pattern meets unrelated ones in
    its column and sits beside unrelated neighbours in its 32-bit word."""
    return [t, t.flip(0).contiguous(), t.roll(4099).contiguous()]


@pytest.mark.parametrize("code", ["f16", "bf16"])
def test_all_16_bit_patterns_widen_exactly(hip_device, code):
    """n = 1: the median of one value is the value, so the output is the exact fp64 widening of
    every non-NaN pattern — infinities, zeros of both signs and subnormals included."""
    dtype = DTYPES[code]
    t = pattern_tensor(code)
    assert t.numel() == 65536 == 128 * constant("robust_tile")
    ctx = FedAvgContext(layout_of([t.numel()]), hip_device)
    try:
        table = table_of([[t.to(hip_device)]])
        out = [torch.full((t.numel(),), SENTINEL, dtype=torch.float64, device=hip_device)]
        ctx.robust_aggregate(table, dtype, "median", 0.0, out)
        assert ctx.flags() == 0
        assert_same_bits(out[0], t.to(torch.float64), f"{code} widening")
    finally:
        ctx.close()


@pytest.mark.parametrize("code", list(DTYPES))
def test_patterns_through_key_map_and_sort(hip_device, code):
    dtype = DTYPES[code]
    trio = pattern_trio(pattern_tensor(code))
    numel = trio[0].numel()
    ctx = FedAvgContext(layout_of([numel]), hip_device)
    try:
        table = table_of([[t.to(hip_device)] for t in trio])
        for mode in ("median", "trimmed_mean"):
            out = [torch.full((numel,), SENTINEL, dtype=torch.float64, device=hip_device)]
            ctx.robust_aggregate(table, dtype, mode, 0.0, out)
            assert ctx.flags() == 0
            assert_same_bits(out[0], rref.reduce_tensor(trio, mode, 0.0), f"{code} patterns {mode}")
    finally:
        ctx.close()


# ---- C4. nothing else is touched ------------------------------------------------------------------
def isolation_case(code: str, tile: int, ae: int):
    """Five clients of wide values over [ae + 1, tile + 3, tile - 1] elements, and the replacement
    for client 2's element ``tile + 1`` of segment 1: far above every sum of the others."""
    sizes = [ae + 1, tile + 3, tile - 1]
    gen = torch.Generator().manual_seed(500 + len(code) + ord(code[1]))
    rows = [[rv.wide_values(gen, s, DTYPES[code]) for s in sizes] for _ in range(5)]
    new = 2.0 ** 15 if code == "f16" else 2.0 ** 60
    return sizes, rows, (2, 1, tile + 1), new


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("code", list(DTYPES))
def test_only_the_output_elements_are_written(hip_device, code, out_dtype, misalign):
    dtype = DTYPES[code]
    sizes, rows, (who, seg, at), new = isolation_case(code, constant("robust_tile"), constant(f"robust_ae_{code}"))
    dev = [[place(t.to(dtype), hip_device, misalign and i == 2) for i, t in enumerate(r)] for r in rows]
    before = [[bits(t).copy() for t in r] for r in dev]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        def run(mode, trim):
            outs = Outs(sizes, out_dtype, hip_device, misalign)
            ctx.robust_aggregate(table_of(dev), dtype, mode, trim, outs.views, out_dtype)
            assert ctx.flags() == 0
            assert outs.guards_untouched()
            return outs.numpy()

        for mode, trim in (("median", 0.0), ("trimmed_mean", 0.0)):
            got = run(mode, trim)
            for i in range(len(sizes)):
                assert_same_bits(got[i], rref.reduce_tensor([r[i] for r in rows], mode, trim, out_dtype).numpy(),
                                 f"{code} {mode} segment {i}")
            for r, b in zip(dev, before):
                for t, w in zip(r, b):
                    assert np.array_equal(bits(t), w), "a client tensor changed"
        # one element of one client changes: exactly that output element follows (got: the mean)
        changed = [[t.clone() for t in r] for r in rows]
        changed[who][seg][at] = new
        dev[who][seg][at] = new
        want = [rref.reduce_tensor([r[i] for r in changed], "trimmed_mean", 0.0, out_dtype).numpy() for i in range(len(sizes))]
        after = run("trimmed_mean", 0.0)
        for i in range(len(sizes)):
            assert_same_bits(after[i], want[i], f"{code} after the change, segment {i}")
            differs = np.flatnonzero(bits(after[i]) != bits(got[i])).tolist()
            assert differs == ([at] if i == seg else []), (i, differs)
    finally:
        ctx.close()


# ---- C5. the two table slots with launches in flight ----------------------------------------------
def test_five_tables_back_to_back_without_a_synchronisation(hip_device):
    """``upload_tables`` rotates two pinned slots between ``fedavg_robust_aggregate`` and
    ``fedavg_mean_around_median`` and waits on the event of the launch that last read a slot. Five
    calls with five different tables — other client counts, so other network widths, and other
    absent entries, so other per-segment counts and pointer lists — are issued with nothing between
    them that reads a flag or synchronises; a call that overwrote a slot before the launch reading
    it had finished would hand that launch another call's pointers. All five are checked at the end."""
    tile, ae = constant("robust_tile"), constant("robust_ae_f32")
    sizes = [tile + 1, 7, ae + 1, 2 * tile + 5]
    T = len(sizes)
    specs = [  # clients, absent {segment: clients}, entry point, rule
        (3, {}, "robust", ("trimmed_mean", 0.0)),
        (17, {1: {0, 5}, 3: {16}}, "mam", [9, 2, 17, 16]),
        (64, {0: set(range(1, 64, 2))}, "robust", ("median", 0.0)),
        (2, {2: {1}}, "mam", [2, 1, 1, 2]),
        (33, {1: set(range(3, 33)), 2: {0}}, "robust", ("trimmed_mean", 0.25)),
    ]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        cases = []
        for i, (n, absent, kind, rule) in enumerate(specs):
            gen = torch.Generator().manual_seed(900 + i)
            rows = [[rv.wide_values(gen, s, torch.float32) for s in sizes] for _ in range(n)]
            table = ClientTable(T)
            for c, r in enumerate(rows):
                table.add_client([None if c in absent.get(t, ()) else r[t].to(torch.float32).to(hip_device)
                                  for t in range(T)], [1.0] * T)
            cols = [[r[t] for c, r in enumerate(rows) if c not in absent.get(t, ())] for t in range(T)]
            if kind == "robust":
                want = [rref.reduce_tensor(col, *rule).numpy() for col in cols]
            else:
                want = [bref.mean_around_median([v.numpy() for v in col], rule[t]) for t, col in enumerate(cols)]
            outs = Outs(sizes, torch.float64, hip_device, False)
            cases.append((table, kind, rule, outs, want))
        torch.cuda.synchronize(hip_device)
        for table, kind, rule, outs, _ in cases:        # back to back: no flag read, no synchronise
            if kind == "robust":
                ctx.robust_aggregate(table, torch.float32, rule[0], rule[1], outs.views)
            else:
                ctx.mean_around_median(table, torch.float32, rule, outs.views)
        assert ctx.flags() == 0
        for i, (_, kind, rule, outs, want) in enumerate(cases):
            assert outs.guards_untouched()
            for t, got in enumerate(outs.numpy()):
                assert_same_bits(got, want[t], f"call {i} ({kind} {rule}), segment {t}")
    finally:
        ctx.close()


def test_a_slot_regrows_while_the_other_is_being_read(hip_device):
    """A slot is freed and regrown when a call's tables outgrow it. From the source: a slot starts
    at 64 KiB (``upload_tables``), a call's tables are ``sizeof(RSeg)`` = 32 bytes per segment (a
    pointer, four int32, one int64) plus 8 bytes per client pointer. With 140 segments, two clients
    need 140 * (32 + 16) = 6720 bytes — both slots stay at their first size — and 64 clients need
    140 * (32 + 512) = 76160 bytes > 65536: the slot regrows (any count from 121 segments up would
    do). Two calls at n = 2 allocate both slots; then, with no synchronisation, three calls at
    n = 64 regrow one slot while the launch reading the other is in flight, regrow the other, and
    reuse the first; then two calls at n = 2 reuse the grown slots. The entry points alternate.
    Everything is checked at the end."""
    S, nmax = 140, 64
    sizes = [1 + t % 3 for t in range(S)]
    assert S * (32 + 8 * nmax) > 64 * 1024 > S * (32 + 8 * 2)
    offs = [0] + [int(v) for v in np.cumsum(sizes)]
    gen = torch.Generator().manual_seed(31)
    host = [rv.wide_values(gen, offs[-1], torch.float64) for _ in range(nmax)]
    dev = [h.to(hip_device) for h in host]
    views = [[d[offs[t]:offs[t + 1]] for t in range(S)] for d in dev]
    plan = [(2, "robust"), (2, "mam"), (64, "robust"), (64, "mam"), (64, "robust"), (2, "mam"), (2, "robust")]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        cases = []
        for i, (n, kind) in enumerate(plan):
            first = (7 * i) % (nmax - n + 1)          # other clients in every call
            who = list(range(first, first + n))
            x = [host[c].numpy() for c in who]
            if kind == "robust":
                want = rref.reduce_tensor([host[c] for c in who], "trimmed_mean", 0.0).numpy()
            else:
                want = bref.mean_around_median(x, n)
            out = torch.full((offs[-1] + 2,), SENTINEL, dtype=torch.float64, device=hip_device)
            cases.append((table_of([views[c] for c in who]), n, kind, out, want))
        torch.cuda.synchronize(hip_device)
        for table, n, kind, out, _ in cases:             # back to back: no flag read, no synchronise
            outs = [out[1 + offs[t]:1 + offs[t + 1]] for t in range(S)]
            if kind == "robust":
                ctx.robust_aggregate(table, torch.float64, "trimmed_mean", 0.0, outs)
            else:
                ctx.mean_around_median(table, torch.float64, n, outs)
        assert ctx.flags() == 0
        for i, (_, n, kind, out, want) in enumerate(cases):
            got = out.cpu().numpy()
            assert got[0] == SENTINEL and got[-1] == SENTINEL
            assert_same_bits(got[1:-1], want, f"call {i} (n = {n}, {kind})")
    finally:
        ctx.close()
