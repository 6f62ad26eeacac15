"""What tests/test_gpu_krum.py cannot see of the pairwise-distance kernel (csrc/krum_kernels.hip):
the summation order that DESIGN.md §5h promises, the ends of every input format's value range, the
state a context keeps between calls, the claim that the accumulator is not touched, and the NaN
flag at the positions that take another path through the kernel.

Every comparison is bit for bit, which needs inputs on which the reference is exact:

* ``ref.order_sensitive_values`` (exact squares, inexact running sums) against
  ``ref.distances_in_order``, the order of the contract restated in numpy. tests/test_krum_host.py
  establishes on these very layouts that the squares are exact and that another order (no chunk
  boundary, reversed chunk partials, two accumulators per chunk, torch's pairwise sum) gives other
  bits, so a pass here is not vacuous.
* integers in [-32, 32], scaled by a power of two where the value range is the subject: every
  difference, square and sum is exact, so ``D = ref.distances(integers) * 2^(2s)``.
* N(0, 1) only where two results of the kernel itself are compared, or against
  ``ref.distances_in_order_fused`` (the contract's order with the FMA's single rounding, in exact
  rational arithmetic) on a layout small enough for a Python loop.

Sizes come from the build's own geometry (``fedavg_kernel_constant``). No input asks the kernel to
read past a tensor: every pointer is a whole torch tensor or a view that ends inside its buffer.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    ClientTable,
    FedAvgContext,
    KrumFedAVGAlgorithm,
    ModelLayout,
    NaNAggregationError,
    ParameterMessage,
    _native,
)
from distributed_learning_simulation_lib_amd.algorithm.aggregation_algorithm import context_for
from tests import krum_reference as ref
from tests import robust_reference
from tests.test_gpu_krum import DTYPES, as_bits, check_shape_of_d, edge_sizes, integers, oracle_over, place

pytestmark = pytest.mark.gpu

INF = float("inf")


def constant(name: str) -> int:
    return _native.kernel_constant(name)


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def on_device(device, rows, dtype, misalign_last=True):
    """Every row's tensors on the device in ``dtype``; the last segment's storage misaligned."""
    last = len(rows[0]) - 1
    return [[place(t.to(dtype), device, misalign_last and i == last) for i, t in enumerate(row)] for row in rows]


def table_of(dev_rows, weights=None) -> ClientTable:
    T = len(dev_rows[0])
    table = ClientTable(T)
    for k, row in enumerate(dev_rows):
        table.add_client(row, [1.0 if weights is None else weights[k]] * T)
    return table


def distances_once(device, dev_rows, dtype, sizes) -> torch.Tensor:
    """``D`` of a fresh context, on the host; no flag may be latched."""
    ctx = FedAvgContext(layout_of(sizes), device)
    try:
        D = ctx.pairwise_sqdist(table_of(dev_rows), dtype)
        assert ctx.flags() == 0
        return D.cpu()
    finally:
        ctx.close()


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, what: str = "") -> None:
    """Equal as integer views; a failure names the first differing entry with both bit patterns."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = as_bits(got), as_bits(want)
    if np.array_equal(g, w):
        return
    at = tuple(int(v) for v in np.argwhere(g != w)[0])
    mask = (1 << (8 * g.dtype.itemsize)) - 1
    raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} entries differ in bits; first at {at}: "
                         f"got 0x{int(g[at]) & mask:x} ({got[at].item()!r}), want 0x{int(w[at]) & mask:x} ({want[at].item()!r})")


def exact_in(dtype, rows) -> bool:
    """A condition on the inputs: every float64 value is representable in ``dtype``, sign of zero
    included."""
    return all(np.array_equal(as_bits(t.to(dtype).to(torch.float64)), as_bits(t)) for row in rows for t in row)


# ---- 1. the summation order ------------------------------------------------------------------
def order_layout(code: str) -> list[int]:
    """The edge sizes plus a segment of three chunks; the last segment is the one stored misaligned."""
    return edge_sizes(code) + [2 * constant("krum_chunk") + 1]


@functools.lru_cache(maxsize=None)
def _order_rows(n: int, sizes: tuple) -> list:
    gen = torch.Generator().manual_seed(4242 + n)
    return [[ref.order_sensitive_values(gen, s) for s in sizes] for _ in range(n)]


def order_rows(n: int, sizes) -> list:
    """``n`` clients of ``ref.order_sensitive_values`` (float64; computed once and left unchanged)."""
    return _order_rows(n, tuple(sizes))


@functools.lru_cache(maxsize=None)
def _order_oracle(n: int, sizes: tuple) -> torch.Tensor:
    return ref.distances_in_order(_order_rows(n, sizes), constant("krum_chunk"))


@pytest.mark.parametrize("n", [5, 65, 130])
@pytest.mark.parametrize("code", list(DTYPES))
def test_summation_order_is_the_contracts(hip_device, code, n):
    dtype, sizes = DTYPES[code], order_layout(code)
    rows = order_rows(n, sizes)
    assert exact_in(dtype, rows)
    D = distances_once(hip_device, on_device(hip_device, rows, dtype), dtype, sizes)
    check_shape_of_d(D, n)
    assert_same_bits(D, _order_oracle(n, tuple(sizes)), f"{code}, n = {n}, sizes {sizes}")


def test_summation_order_follows_the_layout(hip_device):
    """The elements of the fp32, n = 5 case above cut into other segments: the chunk boundaries fall
    elsewhere, the restatement gives other bits, and the kernel follows it."""
    chunk, n = constant("krum_chunk"), 5
    sizes_a = order_layout("f32")
    P = sum(sizes_a)
    sizes_b = [chunk - 3, 5, P - chunk - 2]     # one whole chunk; a short one; two chunks and a tail
    flat = [torch.cat(r) for r in order_rows(n, sizes_a)]
    rows_b = [list(torch.split(x, sizes_b)) for x in flat]
    want_a, want_b = _order_oracle(n, tuple(sizes_a)), ref.distances_in_order(rows_b, chunk)
    differ = int((as_bits(want_a) != as_bits(want_b)).sum()) // 2
    print(f"layout {sizes_b} differs in bits from layout {sizes_a} in {differ} of {n * (n - 1) // 2} pairs")
    assert differ >= 1                           # a condition on the inputs
    D = distances_once(hip_device, on_device(hip_device, rows_b, torch.float32), torch.float32, sizes_b)
    check_shape_of_d(D, n)
    assert_same_bits(D, want_b, f"f32, n = {n}, sizes {sizes_b}")


# ---- 2. the bits do not depend on the client count ---------------------------------------------
@pytest.mark.parametrize("code", ["f32", "bf16"])
def test_bits_do_not_depend_on_the_client_count(hip_device, code):
    """A pair's distance is the same bits among 130 clients, where it may sit in an off-diagonal
    block pair or in a later block, and among 5 or 11, where it sits in block pair (0, 0)."""
    dtype, sizes, n = DTYPES[code], edge_sizes(code), 130
    gen = torch.Generator().manual_seed(130 + len(code))
    host = [[torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in sizes] for _ in range(n)]
    dev = on_device(hip_device, host, dtype)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        big = ctx.pairwise_sqdist(table_of(dev), dtype)
        assert ctx.flags() == 0
        big = big.cpu()
        check_shape_of_d(big, n)
        want = ref.distances(host)
        assert bool(((big - want).abs() <= 2 * (sum(sizes) + 2) * 2.0 ** -53 * want).all())
        for lo, hi in ((60, 71), (0, 5), (125, 130)):   # rows 60..70 straddle the first block edge
            small = ctx.pairwise_sqdist(table_of(dev[lo:hi]), dtype)
            assert ctx.flags() == 0
            small = small.cpu()
            check_shape_of_d(small, hi - lo)
            assert_same_bits(small, big[lo:hi, lo:hi].contiguous(), f"{code}, rows {lo}..{hi - 1} of {n}")
    finally:
        ctx.close()


# ---- 3. the ends of the value range --------------------------------------------------------------
SCALES = [("f16", -24), ("f16", 10), ("bf16", -133), ("bf16", 122), ("f32", -149), ("f32", 122),
          ("f64", -500), ("f64", 500), ("f64", -1074)]


def range_sizes(code: str) -> list[int]:
    ae = constant(f"krum_ae_{code}")
    return [ae - 1, constant("krum_tile") + 1, 2 * ae + 1]


def signed_integers(gen, numel) -> torch.Tensor:
    """float64 integers in [-32, 32]; about half of the zeros are -0.0."""
    x = integers(gen, numel, torch.float64)
    flip = torch.randint(0, 2, (numel,), generator=gen).bool() & (x == 0)
    x[flip] = -0.0
    return x


@pytest.mark.parametrize("code,s", SCALES)
def test_scaled_integers_are_bit_exact(hip_device, code, s):
    """Integers times 2^s: all subnormal at the low scale (fp16 2^-24, bf16 2^-133, fp32 2^-149),
    up to 2^15 / 2^127 at the high one; fp64 at 2^-500 and 2^500 (the largest sum stays below
    2^1024) and at 2^-1074, where every square underflows to +0.0. Nothing rounds, so
    ``D = ref.distances(integers) * 2^(2s)``."""
    dtype, sizes, n = DTYPES[code], range_sizes(code), 9
    gen = torch.Generator().manual_seed(1000 + 7 * s + len(code))
    ints = [[signed_integers(gen, sz) for sz in sizes] for _ in range(n)]
    for k, row in enumerate(ints):               # and planted: client k's -0.0 meets client k + 1's +0.0
        row[1][k], row[1][k + 1] = 0.0, -0.0
    assert all(bool((torch.signbit(row[1]) & (row[1] == 0)).any()) for row in ints)
    scaled = [[t * 2.0 ** s for t in row] for row in ints]
    assert all(bool(((t == 0) == (u == 0)).all()) for r, q in zip(ints, scaled) for t, u in zip(r, q))
    assert exact_in(dtype, scaled)               # nothing is lost on the way into the format
    if s == -1074:
        want = torch.zeros((n, n), dtype=torch.float64)
    else:
        want = ref.distances(ints) * 2.0 ** (2 * s)
        assert bool(torch.isfinite(want).all()) and bool((want.diagonal(1) > 0).all())
    D = distances_once(hip_device, on_device(hip_device, scaled, dtype), dtype, sizes)   # asserts flags() == 0
    check_shape_of_d(D, n)
    assert_same_bits(D, want, f"{code}, scale 2^{s}")


def test_fp64_square_overflow_is_infinity_not_an_error(hip_device):
    """(1e200)^2 overflows: that client's distances are +inf, no flag is raised (an infinity is not
    a NaN), and Krum never chooses it."""
    sizes, n, far = range_sizes("f64"), 9, 4
    gen = torch.Generator().manual_seed(200)
    host = [[integers(gen, sz, torch.float64) for sz in sizes] for _ in range(n)]
    host[far][1] = torch.full((sizes[1],), 1e200, dtype=torch.float64)
    dev = on_device(hip_device, host, torch.float64)
    D = distances_once(hip_device, dev, torch.float64, sizes)               # asserts flags() == 0
    check_shape_of_d(D, n)
    assert D[far].tolist() == [INF] * far + [0.0] + [INF] * (n - far - 1)
    assert_same_bits(D, ref.distances(host), "fp64 overflow")
    algo = KrumFedAVGAlgorithm(1, n - 1, device=hip_device)
    for wid, row in enumerate(dev):
        algo.process_worker_data(wid, ParameterMessage(parameter={f"t{i}": t for i, t in enumerate(row)},
                                                       aggregation_weight=1))
    msg = algo.aggregate_worker_data()
    assert algo.last_selection.chosen == [r for r in range(n) if r != far]
    assert algo.last_selection.scores[far] == INF
    assert all(bool(torch.isfinite(t).all()) for t in msg.parameter.values())


# ---- 4. one context, many calls --------------------------------------------------------------
def place_row(row, device, misalign_last: bool):
    """A client's tensors as views of one device buffer (one copy per client): every segment starts
    on a 16-byte boundary, the last one one element past it if ``misalign_last``. Every view ends
    inside the buffer."""
    esize = row[0].element_size()
    starts, at = [], 0
    for i, t in enumerate(row):
        at = (at + 15) // 16 * 16 + (1 if misalign_last and i == len(row) - 1 else 0)
        starts.append(at)
        at += t.numel()
    buf = torch.zeros(at, dtype=row[0].dtype)
    for st, t in zip(starts, row):
        buf[st:st + t.numel()] = t
    buf = buf.to(device)
    views = [buf[st:st + t.numel()] for st, t in zip(starts, row)]
    assert all(v.data_ptr() % 16 == 0 for v in views[:-1])
    assert (views[-1].data_ptr() % 16 == esize) == misalign_last
    return views


def test_one_context_many_calls(hip_device):
    """Client counts 5, 130, 5, 256, 17 on one context, three calls each without a host
    synchronisation in between: the slot-reuse wait (a slot's 3rd use), the workspace growing on a
    live context (1, 3, then 10 block pairs), both pointer-table slots growing (256 x 41 pointers
    are 82 KiB, above the 64 KiB they start with) and shrinking counts on the grown buffers. The
    rounds read different clients, and every result is kept until the end, so a late or a stale
    write would be seen. Odd clients store the chunk-sized segment misaligned."""
    dtype, ae, tile, chunk = torch.float16, constant("krum_ae_f16"), constant("krum_tile"), constant("krum_chunk")
    small = [1, ae - 1, ae + 1, tile + 1]
    sizes = [small[i % 4] for i in range(40)] + [chunk + 1]
    pool = 256
    gen = torch.Generator().manual_seed(404)
    host = [[integers(gen, s, dtype) for s in sizes] for _ in range(pool)]
    want = ref.distances(host)         # entry (i, j) reads clients i and j only: rounds take sub-matrices
    dev = [place_row(row, hip_device, k % 2 == 1) for k, row in enumerate(host)]
    rounds = [[(0 + i) % pool for i in range(5)], [(7 + i) % pool for i in range(130)],
              [(200 + i) % pool for i in range(5)], list(range(pool))[::-1], [(100 + i) % pool for i in range(17)]]
    assert len(sizes) * pool * 8 > 64 * 1024
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    kept = []
    try:
        for rows in rounds:
            table = table_of([dev[r] for r in rows])
            outs = [ctx.pairwise_sqdist(table, dtype) for _ in range(3)]
            ctx.raise_on_nan([(table, dtype)])
            kept.append((rows, outs))
        for rows, outs in kept:
            idx = torch.tensor(rows)
            for call, D in enumerate(outs):
                D = D.cpu()
                check_shape_of_d(D, len(rows))
                assert_same_bits(D, want[idx][:, idx].contiguous(), f"n = {len(rows)}, call {call}")
    finally:
        ctx.close()


# ---- 5. the accumulator is not touched -----------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float64, torch.float32])
def test_distances_between_accumulate_and_aggregate(hip_device, out_dtype):
    """A round folded in two waves gives the same bits with ``pairwise_sqdist`` (and
    ``robust_aggregate``, which fedavg_hip.h also documents as leaving the accumulator alone)
    called between the waves; the accumulator tensor itself and the total weights do not change."""
    chunk = constant("krum_chunk")
    sizes, n = [constant("krum_tile") + 1, chunk + 1, 3], 6
    weights = [float(k + 1) for k in range(n)]
    gen = torch.Generator().manual_seed(56)
    host = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(n)]
    dev = on_device(hip_device, host, torch.float32)
    first, last, everyone = table_of(dev[:3], weights[:3]), table_of(dev[3:], weights[3:]), table_of(dev, weights)

    def fresh_outs(dtype):
        return [torch.full((s,), 123.0, dtype=dtype, device=hip_device) for s in sizes]

    plain = FedAvgContext(layout_of(sizes), hip_device)
    try:
        plain.accumulate(first, torch.float32)
        want = fresh_outs(out_dtype)
        plain.aggregate(last, torch.float32, want, out_dtype)
        plain.raise_on_nan()
    finally:
        plain.close()

    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        ctx.accumulate(first, torch.float32)
        assert ctx.flags() == 0                      # synchronises
        acc_before, totals_before = ctx.accumulator.clone(), ctx.total_weights()
        assert bool((acc_before != 0).any())
        D = ctx.pairwise_sqdist(everyone, torch.float32)
        median = fresh_outs(torch.float64)
        ctx.robust_aggregate(everyone, torch.float32, "median", 0.0, median, torch.float64)
        assert ctx.flags() == 0
        assert_same_bits(ctx.accumulator, acc_before, "accumulator after pairwise_sqdist and robust_aggregate")
        assert ctx.total_weights() == totals_before
        got = fresh_outs(out_dtype)
        ctx.aggregate(last, torch.float32, got, out_dtype)
        ctx.raise_on_nan()
    finally:
        ctx.close()
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same_bits(g, w, f"aggregate, segment {i}, {out_dtype}")
    D = D.cpu()
    check_shape_of_d(D, n)
    assert_same_bits(D, ref.distances_in_order_fused(host, chunk), "D between the waves")
    for i, m in enumerate(median):
        assert_same_bits(m, robust_reference.reduce_tensor([row[i] for row in host], "median"), f"median, segment {i}")


# ---- 6. NaN and infinity positions ---------------------------------------------------------------
def nan_shapes(code: str) -> dict[str, int]:
    """``a``: a chunk and one element; ``b``: stored misaligned."""
    return {"a": constant("krum_chunk") + 1, "b": 2 * constant(f"krum_ae_{code}") + 1}


def nan_positions(code: str) -> list[tuple[str, int]]:
    chunk, shapes = constant("krum_chunk"), nan_shapes(code)
    return [("b", shapes["b"] - 1),   # the misaligned segment's last element: the guarded path
            ("a", chunk - 1),         # the first chunk's last full vector
            ("a", chunk)]             # the one-element second chunk: a short vector


def place_client(c: dict, device) -> dict:
    return {"a": place(c["a"], device, False), "b": place(c["b"], device, True)}


@functools.lru_cache(maxsize=None)
def nan_round(code: str, n: int):
    """Clean integer clients and what a round with f = 1, m = 3 gives: (clients, scores, chosen
    rows, the FedAvg oracle over the chosen). Computed once and left unchanged."""
    dtype, shapes = DTYPES[code], nan_shapes(code)
    gen = torch.Generator().manual_seed(600 + n + len(code))
    clients = [{k: integers(gen, s, dtype) for k, s in shapes.items()} for _ in range(n)]
    scores, rows = ref.select(ref.distances([list(c.values()) for c in clients]), 1, 3)
    wide = [{k: v.to(torch.float64) for k, v in c.items()} for c in clients]   # exact; the oracle reads numpy
    return clients, scores, rows, oracle_over(wide, rows, [1.0] * n, torch.float64)


def run_round(device, dev_clients, f, m):
    algo = KrumFedAVGAlgorithm(f, m, device=device)
    for wid, c in enumerate(dev_clients):
        algo.process_worker_data(wid, ParameterMessage(parameter=c, aggregation_weight=1))
    return algo, algo.aggregate_worker_data()


def check_clean_round(device, code, n, dev_clients):
    _, scores, rows, want = nan_round(code, n)
    algo, msg = run_round(device, dev_clients, 1, 3)
    assert algo.last_selection.scores == scores and algo.last_selection.chosen == rows
    for name, w in want.items():
        assert_same_bits(msg.parameter[name].reshape(-1), w.reshape(-1), f"clean round, {name}")


def poisoned(dev_clients, clients, bad, name, at, value, device):
    """The device clients with ``value`` at element ``at`` of tensor ``name`` of client ``bad``."""
    c = {k: v.clone() for k, v in clients[bad].items()}
    c[name][at] = value
    out = list(dev_clients)
    out[bad] = place_client(c, device)
    return out


@pytest.mark.parametrize("n,bad", [(70, 69), (130, 128), (5, 0)])
@pytest.mark.parametrize("code", list(DTYPES))
def test_nan_is_flagged_wherever_it_sits(hip_device, code, n, bad):
    """Client 69 of 70 is staged as the column side of block pair (0, 1) and in the diagonal pair
    (1, 1); 128 of 130 sits in the last block. After every error the next round on the same cached
    context is bit-exact: neither the flags nor the reset leak."""
    clients = nan_round(code, n)[0]
    dev_clients = [place_client(c, hip_device) for c in clients]
    layout = ModelLayout(names=tuple(nan_shapes(code)), shapes=tuple((s,) for s in nan_shapes(code).values()))
    ctx = context_for(layout, hip_device)
    check_clean_round(hip_device, code, n, dev_clients)
    for name, at in nan_positions(code):
        with pytest.raises(NaNAggregationError) as e:
            run_round(hip_device, poisoned(dev_clients, clients, bad, name, at, float("nan"), hip_device), 1, 3)
        assert e.value.stage == "input" and e.value.bad_clients == [bad], (name, at, e.value.stage, e.value.bad_clients)
        check_clean_round(hip_device, code, n, dev_clients)
    assert context_for(layout, hip_device) is ctx and ctx.flags() == 0


def test_negative_quiet_nan_with_payload_bf16(hip_device):
    code, n, bad = "bf16", 70, 69
    clients = nan_round(code, n)[0]
    dev_clients = [place_client(c, hip_device) for c in clients]
    nan = torch.tensor([0xFFC5 - 0x10000], dtype=torch.int16).view(torch.bfloat16)[0]   # sign, quiet bit, payload 5
    assert bool(torch.isnan(nan))
    name, at = nan_positions(code)[0]
    bad_clients = poisoned(dev_clients, clients, bad, name, at, nan, hip_device)
    assert bad_clients[bad][name].cpu().view(torch.int16)[at].item() == 0xFFC5 - 0x10000   # the bits arrive
    with pytest.raises(NaNAggregationError) as e:
        run_round(hip_device, bad_clients, 1, 3)
    assert e.value.stage == "input" and e.value.bad_clients == [bad]
    check_clean_round(hip_device, code, n, dev_clients)


@pytest.mark.parametrize("code", list(DTYPES))
def test_minus_infinity_in_a_column_only_client(hip_device, code):
    """-inf in client 69 of 70 (the short vector of the second chunk) is legal: no error, row 69
    is +inf off the diagonal, and with f = 1, m = 68 the client is not chosen."""
    dtype, n, bad = DTYPES[code], 70, 69
    clients = nan_round(code, n)[0]
    dev_clients = [place_client(c, hip_device) for c in clients]
    name, at = nan_positions(code)[2]
    with_inf = poisoned(dev_clients, clients, bad, name, at, -INF, hip_device)
    algo, msg = run_round(hip_device, with_inf, 1, 68)
    assert bad not in algo.last_selection.chosen and len(algo.last_selection.chosen) == 68
    assert algo.last_selection.scores[bad] == INF
    assert all(bool(torch.isfinite(t).all()) for t in msg.parameter.values())
    host = [[c["a"], c["b"]] for c in clients]
    host[bad] = [t.cpu() for t in with_inf[bad].values()]
    sizes = list(nan_shapes(code).values())
    D = distances_once(hip_device, [list(c.values()) for c in with_inf], dtype, sizes)   # asserts flags() == 0
    check_shape_of_d(D, n)
    assert D[bad].tolist() == [INF] * bad + [0.0]
    assert_same_bits(D, ref.distances(host), f"{code}, -inf in client {bad}")
    check_clean_round(hip_device, code, n, dev_clients)
