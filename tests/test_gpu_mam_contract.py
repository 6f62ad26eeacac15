"""The mean-around-median kernel (csrc/robust_kernels.hip, ``mam_tile_kernel``) against DESIGN.md
§5k: the order of the window sum, every rank of the sorting network through the write-back into the
staged bytes, every bit pattern of the 16-bit input formats through the key map and the narrowing of
``Sorted<T>::put``, and that nothing but the output elements is written — the client tensors in
particular, whose staged copy the kernel overwrites. Every comparison is bit for bit with
tests/bulyan_reference.py; no tolerance anywhere. The rotation of the table slots, which this entry
point shares with ``fedavg_robust_aggregate``, is in tests/test_gpu_robust_contract.py.

The order cases and their values are ``tests/robust_values``'; tests/test_robust_values_host.py
shows on the CPU that a descending or a pairwise sum of the same window differs from the contract's
ascending sum in at least a tenth of the elements — except for fp16 inputs, whose sums are exact in
any order: the fp16 cases here run for completeness and say nothing about the order.

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

from distributed_learning_simulation_lib_amd import FedAvgContext, _native
from tests import bulyan_reference as bref
from tests import robust_values as rv
from tests.robust_values import SENTINEL, Outs, assert_same_bits, bits, place
from tests.test_gpu_robust_contract import (CODES, DTYPES, NP_OUT, OUT_DTYPES, RANK_COUNTS, CContext, constant,
                                            isolation_case, layout_of, pattern_tensor, pattern_trio, pointer_table,
                                            rank_case, table_of)

pytestmark = pytest.mark.gpu


def f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().to(torch.float64).numpy()


# ---- C1. the window sum is added ascending --------------------------------------------------------
@pytest.mark.parametrize("code,n", rv.ORDER_CASES)
def test_window_sum_is_added_ascending(hip_device, code, n):
    dtype = DTYPES[code]
    sizes = rv.order_sizes(code, constant("mam_tile"), constant(f"mam_ae_{code}"))
    rows = rv.order_rows(code, n, sizes)
    last = len(sizes) - 1  # the last segment's storage is misaligned for every client
    dev = [[place(t.to(dtype), hip_device, i == last) for i, t in enumerate(r)] for r in rows]
    table = table_of(dev)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        for keep in rv.order_keeps(n):
            for out_dtype in OUT_DTYPES:
                outs = [torch.full((s,), SENTINEL, dtype=out_dtype, device=hip_device) for s in sizes]
                ctx.mean_around_median(table, dtype, keep, outs, out_dtype)
                assert ctx.flags() == 0
                for i, o in enumerate(outs):
                    want = bref.mean_around_median([r[i].numpy() for r in rows], keep, NP_OUT[out_dtype])
                    assert_same_bits(o, want, f"{code} n={n} keep={keep} out={out_dtype} segment {i}")
    finally:
        ctx.close()


# ---- C2. every rank of the network ----------------------------------------------------------------
@pytest.mark.parametrize("n", RANK_COUNTS)
@pytest.mark.parametrize("code", ["f32", "f64"])
def test_every_rank_through_the_write_back(hip_device, code, n):
    """Every element holds a permutation of 1, 4, 9, ..., n^2. ``keep = 1`` must return rank
    ``(n - 1) // 2`` exactly, ``keep = n`` the full (exact) sum divided once, and segment t with
    ``keep = n - 2t`` the restatement's window, which is not centred: the squares are not symmetric
    about their median."""
    x, dev, views, numel, S = rank_case(hip_device, code, n, constant("mam_tile"))
    out = torch.full((S * numel,), SENTINEL, dtype=torch.float64, device=hip_device)
    outs = (ctypes.c_void_p * S)(*[out[t * numel:(t + 1) * numel].data_ptr() for t in range(S)])
    c = CContext(hip_device, [numel] * S)
    try:
        def run(keeps):
            out.fill_(SENTINEL)
            st = c.lib.fedavg_mean_around_median(c.h, pointer_table(views), CODES[code], n, (ctypes.c_int32 * S)(*keeps),
                                                 outs, _native.F64, c.stream)
            assert st == _native.OK, _native.last_error()
            assert c.flags() == 0
            return out.cpu().numpy().reshape(S, numel)

        assert (run([1] * S) == float(((n - 1) // 2 + 1) ** 2)).all()
        assert (run([n] * S) == float(Fraction(sum(j * j for j in range(1, n + 1)), n))).all()
        got = run([n - 2 * t for t in range(S)])
        for t in range(S):
            want = bref.mean_around_median([x[r, t] for r in range(n)], n - 2 * t)
            assert_same_bits(got[t], want, f"{code} n={n} keep={n - 2 * t}")
    finally:
        c.close()


# ---- C3. every bit pattern through the key map and the narrowing ----------------------------------
@pytest.mark.parametrize("code", ["f16", "bf16"])
def test_all_16_bit_patterns_widen_exactly(hip_device, code):
    """n = 1, ``keep = 1``: every non-NaN pattern goes through the key map, back into its 16 staged
    bits and out as its exact fp64 widening — infinities, both zeros and subnormals included."""
    dtype = DTYPES[code]
    t = pattern_tensor(code)
    assert t.numel() == 65536 == 128 * constant("mam_tile")
    ctx = FedAvgContext(layout_of([t.numel()]), hip_device)
    try:
        out = [torch.full((t.numel(),), SENTINEL, dtype=torch.float64, device=hip_device)]
        ctx.mean_around_median(table_of([[t.to(hip_device)]]), dtype, 1, out)
        assert ctx.flags() == 0
        assert_same_bits(out[0], t.to(torch.float64), f"{code} widening")
    finally:
        ctx.close()


@pytest.mark.parametrize("code", list(DTYPES))
def test_patterns_through_key_map_sort_and_write_back(hip_device, code):
    dtype = DTYPES[code]
    trio = pattern_trio(pattern_tensor(code))
    numel = trio[0].numel()
    ctx = FedAvgContext(layout_of([numel]), hip_device)
    try:
        out = [torch.full((numel,), SENTINEL, dtype=torch.float64, device=hip_device)]
        ctx.mean_around_median(table_of([[t.to(hip_device)] for t in trio]), dtype, 2, out)
        assert ctx.flags() == 0
        assert_same_bits(out[0], bref.mean_around_median([f64(t) for t in trio], 2), f"{code} patterns keep=2")
    finally:
        ctx.close()


# ---- C4. nothing else is touched ------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("code", list(DTYPES))
def test_only_the_output_elements_are_written(hip_device, code, out_dtype, misalign):
    """The kernel overwrites its staged copy of the inputs with the sorted values; the client
    tensors themselves must come back with the bits they had."""
    dtype = DTYPES[code]
    sizes, rows, (who, seg, at), new = isolation_case(code, constant("mam_tile"), constant(f"mam_ae_{code}"))
    n = len(rows)
    dev = [[place(t.to(dtype), hip_device, misalign and i == 2) for i, t in enumerate(r)] for r in rows]
    before = [[bits(t).copy() for t in r] for r in dev]
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        def run(keep):
            outs = Outs(sizes, out_dtype, hip_device, misalign)
            ctx.mean_around_median(table_of(dev), dtype, keep, outs.views, out_dtype)
            assert ctx.flags() == 0
            assert outs.guards_untouched()
            return outs.numpy()

        for keep in (3, n):
            got = run(keep)
            for i in range(len(sizes)):
                assert_same_bits(got[i], bref.mean_around_median([r[i].numpy() for r in rows], keep, NP_OUT[out_dtype]),
                                 f"{code} keep={keep} segment {i}")
            for r, b in zip(dev, before):
                for t, w in zip(r, b):
                    assert np.array_equal(bits(t), w), "a client tensor changed"
        # one element of one client changes: exactly that output element follows (got: keep = n)
        changed = [[t.clone() for t in r] for r in rows]
        changed[who][seg][at] = new
        dev[who][seg][at] = new
        after = run(n)
        for i in range(len(sizes)):
            want = bref.mean_around_median([r[i].numpy() for r in changed], n, NP_OUT[out_dtype])
            assert_same_bits(after[i], want, f"{code} after the change, segment {i}")
            differs = np.flatnonzero(bits(after[i]) != bits(got[i])).tolist()
            assert differs == ([at] if i == seg else []), (i, differs)
    finally:
        ctx.close()
