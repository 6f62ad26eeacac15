"""The inputs of the sort kernels' contract suites can tell summation orders apart — shown with the
restatements alone (tests/robust_reference.py, tests/bulyan_reference.py), never with the code under
test. No GPU.

DESIGN.md §5g / §5k promise ``sum = s_k``, then ``sum = sum + s_j`` ascending, every add rounded in
fp64. For every (dtype, n, rule) that tests/test_gpu_robust_contract.py and
tests/test_gpu_mam_contract.py run on ``robust_values.wide_values`` the kept values are added three
ways here: ascending (the contract; asserted to be the restatement's own result, bit for bit),
descending, and as a pairwise tree. At least ``BAR`` = 10 % of the elements must differ in bits from
the ascending result for each alternative: a condition on the inputs, not a measurement. A kernel
that added in one of those orders would therefore fail the GPU suites in at least a tenth of its
elements.

Two kept values or fewer have one sum only (an add commutes): those rules — the median, ``keep = 2``
— are asserted to agree in all three orders, and say nothing about the order.

**fp16 inputs cannot reveal the order.** Sixty-four values of at most 65504 whose lowest bit is at
least 2^-24 span 46 bits, so every fp64 partial sum is exact in any order. For fp16 the tests below
assert exactly that — all three orders agree in every element — so that a passing fp16 case of the
GPU suites is not read as evidence for the order promise: for fp16 inputs it is vacuous.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import bulyan_reference as bref
from tests import robust_reference as rref
from tests import robust_values as rv

BAR = 0.10


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1).view(np.int64)


def ascending(kept: np.ndarray) -> np.ndarray:
    total = kept[0].copy()
    for j in range(1, len(kept)):
        total = total + kept[j]
    return total


def descending(kept: np.ndarray) -> np.ndarray:
    return ascending(kept[::-1])


def tree(kept: np.ndarray) -> np.ndarray:
    """A pairwise tree: the lower ``m // 2`` values and the rest are summed on their own and added.
    Three values give ``a + (b + c)``, four ``(a + b) + (c + d)``."""
    m = len(kept)
    if m == 1:
        return kept[0].copy()
    return tree(kept[: m // 2]) + tree(kept[m // 2:])


def fractions_differing(kept: np.ndarray) -> tuple[np.ndarray, float, float]:
    asc = ascending(kept)
    return asc, float((bits(descending(kept)) != bits(asc)).mean()), float((bits(tree(kept)) != bits(asc)).mean())


@functools.lru_cache(maxsize=None)
def columns(code: str, n: int) -> np.ndarray:
    """float64 [n, P]: the case's clients with their segments side by side."""
    rows = rv.order_rows(code, n, rv.order_sizes(code))
    return np.stack([torch.cat(r).numpy() for r in rows])


def check(code: str, kept: np.ndarray, what) -> None:
    asc, down, pair = fractions_differing(kept)
    print(f"{what}: kept {len(kept)}, descending differs in {down:.3f}, tree in {pair:.3f}")
    if code in rv.EXACT_CODES or len(kept) <= 2:
        assert down == 0.0 and pair == 0.0, what
    else:
        assert down >= BAR and pair >= BAR, (what, down, pair)


def test_wide_values_are_representable_and_full_width():
    gen = torch.Generator().manual_seed(1)
    for code, dtype in rv.DTYPES.items():
        v = rv.wide_values(gen, 4096, dtype)
        assert v.dtype == torch.float64 and bool((v.to(dtype).to(torch.float64) == v).all())
        lo, hi = rv.EXPONENTS[code]
        e = torch.floor(torch.log2(v.abs()))
        assert e.min() == lo and e.max() == hi and bool((v < 0).any()) and bool((v > 0).any())
        # the lowest mantissa bit of the format is set in about half of the values
        m = {"f32": 23, "f16": 10, "bf16": 7, "f64": 52}[code]
        odd = torch.remainder(v.abs() / torch.exp2(e) * 2.0 ** m, 2.0) == 1.0
        assert 0.4 < float(odd.double().mean()) < 0.6, code
    assert torch.finfo(torch.float16).max == 65504.0 and rv.EXPONENTS["f16"] == (-14, 15)


@pytest.mark.parametrize("code,n", rv.ORDER_CASES)
def test_kept_sum_orders_differ_on_the_order_cases(code, n):
    x = columns(code, n)
    s = rref.sort_total_order(torch.from_numpy(x)).numpy()
    for mode, trim in rv.ORDER_RULES:
        k = (n - 1) // 2 if mode == "median" else rref.trim_count(trim, n)
        kept = s[k: n - k]
        want = rref.reduce_tensor(list(torch.from_numpy(x)), mode, trim).numpy()
        assert np.array_equal(bits(ascending(kept) / np.float64(n - 2 * k)), bits(want)), (code, n, mode, trim)
        check(code, kept, (code, n, mode, trim))


@pytest.mark.parametrize("code,n", rv.ORDER_CASES)
def test_window_sum_orders_differ_on_the_order_cases(code, n):
    x = columns(code, n)
    s = bref.sort_total_order(x)
    cols = np.arange(x.shape[1])
    for keep in rv.order_keeps(n):
        lo = bref.window_by_shrinking(s, keep)
        kept = np.stack([s[lo + j, cols] for j in range(keep)])
        want = bref.mean_around_median(list(x), keep)
        assert np.array_equal(bits(ascending(kept) / np.float64(keep)), bits(want)), (code, n, keep)
        check(code, kept, (code, n, "keep", keep))


def test_fp16_sums_are_exact_by_construction():
    """The span argument of the module docstring on the generator's own values."""
    x = columns("f16", 64)
    assert np.abs(x).max() <= 65504.0
    assert (np.remainder(np.abs(x) * 2.0 ** 24, 1.0) == 0.0).all()        # multiples of 2^-24
    assert 64 * 65504.0 * 2.0 ** 24 < 2.0 ** 53                           # so every partial sum is exact


def test_distinct_columns():
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 64):
        x = rv.distinct_columns(rng, n, 300)
        assert x.shape == (n, 300) and x.dtype == np.float64
        assert (np.sort(x, axis=0) == (np.arange(1, n + 1.0) ** 2)[:, None]).all()
        if n == 64:
            assert len({tuple(c) for c in x.T}) == 300                    # the columns are permuted independently
    # not symmetric about its middle: the mean of the two ends is not the median
    assert (1 + 25) / 2 != 9


def test_pattern_tensors():
    for dtype, nans in ((torch.float16, 2046), (torch.bfloat16, 254)):
        t, replaced = rv.all_patterns_16(dtype)
        assert replaced == nans and t.dtype == dtype and t.numel() == 65536 and not bool(torch.isnan(t).any())
        b = t.view(torch.int16).to(torch.int32).numpy() & 0xFFFF
        keep = b == np.arange(65536)
        assert int((~keep).sum()) == nans and len(np.unique(b[keep])) == 65536 - nans
        assert bool(torch.isinf(t).sum() == 2) and bool((t == 0).sum() == 2)
    gen = torch.Generator().manual_seed(2)
    for dtype in (torch.float32, torch.float64):
        t, replaced = rv.random_patterns(gen, 8192, dtype)
        assert t.dtype == dtype and t.numel() == 8192 and not bool(torch.isnan(t).any())
        assert len(torch.unique(t.view(torch.int32 if dtype == torch.float32 else torch.int64))) > 8000
        assert replaced < 200      # 2^-8 (fp32) or 2^-11 (fp64) of all patterns are NaNs
