"""Inputs for the contract suites of the two sort kernels (csrc/robust_kernels.hip): generators in
plain numpy / torch, and the list of cases that the order tests run. Test support only (no test in
this file); nothing is imported from the package.

* ``wide_values``: values whose plain fp64 sums round, so that the order of the adds shows in the
  bits. tests/test_robust_values_host.py proves with the restatements alone that a descending sum
  and a pairwise tree differ from the ascending (contract) sum on these values, for every case of
  ``ORDER_CASES``; the GPU suites run exactly those cases.
* ``distinct_columns``: per element a permutation of n distinct integers, so that every rank of the
  sorting network holds its own value and every sum is exact.
* ``all_patterns_16`` / ``random_patterns``: bit patterns of the input formats, NaNs replaced.
"""

from __future__ import annotations

import numpy as np
import torch

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}

# Exponent range of ``wide_values``. The kept values of one element must span more than the 53 bits
# of an fp64 mantissa before an add rounds at all: a 24-bit (fp32) or 8-bit (bf16) mantissa needs a
# wide spread of exponents, a 53-bit one (fp64) rounds within a few binades. fp16 gets every normal
# exponent — and still cannot round (see ``EXACT_CODES``).
EXPONENTS = {"f32": (-40, 40), "bf16": (-60, 60), "f64": (-2, 2), "f16": (-14, 15)}
# fp16: 64 values of at most 65504 whose lowest set bit is at least 2^-24 (the normal range; the
# generator draws no subnormal) — every partial sum is a multiple of 2^-24 below 2^22, 46 bits, and
# is exact in fp64 whatever the order. The order promise is vacuous for fp16 inputs.
EXACT_CODES = ("f16",)

# The cases of the order tests: client counts on both sides of the 16- and 32-wide networks and the
# widest one; the host test holds the inputs to its 10 % condition at every one of them. bf16's
# 8-bit mantissas need more kept values before a tenth of the sums round differently: with a
# quarter trimmed at each end 16 or 17 clients reach 5 to 7 % only (measured with the restatement,
# at this and at wider and narrower exponent ranges), so its counts start at 32.
ORDER_COUNTS = {"f32": (16, 17, 32, 33, 64), "f16": (16, 17, 32, 33, 64), "bf16": (32, 33, 63, 64),
                "f64": (16, 17, 32, 33, 64)}
ORDER_RULES = (("trimmed_mean", 0.0), ("trimmed_mean", 0.1), ("trimmed_mean", 0.25), ("median", 0.0))
ORDER_CASES = tuple((code, n) for code in DTYPES for n in ORDER_COUNTS[code])
# segment sizes of the documented geometry (tile 512, 16 bytes per lane and pass):
# [ae + 1, tile - 1, tile + 1]; the GPU suites take theirs from the built library
DEFAULT_TILE = 512
DEFAULT_AE = {"f32": 4, "f16": 8, "bf16": 8, "f64": 2}


def order_keeps(n: int) -> tuple[int, ...]:
    """``keep`` of the mean around the median in the order tests."""
    return (n, (n + 1) // 2, 2)


def order_sizes(code: str, tile: int = DEFAULT_TILE, ae: int | None = None) -> list[int]:
    ae = DEFAULT_AE[code] if ae is None else ae
    return [ae + 1, tile - 1, tile + 1]


def wide_values(gen: torch.Generator, numel: int, dtype: torch.dtype) -> torch.Tensor:
    """float64 [numel], every value representable in ``dtype`` (finite, normal, non-zero): a
    full-width random mantissa in [1, 2) times 2^e with a random sign, e uniform over
    ``EXPONENTS`` of the format."""
    code = {v: k for k, v in DTYPES.items()}[dtype]
    lo, hi = EXPONENTS[code]
    e = torch.randint(lo, hi + 1, (numel,), generator=gen).to(torch.float64)
    sign = torch.randint(0, 2, (numel,), generator=gen).to(torch.float64) * 2.0 - 1.0
    # 52 random bits below the leading one (1.0 + torch.rand would round its last bit away)
    mant = 1.0 + torch.randint(0, 2 ** 52, (numel,), generator=gen).to(torch.float64) * 2.0 ** -52
    if dtype != torch.float64:
        # round the mantissa in the target format first: a mantissa that rounds up to 2.0 at the top
        # exponent would leave fp16's range
        mant = mant.to(dtype).to(torch.float64).clamp(max=2.0 - 2.0 ** -7)
    v = (sign * mant * torch.exp2(e)).to(dtype).to(torch.float64)
    assert bool(torch.isfinite(v).all()) and bool((v != 0).all())
    return v


def order_rows(code: str, n: int, sizes: list[int]) -> list[list[torch.Tensor]]:
    """The order tests' clients for case (code, n): ``rows[c][t]`` is client c's float64 values of
    segment t, representable in the case's dtype. The same seed on the host and on the GPU."""
    gen = torch.Generator().manual_seed(7000 + 100 * list(DTYPES).index(code) + n)
    return [[wide_values(gen, s, DTYPES[code]) for s in sizes] for _ in range(n)]


def distinct_columns(rng: np.random.Generator, n: int, numel: int) -> np.ndarray:
    """float64 [n, numel]: every column is its own random permutation of the n distinct values
    ``j * j`` for j = 1 .. n — exact in every input format but fp16 above n = 45 (not used there),
    every sum exact in fp64, and the set is not symmetric about its middle."""
    base = np.arange(1, n + 1, dtype=np.float64) ** 2
    order = np.argsort(rng.random((n, numel)), axis=0)
    out = base[order]
    assert (np.sort(out, axis=0) == base[:, None]).all()
    return out


_PATTERN16 = {torch.float16: (0x7C00, 0x03FF), torch.bfloat16: (0x7F80, 0x007F)}


def all_patterns_16(dtype: torch.dtype, replacement: float = 1.5) -> tuple[torch.Tensor, int]:
    """All 65536 bit patterns of fp16 or bf16 in ascending unsigned order as a tensor of ``dtype``,
    with the NaN patterns replaced by ``replacement``; and the count of replaced patterns, which is
    asserted to be the format's NaN count (both signs, every non-zero mantissa under the all-ones
    exponent). Both infinities, both zeros and every subnormal stay."""
    exp_mask, man_mask = _PATTERN16[dtype]
    bits = torch.arange(65536, dtype=torch.int32)
    t = bits.to(torch.int16).view(dtype).clone()     # the low 16 bits of every index
    assert np.array_equal(t.view(torch.int16).to(torch.int32).numpy() & 0xFFFF, bits.numpy())
    nan = torch.isnan(t)
    by_bits = ((bits & exp_mask) == exp_mask) & ((bits & man_mask) != 0)
    assert bool((nan == by_bits).all())
    count = int(nan.sum())
    assert count == 2 * man_mask
    t[nan] = replacement
    return t, count


def random_patterns(gen: torch.Generator, numel: int, dtype: torch.dtype, replacement: float = 1.5
                    ) -> tuple[torch.Tensor, int]:
    """``numel`` uniformly random bit patterns of fp32 or fp64 with the NaN patterns replaced as in
    ``all_patterns_16``; and the count of replaced patterns."""
    if dtype == torch.float64:
        raw = torch.randint(-2 ** 63, 2 ** 63 - 1, (numel,), generator=gen, dtype=torch.int64)
    else:
        raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (numel,), generator=gen, dtype=torch.int64).to(torch.int32)
    t = raw.view(dtype).clone()
    nan = torch.isnan(t)
    t[nan] = replacement
    return t, int(nan.sum())


# ---- helpers of the GPU suites (plain torch: they work on any device) ----------------------------
SENTINEL = 12345.0


def bits(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        if x.dtype in (torch.float16, torch.bfloat16):
            return x.view(torch.int16).numpy().reshape(-1)
        x = x.numpy()
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view({8: np.int64, 4: np.int32, 2: np.int16}[x.dtype.itemsize])


def assert_same_bits(got, want, what="") -> None:
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if not np.array_equal(g, w):
        at = int(np.argwhere(g != w)[0][0])
        flat = [np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).reshape(-1) for v in (got, want)]
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} elements differ in bits; first at {at}: "
                             f"got {flat[0][at]!r}, want {flat[1][at]!r}")


def place(t: torch.Tensor, device, misalign: bool) -> torch.Tensor:
    """``t`` on the device; ``misalign``: a contiguous view one element into a larger buffer, so its
    storage starts off a 16-byte boundary and ends with the buffer."""
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
