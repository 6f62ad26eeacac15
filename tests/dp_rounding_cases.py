"""Rows at which the clip-and-noise pass's final rounding into a 16-bit dtype is decided in the last
place (fedavg_dp_noise, DESIGN.md §5r: ``out = RNE(o)``, one rounding of the fp64 ``o``), shared by
tests/test_dp_host.py (the proofs and the CPU path) and tests/test_gpu_dp_contract.py (the kernel).

* Sharp pairs: a row ``[x, b]`` in row mode with no noise has ``o = x / s`` with ``s`` from the two
  elements. ``find_sharp_pairs`` searches 16-bit patterns for rows whose ``o`` rounds to a float32
  that lies exactly half way between two values of the 16-bit dtype while ``o`` itself does not, on
  the side where the tie then goes the other way: rounding through float32 gives other bits than one
  rounding. ``SHARP_PAIRS`` freezes what the searches in ``sharp_search_ranges`` found, so no test
  searches; tests/test_dp_host.py proves every frozen pair with exact rational arithmetic.
* Exact ties: a row ``[2 C, m * tiny]`` with ``tiny`` the dtype's smallest subnormal has ``s == 2``
  exactly and ``o = m * tiny / 2``: half way for an odd ``m``, up to an even neighbour for ``m = 3, 7,
  11``, down for ``m = 1, 5, 9``. With the suite's ``C = 0.5`` an fp16 row cannot have ``s == 2``:
  ``1 + 2**-48`` is an fp64 number. ``TIE_C = 128`` makes the first square ``2**16``, whose half ulp
  ``2**-37`` absorbs ``m * m * 2**-48`` for every ``m`` used here; ``tie_rows`` asserts it.

Test infrastructure only.
"""

from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch

from tests import dp_cases as cases
from tests import dp_reference as ref

DTYPES = ("f16", "bf16")
SHARP_C = cases.C
TIE_C = 128.0
TIE_M = (1, 2, 3, 4, 5, 6, 7, 9, 11, -1, -3, -5, -7, -10)
# (mantissa bits without the hidden one, smallest normal exponent)
FORMAT = {"f16": (10, -14), "bf16": (7, -126)}


def value_of(bits: np.ndarray, dtype: str) -> np.ndarray:
    """The float64 values of 16-bit patterns."""
    b = np.asarray(bits, dtype=np.uint16)
    if dtype == "f16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def tensor_of(bits: np.ndarray, dtype: str) -> torch.Tensor:
    b = np.asarray(bits, dtype=np.uint16)
    return torch.from_numpy(b.view(np.int16).copy()).view(cases.TORCH[dtype])


def direct_bits(o: np.ndarray, dtype: str) -> np.ndarray:
    """The restatement's one rounding."""
    return np.frombuffer(ref.narrow_bytes(np.asarray(o, dtype=np.float64), dtype), dtype=np.uint16)


def detour_bits(o: np.ndarray, dtype: str) -> np.ndarray:
    """What a kernel gives that rounds ``o`` to float32 first and that float32 to the dtype."""
    f = np.asarray(o, dtype=np.float64).astype(np.float32)
    if dtype == "f16":
        return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def exact_bits(o: Fraction, dtype: str) -> int:
    """RNE of the rational ``o`` into the dtype, in integer arithmetic (below the overflow threshold)."""
    mant, emin = FORMAT[dtype]
    sign, v = (0x8000, -o) if o < 0 else (0, o)
    if v == 0:
        return sign
    e = emin
    while v >= Fraction(2) ** (e + 1):
        e += 1
    q = v / Fraction(2) ** (e - mant)  # in units of the last place: < 2^(mant + 1), >= 2^mant if normal
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    # n = 2^(mant + 1) carries into the next exponent: the fields add up to the right pattern
    biased = e - emin + 1 if n >= 1 << mant else 0
    return sign | ((biased << mant) + (n - (1 << mant) if biased else n))


def row_scale(row: np.ndarray, dtype: str, c: float) -> np.float64:
    return ref.scale_of(ref.sum_of_squares([row], dtype), c)


def find_sharp_pairs(dtype: str, x_bits: np.ndarray, b_bits: np.ndarray, c: float = SHARP_C) -> list[tuple[int, int]]:
    """The pairs of patterns ``(x, b)`` whose row ``[x, b]`` (row mode, no noise, clipping norm ``c``)
    has an ``o = x / s`` that the float32 detour rounds to other bits than one rounding. Both
    squares and the quotient follow the contract's lines: lane 0 adds ``x * x`` then ``b * b``."""
    x_bits, b_bits = np.asarray(x_bits, dtype=np.uint16), np.asarray(b_bits, dtype=np.uint16)
    b = value_of(b_bits, dtype)[None, :]
    found: list[tuple[int, int]] = []
    for lo in range(0, x_bits.size, 256):
        x = value_of(x_bits[lo : lo + 256], dtype)[:, None]
        acc = (0.0 + x * x) + b * b
        t = np.sqrt(acc) / np.float64(c)
        o = x / np.where(t < 1.0, 1.0, t)
        hit = direct_bits(o.reshape(-1), dtype) != detour_bits(o.reshape(-1), dtype)
        for i, j in np.argwhere(hit.reshape(o.shape)):
            found.append((int(x_bits[lo + i]), int(b_bits[j])))
    return found


def sharp_search_ranges(dtype: str) -> tuple[np.ndarray, np.ndarray]:
    """The positive patterns the frozen pairs were searched in. fp16: magnitudes in [2^-6, 2^6), 151 M
    pairs, 6867 sharp ones (fp32 keeps 13 bits more than fp16). bf16: [2^-30, 2^30), 59 M pairs, 31
    sharp ones (16 bits more, and 8-bit significands give few different quotients): all of them are
    the one row [1, 0x97 / 256] scaled by the powers of two from 2^-1 up, since a scaling leaves the
    significand of ``o`` as it is once the row is clipped."""
    mant, emin = FORMAT[dtype]
    span = 6 if dtype == "f16" else 30
    bias = 1 - emin
    bits = np.arange((bias - span) << mant, (bias + span) << mant, dtype=np.uint16)
    return bits, bits


# From find_sharp_pairs(dtype, *sharp_search_ranges(dtype)). fp16: two per binade of x, drawn at
# random. bf16: the row in twenty binades, every third x and every third b negated (the squares and
# the magnitude of o stay; the sign goes through the rounding).
SHARP_PAIRS: dict[str, list[tuple[int, int]]] = {
    "f16": [
        (0x25FA, 0x44F1), (0x2654, 0x3DDB), (0x2849, 0x405F), (0x2AE5, 0x4004), (0x2DB6, 0x43EA), (0x2FDF, 0x530E),
        (0x30F7, 0x4B19), (0x32D9, 0x4BCC), (0x3632, 0x3E5C), (0x3705, 0x4538), (0x3A96, 0x2BBD), (0x3ACB, 0x31B1),
        (0x3C73, 0x3318), (0x3ECA, 0x4945), (0x41BF, 0x3E2F), (0x4208, 0x2C44), (0x45ED, 0x5324), (0x4761, 0x3138),
        (0x4942, 0x4BD5), (0x497C, 0x33C2), (0x4C70, 0x5140), (0x4DF2, 0x3E51), (0x50AA, 0x4D7F), (0x52F0, 0x49D0),
    ],
    "bf16": [
        (0x3F00, 0x3E97), (0xBF80, 0x3F17), (0x4000, 0xBF97), (0x4080, 0x4017), (0xC100, 0x4097), (0x4180, 0xC117),
        (0x4200, 0x4197), (0xC280, 0x4217), (0x4300, 0xC297), (0x4380, 0x4317), (0xC400, 0x4397), (0x4480, 0xC417),
        (0x4500, 0x4497), (0xC580, 0x4517), (0x4600, 0xC597), (0x4680, 0x4617), (0xC700, 0x4697), (0x4780, 0xC717),
        (0x4800, 0x4797), (0xC880, 0x4817),
    ],
}


def sharp_rows(dtype: str) -> tuple[torch.Tensor, bytes]:
    """(the rows ``[x, b]`` of every frozen pair as one tensor, the restatement's bytes for it: row
    length 2, ``SHARP_C``, no noise)."""
    x = tensor_of(np.array(SHARP_PAIRS[dtype], dtype=np.uint16).reshape(-1), dtype)
    (want,) = ref.expected([cases.widen(x)], dtype, 2, SHARP_C, 0.0, cases.SEED, cases.DRAW)
    return x, want


def tie_rows(dtype: str) -> tuple[torch.Tensor, bytes]:
    """(the rows ``[2 TIE_C, m * tiny]`` for ``m`` in ``TIE_M``, the restatement's bytes)."""
    tiny = 2.0 ** (FORMAT[dtype][1] - FORMAT[dtype][0])
    x = torch.tensor([[2 * TIE_C, m * tiny] for m in TIE_M], dtype=torch.float64).to(cases.TORCH[dtype]).reshape(-1)
    wide = cases.widen(x)
    assert wide.tolist() == [v for m in TIE_M for v in (2 * TIE_C, m * tiny)]  # the dtype holds them
    for row in wide.reshape(-1, 2):
        assert row_scale(row, dtype, TIE_C) == 2.0
    (want,) = ref.expected([wide], dtype, 2, TIE_C, 0.0, cases.SEED, cases.DRAW)
    return x, want
