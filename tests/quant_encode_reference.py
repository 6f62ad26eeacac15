"""Independent numpy restatement of the broadcast encoder (fedavg_quant_encode).

The records are the oracles' own: ``oracle.qsgd_oracle.quantize`` draws its uniforms from an
``rng`` object, and ``PhiloxStream`` below is such an object that returns the contract's uniform
stream (Philox4x32-10, written here from its definition, sharing no code with the package); the
NNADQ record is ``oracle.nnadq_oracle.quantize`` unchanged. Test infrastructure only.
"""

from __future__ import annotations

import numpy as np

from oracle import nnadq_oracle, qsgd_oracle

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox_scalar(ctr: tuple[int, int, int, int], key: tuple[int, int]) -> tuple[int, int, int, int]:
    """Philox4x32-10 on Python integers: ten rounds, the key bumped by the Weyl constants between
    rounds."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def philox_blocks(blocks: np.ndarray, t: int, draw: int, seed: int) -> np.ndarray:
    """out[b] = Philox(ctr = (block low, block high, t, draw), key = (seed low, seed high)) for every
    block of ``blocks`` (uint64), vectorised over the blocks: uint32 [len, 4]."""
    b = blocks.astype(np.uint64)
    x = [b & np.uint64(MASK), b >> np.uint64(32), np.full_like(b, t), np.full_like(b, draw)]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * x[0], np.uint64(M1) * x[2]
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ x[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
    return np.stack(x, axis=1).astype(np.uint32)


def uniforms(seed: int, draw: int, t: int, n: int, dtype) -> np.ndarray:
    """Element i's uniform. fp32: word i % 4 of block i // 4, (word >> 8) * 2^-24. fp64: block i // 2,
    lo = word 2 (i % 2), hi = word 2 (i % 2) + 1, ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53."""
    i = np.arange(n, dtype=np.uint64)
    if np.dtype(dtype) == np.float32:
        out = philox_blocks(np.arange((n + 3) // 4, dtype=np.uint64), t, draw, seed)
        word = out[(i // np.uint64(4)).astype(np.int64), (i % np.uint64(4)).astype(np.int64)]
        return ((word >> np.uint32(8)).astype(np.float64) * 2.0**-24).astype(np.float32)  # 24 bits: exact
    out = philox_blocks(np.arange((n + 1) // 2, dtype=np.uint64), t, draw, seed)
    blk, h = (i // np.uint64(2)).astype(np.int64), (i % np.uint64(2)).astype(np.int64)
    lo, hi = out[blk, 2 * h].astype(np.uint64), out[blk, 2 * h + 1].astype(np.uint64)
    m = (hi >> np.uint64(5)) * np.uint64(1 << 26) + (lo >> np.uint64(6))
    return m.astype(np.float64) * 2.0**-53  # 53 bits: exact


class PhiloxStream:
    """Stands in for the ``numpy.random.Generator`` of ``qsgd_oracle.quantize``: ``random(n)`` is
    the contract's stream of tensor ``t``."""

    def __init__(self, seed: int, draw: int, t: int, dtype) -> None:
        self.seed, self.draw, self.t, self.dtype = seed, draw, t, np.dtype(dtype)

    def random(self, n: int) -> np.ndarray:
        return uniforms(self.seed, self.draw, self.t, n, self.dtype)


def expected_record(x: np.ndarray, scheme: str, t: int = 0, level: int = 255, weight: float = 0.01, seed: int = 0,
                    draw: int = 0) -> np.ndarray:
    x = np.asarray(x).reshape(-1)
    assert x.dtype in (np.float32, np.float64)
    if scheme == "nnadq":
        return nnadq_oracle.quantize(x, weight)
    return qsgd_oracle.quantize(x, PhiloxStream(seed, draw, t, x.dtype), level)


def expected_records(parameter: dict[str, np.ndarray], scheme: str, level: int = 255, weight: float = 0.01,
                     seed: int = 0, draw: int = 0) -> dict[str, np.ndarray]:
    """One record per tensor; ``t`` is the tensor's position in the dict."""
    return {k: expected_record(v, scheme, t, level, weight, seed, draw) for t, (k, v) in enumerate(parameter.items())}


def has_mixed_zero_extremum(x: np.ndarray) -> bool:
    """The one case whose NNADQ header is compared numerically: the minimum is a zero and zeros of
    both signs occur (numpy's min then returns either zero; the contract says -0.0)."""
    x = np.asarray(x).reshape(-1)
    if x.size == 0 or x.min() != 0:
        return False
    z = x[x == 0]
    return bool(np.signbit(z).any() and (~np.signbit(z)).any())


def assert_same_record(got: np.ndarray, want: np.ndarray, x: np.ndarray, scheme: str, what: str = "") -> None:
    """Bytewise, except the sign of an NNADQ ``lo`` that is a zero where zeros of both signs are
    the minimum (then: lo is a zero, and every other byte is equal)."""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    assert got.shape == want.shape, what
    if scheme == "nnadq" and has_mixed_zero_extremum(x):
        assert got[0:8].view(np.float64)[0] == want[0:8].view(np.float64)[0] == 0.0, what
        assert np.array_equal(got[8:], want[8:]), what
        return
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:8]}: got {got[bad[:8]]}, want {want[bad[:8]]}")
