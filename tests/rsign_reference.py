"""A plain numpy restatement of the rotated 1-bit contract (include/fedavg_hip.h, fedavg_rsign_compress
and fedavg_rsign_aggregate_delta): the transform as a loop over levels and pairs, the sums as a tree,
the two scale rules, the fold. Element by element, with no vectorised shortcut that could hide an
order: the kernels and rotated.py are compared with it bit for bit."""

import numpy as np
import torch

from distributed_learning_simulation_lib_amd.dp import _narrow
from distributed_learning_simulation_lib_amd.quantized import philox4x32


def geometry(n):
    B = 64
    while B < n and B < 4096:
        B *= 2
    nb = -(-n // B)
    return B, nb, nb * B


def diagonal(seed, draw, tid, n_pad):
    """True where D is -1."""
    neg = np.zeros(n_pad, dtype=bool)
    for block in range(-(-n_pad // 128)):
        words = philox4x32(np.array([block & 0xFFFFFFFF, block >> 32, tid, draw], dtype=np.uint32),
                           (seed & 0xFFFFFFFF, seed >> 32))
        for j in range(128):
            e = 128 * block + j
            if e < n_pad:
                neg[e] = (int(words[j // 32]) >> (j % 32)) & 1
    return neg


def fwht(x, B):
    """H_B of every block of the fp64 vector x: levels h = 1, 2, ..., B / 2, pairs (i, i + h) with i & h == 0."""
    y = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for b0 in range(0, y.size, B):
            blk = y[b0:b0 + B]
            h = 1
            while h < B:
                lo = np.array([i for i in range(B) if i & h == 0])
                a, b = blk[lo].copy(), blk[lo + h].copy()
                blk[lo], blk[lo + h] = a + b, a - b
                h *= 2
    return y


def tree(x):
    x = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        while x.size > 1:
            x = x[0::2] + x[1::2]
    return x[0]


def narrow(x, dtype):
    """x rounded once into the torch dtype, as fp64 values."""
    return _narrow(np.asarray(x, dtype=np.float64), dtype).to(torch.float64).numpy()


def encode(total, dtype, seed, draw, tid, mode):
    """total: the fp64 values of delta + error already rounded into dtype. Returns (bits uint8 [n_pad / 8],
    scales as fp64 values of the scale dtype, residual as fp64 values of dtype)."""
    n = total.size
    B, nb, n_pad = geometry(n)
    D = diagonal(seed, draw, tid, n_pad)
    u = np.zeros(n_pad)
    u[:n] = np.where(D[:n], -total, total)
    y = fwht(u, B)
    sdt = torch.float64 if dtype == torch.float64 else torch.float32
    scales = np.zeros(nb)
    with np.errstate(all="ignore"):
        for k in range(nb):
            blk = y[k * B:(k + 1) * B]
            l1, l2 = tree(np.abs(blk)), tree(blk * blk)
            sigma = l2 / l1 if mode == "unbiased" else l1 / B
            scales[k] = 0.0 if l1 == 0 else sigma / B
    scales = narrow(scales, sdt)
    neg = np.signbit(y)
    z = fwht(np.where(neg, -np.repeat(scales, B), np.repeat(scales, B)), B)
    sent = narrow(np.where(D, -z, z)[:n], dtype)
    return np.packbits(neg, bitorder="little"), scales, narrow(total - sent, dtype)


def fold(bits, scales, weights, divisor, base, seed, draw, tid):
    """bits[i], scales[i]: client i's payload of one tensor; base: fp64 [n]. Returns the fp64 result."""
    n = base.size
    B, nb, n_pad = geometry(n)
    acc = None
    with np.errstate(all="ignore"):
        for b, s, w in zip(bits, scales, weights):
            neg = np.unpackbits(b, bitorder="little")[:n_pad].astype(bool)
            s = np.repeat(np.asarray(s, dtype=np.float64), B)
            p = np.where(neg, -s, s) * np.float64(w)
            acc = p if acc is None else acc + p
        z = fwht(acc / np.float64(divisor), B)
        return base + np.where(diagonal(seed, draw, tid, n_pad), -z, z)[:n]
