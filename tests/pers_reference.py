"""The PersonalizedFedAVG reduce of csrc/personalized_kernels.hip restated in plain numpy float64,
from the formulas at the top of that file. Test support only (no test in this file); nothing is
imported from the package, and nothing here runs on a GPU.

Per receiver j (a row of ``weights[M][N]`` with the id ``receiver_ids[j]``) and per segment t::

    acc_j[t] = x_k.astype(f64) * w_jk            the first client k that j folds, in arrival order
    acc_j[t] = acc_j[t] + x_k.astype(f64) * w_jk every later one: product and sum rounded separately
    W_j[t]   = w_jk, then W_j[t] + w_jk          in the same order
    out_j[t] = acc_j[t] / W_j[t]
    central[t] = out_0[t] * (1 / M), then central[t] + out_j[t] * (1 / M) in row order

A receiver folds every client but the one with its own id and the ones that did not send segment t
(``None``). A weight of 0 is folded like any other weight. Nothing here raises on a NaN: the three
NaN assertions of the reference become the verdicts ``Result.flags`` (the bits ``fedavg_pers_check``
reports), so that a test can ask for exactly those bits.

``fma`` / ``fused_chain`` are the exact fused fold — ``round(acc + x * w)`` with one rounding, through
``fractions.Fraction`` — for the host-side proofs of tests/test_pers_values_host.py only.
"""

from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

import numpy as np

# the bits of fedavg_pers_check (include/fedavg_hip.h: FEDAVG_FLAG_*)
FLAG_ACC_NAN, FLAG_RESULT_NAN, FLAG_CENTRAL_NAN = 0x1, 0x2, 0x4


@dataclass
class Result:
    outs: list[list[np.ndarray]]          # [M][T] float64
    central: list[np.ndarray]             # [T] float64
    totals: np.ndarray                    # [M][T] float64
    flags: int                            # with the centralized verdict
    flags_no_central: int                 # of a call that asks for no centralized model
    stacked: list[np.ndarray]             # [T] float64 [M, size]: ``outs`` with the receivers stacked


def folded(clients, client_ids, receiver_id, t) -> list[int]:
    """The clients that a receiver folds in segment t, in arrival order."""
    return [k for k, row in enumerate(clients) if client_ids[k] != receiver_id and row[t] is not None]


def separate_chain(xs, ws) -> np.ndarray:
    """The reference's chain: every product and every sum is one rounded fp64 operation (numpy
    never fuses them)."""
    acc = None
    with np.errstate(all="ignore"):
        for x, w in zip(xs, ws):
            p = np.asarray(x, dtype=np.float64) * np.float64(w)
            acc = p if acc is None else acc + p
    return acc


def reduce(clients, client_ids, weights, receiver_ids) -> Result:
    """``clients[N][T]``: float64 arrays (the exact widening of the input format) or ``None``;
    ``weights[M][N]``; ids as in ``PersonalizedContext.aggregate``."""
    w = np.asarray(weights, dtype=np.float64)
    M, N, T = len(receiver_ids), len(clients), len(clients[0])
    assert w.shape == (M, N) and len(client_ids) == N and len(set(client_ids)) == N and len(set(receiver_ids)) == M
    stacked, totals, flags = [], np.zeros((M, T)), 0
    with np.errstate(all="ignore"):
        for t in range(T):
            # receivers that fold the same clients share their chain's steps: one elementwise
            # numpy operation per step serves all of them (each element is still one rounded fp64
            # product or sum)
            same_list: dict[tuple, list[int]] = {}
            for j, rid in enumerate(receiver_ids):
                ks = tuple(folded(clients, client_ids, rid, t))
                assert ks, f"receiver {j} has no data for segment {t}"
                same_list.setdefault(ks, []).append(j)
            size = next(row[t].size for row in clients if row[t] is not None)
            acc = np.empty((M, size))
            for ks, rows in same_list.items():
                a = tot = None
                for k in ks:
                    wk = w[rows, k]
                    p = np.asarray(clients[k][t], dtype=np.float64)[None, :] * wk[:, None]
                    a = p if a is None else a + p
                    tot = wk.copy() if tot is None else tot + wk
                acc[rows], totals[rows, t] = a, tot
            out = acc / totals[:, t][:, None]
            flags |= FLAG_ACC_NAN if np.isnan(acc).any() else 0
            flags |= FLAG_RESULT_NAN if np.isnan(out).any() else 0
            stacked.append(out)
        cw = np.float64(1.0) / np.float64(M)
        central = []
        for out in stacked:
            d = out * cw
            c = d[0].copy()
            for j in range(1, M):
                c = c + d[j]
            central.append(c)
    with_central = flags | (FLAG_CENTRAL_NAN if any(np.isnan(c).any() for c in central) else 0)
    outs = [[stacked[t][j] for t in range(T)] for j in range(M)]
    return Result(outs, central, totals, with_central, flags, stacked)


# ---- the exact fused fold (host proofs only) -----------------------------------------------------
def fma(x: float, w: float, acc: float) -> float:
    """round(acc + x * w), rounded once to nearest even: ``float(Fraction)`` is correctly rounded.
    Finite operands only; a zero result is +0.0 (the proofs plant no zero)."""
    return float(Fraction(x) * Fraction(w) + Fraction(acc))


def fused_chain(xs, ws) -> np.ndarray:
    """The chain of ``separate_chain`` with every fold fused (the first fold rounds its product)."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    out = np.empty(xs[0].shape, dtype=np.float64)
    for e in range(out.size):
        acc = 0.0
        for x, w in zip(xs, ws):
            acc = fma(float(x[e]), float(w), acc)
        out[e] = acc
    return out


# ---- comparisons ---------------------------------------------------------------------------------
def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1).view(np.int64)


def differing(got, want) -> np.ndarray:
    """Indices at which two float64 arrays differ: another NaN mask, or other bits where neither
    is a NaN (a NaN compares as a NaN, whatever its payload)."""
    g, w = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    gn, wn = np.isnan(g), np.isnan(w)
    return np.flatnonzero((gn != wn) | (~gn & ~wn & (bits64(g) != bits64(w))))
