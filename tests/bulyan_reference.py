"""Restatement of Bulyan and of the mean around the median in numpy and plain Python (test-only;
NOT a reference algorithm — DESIGN.md §5k is the contract, and this file restates it independently
of the package: nothing is imported from it).

Per round, for the ``n`` counted clients in arrival order (``None`` = skipped), with ``f`` Byzantine
clients assumed (``None``: ``(n - 3) // 4``), ``theta = n - 2f`` and ``beta = n - 4f``:

* ``distances``: ``D[i][j] = sum_e (x_i[e] - x_j[e])^2`` in float64, an explicit loop over the pairs
  (numpy's own summation order: it pins the package only where every step is exact, which is the
  data the tests draw);
* ``select``: ``theta`` times, among the rows R still there (``r`` of them): the only row left with
  score 0.0, or else the row with the smallest (score, row), the score being the
  ``max(1, r - f - 2)`` smallest ``D[i][j]`` (j in R, j != i; ties in ascending j) added from the
  smallest; the picked row leaves R;
* ``mean_around_median``: per element the values in float64, sorted on an unsigned key of the bits
  (the IEEE total order); ``med`` the lower median; the window SHRINKS FROM THE ENDS: from
  ``lo = 0, hi = n - 1``, while more than ``beta`` values are left, ``lo += 1`` if
  ``(med - s_lo) > (s_hi - med)`` else ``hi -= 1`` (one rounded subtraction each, ``>`` false on
  NaN); then ``s_lo + ... + s_hi`` added ascending from ``s_lo`` and one division by ``beta``.
  The package counts the window's start instead; a host test compares the two forms.
"""

from __future__ import annotations

import numpy as np

_SIGN = np.uint64(1) << np.uint64(63)


class BulyanNaN(Exception):
    def __init__(self, stage: str) -> None:
        super().__init__(stage)
        self.stage = stage


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64).reshape(-1)


def sort_total_order(x: np.ndarray) -> np.ndarray:
    """float64 [n, P] sorted along axis 0 in the IEEE total order: the unsigned key of a value is
    its bits inverted if the sign bit is set, else its bits with the sign bit set."""
    bits = np.ascontiguousarray(x).view(np.uint64)
    key = np.where((bits & _SIGN) != 0, ~bits, bits | _SIGN)
    order = np.argsort(key, axis=0, kind="stable")
    return np.take_along_axis(x, order, axis=0)


def window_by_shrinking(s: np.ndarray, beta: int) -> np.ndarray:
    """``lo`` per column of the sorted float64 [n, P]: the kept window is ``[lo, lo + beta)``."""
    n, P = s.shape
    cols = np.arange(P)
    med = s[(n - 1) // 2]
    lo = np.zeros(P, dtype=np.int64)
    hi = np.full(P, n - 1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(n - beta):
            up = (med - s[lo, cols]) > (s[hi, cols] - med)
            lo = lo + up
            hi = hi - ~up
    assert ((hi - lo + 1) == beta).all()
    return lo


def mean_around_median(values: list, beta: int, out_dtype=np.float64) -> np.ndarray:
    """The coordinate step over one tensor's client values (numpy arrays of one shape)."""
    n = len(values)
    assert 1 <= beta <= n
    shape = np.asarray(values[0]).shape
    x = np.stack([_f64(v) for v in values])
    if np.isnan(x).any():
        raise BulyanNaN("input")
    s = sort_total_order(x)
    lo = window_by_shrinking(s, beta)
    cols = np.arange(x.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        total = s[lo, cols].copy()
        for j in range(1, beta):
            total = total + s[lo + j, cols]
        out = total / np.float64(beta)
    if np.isnan(out).any():
        raise BulyanNaN("result")
    with np.errstate(over="ignore"):
        return out.astype(out_dtype).reshape(shape)


def distances(clients: list[list]) -> np.ndarray:
    """``clients[i]``: client i's tensors (same order and shapes for all). float64 [n, n]."""
    n = len(clients)
    flat = [np.concatenate([_f64(t) for t in c]) if c else np.zeros(0) for c in clients]
    if any(np.isnan(x).any() for x in flat):
        raise BulyanNaN("input")
    D = np.zeros((n, n), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            for j in range(i + 1, n):
                d = flat[i] - flat[j]
                D[i, j] = D[j, i] = np.sum(d * d)
    if np.isnan(D).any():
        raise BulyanNaN("accumulator")
    return D


def select(D, f: int) -> tuple[list[int], list[float]]:
    """(rows in pick order, the winning score of each pick)."""
    M = [[float(v) for v in row] for row in np.asarray(D, dtype=np.float64).tolist()]
    n = len(M)
    if any(len(row) != n for row in M):
        raise ValueError("square")
    if f < 0 or n < 4 * f + 3:
        raise ValueError("n >= 4f + 3")
    remaining = list(range(n))
    picked, won = [], []
    for _ in range(n - 2 * f):
        r = len(remaining)
        if r == 1:
            winner, score = remaining[0], 0.0
        else:
            c = max(1, r - f - 2)
            winner, score = None, None
            for i in remaining:
                others = [(M[i][j], j) for j in remaining if j != i]
                others.sort(key=lambda p: (p[0], p[1]))
                s = 0.0
                for d, _ in others[:c]:
                    s += d
                if winner is None or s < score:   # rows ascend: an equal score keeps the earlier row
                    winner, score = i, s
        picked.append(winner)
        won.append(score)
        remaining.remove(winner)
    return picked, won


def bulyan_round(clients: list, f: int | None = None, out_dtype=np.float64):
    """A whole round. ``clients``: per client a dict name -> numpy array, or ``None`` (skipped).
    Returns ``(result dict, picked positions among the counted clients in pick order, scores,
    (f, theta, beta))``."""
    counted = [c for c in clients if c is not None]
    n = len(counted)
    names = list(counted[0])
    if f is None:
        f = (n - 3) // 4
    if f < 0 or n < 4 * f + 3:
        raise ValueError("n >= 4f + 3")
    theta, beta = n - 2 * f, n - 4 * f
    D = distances([[c[name] for name in names] for c in counted])
    picked, won = select(D, f)
    chosen = sorted(picked)
    result = {name: mean_around_median([counted[r][name] for r in chosen], beta, out_dtype) for name in names}
    return result, picked, won, (f, theta, beta)
