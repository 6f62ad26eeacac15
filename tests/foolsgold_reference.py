"""FoolsGold restated in plain numpy from its contract: the history step, the Gram
matrix in float64, the rule and the fold. Written from the contract, not from the package's code.
Clients, points and histories are lists of float64 numpy arrays, one per tensor of the layout."""

from __future__ import annotations

import math

import numpy as np


def gram(rows, point=None, history=None):
    """``(G, history_out, A)``: per element ``d = x - v`` (no point: ``x``), ``h = history + d``; ``G``
    the Gram matrix of the rows ``h`` (``d`` without history) and ``A`` the same sum over absolute
    values, the scale of the error bound."""
    n = len(rows)
    G, A = np.zeros((n, n)), np.zeros((n, n))
    new = [[] for _ in range(n)] if history is not None else None
    for s in range(len(rows[0])):
        R = []
        for i in range(n):
            r = rows[i][s].astype(np.float64) - point[s] if point is not None else rows[i][s].astype(np.float64)
            if history is not None:
                r = history[i][s] + r
                new[i].append(r)
            R.append(r.reshape(-1))
        R = np.stack(R)
        G = G + R @ R.T
        A = A + np.abs(R) @ np.abs(R).T
    return G, new, A


def coefficients(G, kappa=1.0):
    """``(alphas, max_cosines)`` of the n x n Gram matrix."""
    G = np.asarray(G, dtype=np.float64)
    n = len(G)
    if n == 1:
        return [1.0], [0.0]
    s = np.sqrt(np.diag(G))
    den = np.outer(s, s)
    cs = np.divide(G, den, out=np.zeros_like(G), where=den != 0)
    np.fill_diagonal(cs, 0.0)
    m = cs.max(axis=1)
    for i in range(n):
        for j in range(n):
            if i != j and m[i] < m[j]:
                cs[i, j] = cs[i, j] * m[i] / m[j]
    w = np.clip(1.0 - cs.max(axis=1), 0.0, 1.0)
    if w.max() == 0:
        return [0.0] * n, m.tolist()
    w = w / w.max()
    w[w == 1] = 0.99
    a = [kappa * (math.log(x / (1.0 - x)) + 0.5) if x > 0 else -math.inf for x in w.tolist()]
    return np.clip(a, 0.0, 1.0).tolist(), m.tolist()


def fold(rows, alphas, point, out_dtype=np.float64):
    """``v + (sum_i alpha_i (x_i - v)) / n`` per tensor: subtract, multiply, add in client order (the
    first product starts the sum), divide, add, then one rounding to ``out_dtype``."""
    outs = []
    for s, z in enumerate(point):
        acc = None
        for r, c in zip(rows, alphas):
            p = (r[s].astype(np.float64) - z) * c
            acc = p if acc is None else acc + p
        outs.append((z + acc / float(len(rows))).astype(out_dtype))
    return outs


def foolsgold_round(rows, point, history, kappa=1.0, G=None, out_dtype=np.float64):
    """One round: ``(result, history_out, alphas, G)``; ``G`` given: the rule and the fold on it."""
    G_own, new, _ = gram(rows, point, history)
    G = G_own if G is None else G
    alphas, _ = coefficients(G, kappa)
    return fold(rows, alphas, point, out_dtype), new, alphas, G
