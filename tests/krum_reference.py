"""Torch-CPU restatement of Krum / Multi-Krum (test-only; NOT a reference algorithm — DESIGN.md
§5h is the contract, this file restates it independently of the package: nothing is imported
from it).

Per round, for the ``n`` counted clients in arrival order:
* ``D[i][j] = sum_e (x_i[e] - x_j[e])^2`` over all elements of all tensors, values converted
  exactly to float64, an explicit loop over the pairs; symmetric, ``+0.0`` diagonal;
* ``score_i`` = the ``n - f - 2`` smallest ``D[i][j]`` (``j != i``) added from the smallest, ties
  in ascending ``j``; ``n >= 2f + 3``;
* the ``m`` smallest ``(score, row)`` are chosen (``1 <= m <= n - f``).

``distances`` fixes no summation order (torch's pairwise ``sum``), so it pins the kernel only where
every step is exact or through the contract's bound. ``distances_in_order`` restates the order of
the determinism contract itself: per segment, per chunk of ``chunk`` elements (the caller passes
the build's ``krum_chunk``), ascending element order into one float64 accumulator per pair; then
the chunk partials added sequentially from ``+0.0`` in layout order. It multiplies and adds
separately, so it equals a kernel that uses an FMA only on data whose squares ``d * d`` are exact
in float64 (``order_sensitive_values`` draws such data); ``distances_in_order_fused`` rounds
``d * d + acc`` once, as an FMA does, for any finite data, but is a Python loop for small inputs.
"""

from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch


class KrumNaN(Exception):
    def __init__(self, stage: str) -> None:
        super().__init__(stage)
        self.stage = stage


def distances(clients: list[list[torch.Tensor]]) -> torch.Tensor:
    """``clients[i]``: client i's tensors (same order and shapes for all). float64 [n, n]."""
    n = len(clients)
    flat = [torch.cat([t.detach().cpu().to(torch.float64).reshape(-1) for t in c]) for c in clients]
    if any(bool(torch.isnan(x).any()) for x in flat):
        raise KrumNaN("input")
    D = torch.zeros((n, n), dtype=torch.float64)
    for i in range(n):
        for j in range(i + 1, n):
            diff = flat[i] - flat[j]
            D[i, j] = torch.sum(diff * diff)
            D[j, i] = D[i, j]
    if bool(torch.isnan(D).any()):
        raise KrumNaN("accumulator")
    return D


def scores(D: torch.Tensor, f: int) -> list[float]:
    n = D.shape[0]
    if f < 0 or n < 2 * f + 3:
        raise ValueError("n >= 2f + 3")
    out = []
    for i in range(n):
        others = [(D[i, j].item(), j) for j in range(n) if j != i]
        others.sort(key=lambda p: (p[0], p[1]))
        s = 0.0
        for d, _ in others[: n - f - 2]:
            s += d
        out.append(s)
    return out


def select(D: torch.Tensor, f: int, m: int) -> tuple[list[float], list[int]]:
    """(scores, chosen rows in arrival order)."""
    sc = scores(D, f)
    n = len(sc)
    if not 1 <= m <= n - f:
        raise ValueError("1 <= m <= n - f")
    ranked = sorted(range(n), key=lambda i: (sc[i], i))
    return sc, sorted(ranked[:m])


# ---- the summation order of the determinism contract ---------------------------------------------
def order_sensitive_values(gen: torch.Generator, numel: int) -> torch.Tensor:
    """float64 [numel]: sign * (k / 128, k in 128..255) * 2^e, e in [-9, 9).

    Every value is representable in bf16 (8 significant bits), fp16, fp32 and fp64. Every value,
    and so every difference of two, is a multiple of 2^-16 below 2^10 in magnitude: at most 26
    significant bits, so every square is exact in float64. The running sums are not (terms from
    2^-32 to 2^20 meet in one accumulator), so the result depends on the order of the additions."""
    k = torch.randint(128, 256, (numel,), generator=gen).to(torch.float64)
    e = torch.randint(-9, 9, (numel,), generator=gen).to(torch.float64)
    sign = torch.randint(0, 2, (numel,), generator=gen).to(torch.float64) * 2.0 - 1.0
    return sign * (k / 128.0) * torch.exp2(e)


def _segments(clients: list[list[torch.Tensor]]) -> list[np.ndarray]:
    """Per segment a float64 array [elements, clients]."""
    segs = []
    for t in range(len(clients[0])):
        rows = [c[t].detach().cpu().to(torch.float64).reshape(-1).numpy() for c in clients]
        segs.append(np.ascontiguousarray(np.stack(rows, axis=1)))
    return segs


def chunk_partials(clients: list[list[torch.Tensor]], chunk: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(partials [chunks in layout order, pairs], iu, ju): per chunk and per pair ``i < j`` (the
    pairs of ``np.triu_indices(n, 1)``) one accumulator from ``+0.0``, the chunk's elements in
    ascending order: ``d = x_i[e] - x_j[e]``, ``acc = acc + d * d``."""
    n = len(clients)
    iu, ju = np.triu_indices(n, 1)
    partials = []
    for x in _segments(clients):
        for start in range(0, x.shape[0], chunk):
            acc = np.zeros(len(iu), dtype=np.float64)
            for row in x[start:start + chunk]:
                d = row[iu] - row[ju]
                acc = acc + d * d
            partials.append(acc)
    return np.stack(partials) if partials else np.zeros((0, len(iu))), iu, ju


def _mirror(values: np.ndarray, iu: np.ndarray, ju: np.ndarray, n: int) -> torch.Tensor:
    D = np.zeros((n, n), dtype=np.float64)
    D[iu, ju] = values
    D[ju, iu] = values
    return torch.from_numpy(D)


def distances_in_order(clients: list[list[torch.Tensor]], chunk: int) -> torch.Tensor:
    """float64 [n, n] in the contract's summation order (see the module docstring)."""
    partials, iu, ju = chunk_partials(clients, chunk)
    total = np.zeros(len(iu), dtype=np.float64)
    for p in partials:
        total = total + p
    return _mirror(total, iu, ju, len(clients))


def distances_in_order_fused(clients: list[list[torch.Tensor]], chunk: int) -> torch.Tensor:
    """The same order with ``d * d + acc`` rounded once (an FMA), in exact rational arithmetic: a
    Python loop over pairs and elements, for small finite inputs only."""
    n = len(clients)
    segs = [x.T.tolist() for x in _segments(clients)]   # [client][element]
    iu, ju = np.triu_indices(n, 1)
    values = []
    for i, j in zip(iu.tolist(), ju.tolist()):
        total = 0.0
        for x in segs:
            xi, xj = x[i], x[j]
            for start in range(0, len(xi), chunk):
                acc = 0.0
                for a, b in zip(xi[start:start + chunk], xj[start:start + chunk]):
                    d = Fraction(a - b)
                    acc = float(d * d + Fraction(acc))   # int / int division: correctly rounded
                total = total + acc
        values.append(total)
    return _mirror(np.asarray(values, dtype=np.float64), iu, ju, n)
