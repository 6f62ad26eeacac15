"""Torch-CPU restatement of Krum / Multi-Krum (test-only; NOT a reference algorithm — DESIGN.md
§5h is the contract, this file restates it independently of the package: nothing is imported
from it).

Per round, for the ``n`` counted clients in arrival order:
* ``D[i][j] = sum_e (x_i[e] - x_j[e])^2`` over all elements of all tensors, values converted
  exactly to float64, an explicit loop over the pairs; symmetric, ``+0.0`` diagonal;
* ``score_i`` = the ``n - f - 2`` smallest ``D[i][j]`` (``j != i``) added from the smallest, ties
  in ascending ``j``; ``n >= 2f + 3``;
* the ``m`` smallest ``(score, row)`` are chosen (``1 <= m <= n - f``).
"""

from __future__ import annotations

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
