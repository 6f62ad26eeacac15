"""Host arithmetic of the side rules: what the robust, Krum, Bulyan, geometric-median, clipping,
FLTrust and server-optimiser algorithms compute on the CPU between two kernel calls, and on their CPU
paths in place of them.

Pure host code in plain Python floats (``server_opt_update`` alone works on torch CPU tensors): no
library, no device. The GPU wrappers that these functions serve are ``FedAvgContext``'s
(``fedavg.py``, which re-exports every name here); DESIGN.md §5h-§5m state the arithmetic.
"""

from __future__ import annotations

import math
from collections.abc import Sequence
from typing import Any

import numpy as np
import torch

ROBUST_MODES = ("trimmed_mean", "median")


def check_robust_rule(mode: str, trim: float) -> None:
    """ValueError for an unknown robust rule or a trim fraction outside [0, 0.5)."""
    if mode not in ROBUST_MODES:
        raise ValueError(f"robust aggregation mode must be one of {ROBUST_MODES}, not {mode!r}")
    if mode == "trimmed_mean" and not 0 <= trim < 0.5:  # NaN fails it too
        raise ValueError(f"trim must satisfy 0 <= trim < 0.5 (the kept range must not be empty), not {trim}")


def robust_trim(mode: str, trim: float, n: int) -> int:
    """Values dropped at each end of a tensor's n sorted client values: floor(trim * n) for the
    trimmed mean; (n - 1) // 2 for the median, which leaves the one or two middle values."""
    return (n - 1) // 2 if mode == "median" else math.floor(trim * n)


def krum_select(D: Any, f: int, m: int) -> tuple[list[float], list[int]]:
    """Krum scores and the one-shot Multi-Krum choice from the n x n matrix of squared distances
    (host arithmetic in fp64, shared by the GPU and the CPU path).

    ``f`` is the assumed number of Byzantine clients (``n >= 2f + 3``). ``score_i`` is the sum of
    the ``n - f - 2`` smallest ``D[i][j]``, ``j != i``: sorted ascending, ties in ascending ``j``,
    added sequentially from the smallest. The ``m`` rows (``1 <= m <= n - f``; 1 is Krum) with the
    smallest ``(score, row)`` are chosen, so ties go to the earlier arrival. Returns
    ``(scores, chosen_rows)``, the rows in ascending order (arrival order)."""
    rows = [[float(x) for x in r] for r in (D.tolist() if hasattr(D, "tolist") else D)]
    n = len(rows)
    if any(len(r) != n for r in rows):
        raise ValueError("the distance matrix must be square")
    f, m = int(f), int(m)
    if f < 0 or n < 2 * f + 3:
        raise ValueError(f"Krum needs n >= 2f + 3 clients: n = {n}, f = {f}")
    if not 1 <= m <= n - f:
        raise ValueError(f"Multi-Krum selects 1 <= m <= n - f = {n - f} clients, not {m}")
    keep = n - f - 2
    scores = []
    for i, r in enumerate(rows):
        near = sorted((d, j) for j, d in enumerate(r) if j != i)[:keep]
        s = 0.0
        for d, _ in near:
            s = s + d
        scores.append(s)
    order = sorted(range(n), key=lambda i: (scores[i], i))
    return scores, sorted(order[:m])


def bulyan_select(D: Any, f: int) -> tuple[list[int], list[float]]:
    """Bulyan's selection from the n x n matrix of squared distances (host arithmetic
    in plain Python floats, shared by the GPU and the CPU path): Krum applied iteratively.

    ``f`` is the assumed number of Byzantine clients (``n >= 4f + 3``); ``theta = n - 2f`` rows are
    picked. Start from R, all rows, and repeat ``theta`` times with ``r = |R|``: if ``r == 1`` the
    row that is left is taken with score 0.0; otherwise, with ``c = max(1, r - f - 2)``,
    ``score_i`` (i in R) is the sum of the ``c`` smallest ``D[i][j]``, j in R without i — sorted
    ascending, ties in ascending ``j``, added sequentially from the smallest starting at 0.0 — and
    the row with the smallest ``(score, row)`` is picked and leaves R, so ties go to the earlier
    arrival. The ``max(1, .)`` is this project's choice: the paper's ``r - f - 2`` neighbours run
    out in the last picks (``r`` goes down to ``2f + 1``, where ``r - f - 2 = f - 1`` is 0 for
    ``f = 1`` and all of R is picked for ``f = 0``), and a row is then judged by its nearest
    neighbour. Returns ``(picked_rows, pick_scores)``: the rows in pick order and the winning
    score of each pick."""
    rows = [[float(x) for x in r] for r in (D.tolist() if hasattr(D, "tolist") else D)]
    n = len(rows)
    if any(len(r) != n for r in rows):
        raise ValueError("the distance matrix must be square")
    f = int(f)
    if f < 0 or n < 4 * f + 3:
        raise ValueError(f"Bulyan needs n >= 4f + 3 clients: n = {n}, f = {f}")
    # every row's neighbours once, nearest first; a pick only removes entries from these lists
    near = [sorted((d, j) for j, d in enumerate(r) if j != i) for i, r in enumerate(rows)]
    alive = [True] * n
    picked: list[int] = []
    scores: list[float] = []
    for r in range(n, 2 * f, -1):
        best: tuple[float, int] | None = None
        if r == 1:
            best = (0.0, alive.index(True))
        else:
            c = max(1, r - f - 2)
            for i in range(n):
                if not alive[i]:
                    continue
                s, left = 0.0, c
                for d, j in near[i]:
                    if alive[j]:
                        s = s + d
                        left -= 1
                        if left == 0:
                            break
                if best is None or (s, i) < best:
                    best = (s, i)
        assert best is not None
        scores.append(best[0])
        picked.append(best[1])
        alive[best[1]] = False
    return picked, scores


def geometric_median_step(dist_sq: Sequence[float], alpha: Sequence[float],
                          smoothing: float) -> tuple[list[float], float]:
    """One smoothed Weiszfeld step of the geometric median (host arithmetic in plain
    Python floats, shared by the GPU and the CPU path): from the clients' squared distances ``D_i``
    to the current point and their weights ``alpha_i``, with ``d_i = math.sqrt(D_i)``, the next
    fold's weights ``beta_i = alpha_i / max(smoothing, d_i)`` and the objective
    ``sum_i alpha_i * d_i`` at the current point, added sequentially in arrival order from 0.0.
    Returns ``(beta, objective)``."""
    ds = [float(x) for x in (dist_sq.tolist() if hasattr(dist_sq, "tolist") else dist_sq)]
    al = [float(a) for a in alpha]
    nu = float(smoothing)
    if len(ds) != len(al):
        raise ValueError("one squared distance per weight is required")
    if not nu > 0:
        raise ValueError(f"smoothing must be > 0, not {smoothing}")
    beta, objective = [], 0.0
    for D, a in zip(ds, al):
        d = math.sqrt(D)
        beta.append(a / max(nu, d))
        objective = objective + a * d
    return beta, objective


def clipping_coefficients(dist_sq: Sequence[float], alpha: Sequence[float],
                          radius: float) -> tuple[list[float], int]:
    """The coefficients of one centred-clipping step (host arithmetic in plain Python
    floats, shared by the GPU and the CPU path): from the clients' squared distances ``D_i`` to the
    current centre and their weights ``alpha_i``, with ``d_i = math.sqrt(D_i)``,
    ``c_i = 1.0 if d_i <= radius else radius / d_i`` (``D_i = +inf`` gives 0.0) and
    ``coef_i = alpha_i * c_i``. Returns ``(coef, clipped)``: the coefficients and the number of
    clients whose distance exceeded the radius."""
    ds = [float(x) for x in (dist_sq.tolist() if hasattr(dist_sq, "tolist") else dist_sq)]
    al = [float(a) for a in alpha]
    tau = float(radius)
    if len(ds) != len(al):
        raise ValueError("one squared distance per weight is required")
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"radius must be a finite number > 0, not {radius}")
    coef, clipped = [], 0
    for D, a in zip(ds, al):
        d = math.sqrt(D)
        if d <= tau:
            c = 1.0
        else:
            c = tau / d
            clipped += 1
        coef.append(a * c)
    return coef, clipped


def trust_coefficients(dots: Sequence[float], sqnorms: Sequence[float],
                       root_sqnorm: float) -> tuple[list[float], list[float]]:
    """FLTrust's trust scores and coefficients (host arithmetic in plain Python
    floats, shared by the GPU and the CPU path): from the clients' dots ``T_i = <x_i - v, g>`` with
    the root direction, their squared norms ``S_i = |x_i - v|^2`` and the root's own squared norm,
    in this operation order: ``n0 = math.sqrt(root_sqnorm)``, ``ni = math.sqrt(S_i)``,
    ``den = ni * n0``; a client whose ``S_i`` is not finite or whose ``den`` is 0 is distrusted
    (score and coefficient 0.0); otherwise ``cos = T_i / den``, ``score = cos if cos > 0 else 0.0``
    (the ReLU-clipped cosine; a NaN cosine scores 0.0) and ``coefficient = score * (n0 / ni)`` (the
    score times the rescaling of the client's update to the root's norm). Returns
    ``(scores, coefficients)``."""
    ts = [float(x) for x in (dots.tolist() if hasattr(dots, "tolist") else dots)]
    ss = [float(x) for x in (sqnorms.tolist() if hasattr(sqnorms, "tolist") else sqnorms)]
    root = float(root_sqnorm)
    if len(ts) != len(ss):
        raise ValueError("one dot per squared norm is required")
    n0 = math.sqrt(root)
    scores, coef = [], []
    for T, S in zip(ts, ss):
        if not math.isfinite(S):
            scores.append(0.0)
            coef.append(0.0)
            continue
        ni = math.sqrt(S)
        den = ni * n0
        if den == 0:
            scores.append(0.0)
            coef.append(0.0)
            continue
        cos = T / den
        score = cos if cos > 0 else 0.0
        scores.append(score)
        coef.append(score * (n0 / ni))
    return scores, coef


SERVER_OPT_MODES = ("avgm", "adagrad", "yogi", "adam")  # FEDAVG_OPT_AVGM / ADAGRAD / YOGI / ADAM in this order


def check_server_opt(mode: str, lr: float, beta1: float, beta2: float,
                     tau: float) -> tuple[int, float, float, float, float, float, float]:
    """The hyper-parameters of a server optimiser step, validated as the C call
    validates them: ``mode`` one of ``SERVER_OPT_MODES``; ``lr`` finite and > 0; ``beta1`` and
    ``beta2`` in [0, 1); ``tau`` finite and > 0 in the adaptive modes (``"avgm"`` ignores it).
    Returns ``(code, lr, beta1, 1 - beta1, beta2, 1 - beta2, tau)`` as Python floats: ``1 - beta`` is
    computed here once, so the kernel, the CPU path and a restatement use the same doubles."""
    if mode not in SERVER_OPT_MODES:
        raise ValueError(f"mode must be one of {SERVER_OPT_MODES}, not {mode!r}")
    lr, beta1, beta2, tau = float(lr), float(beta1), float(beta2), float(tau)
    if not (lr > 0 and math.isfinite(lr)):
        raise ValueError(f"the learning rate must be a finite number > 0, not {lr}")
    for name, b in (("beta1", beta1), ("beta2", beta2)):
        if not 0 <= b < 1:
            raise ValueError(f"{name} must lie in [0, 1), not {b}")
    if mode != "avgm" and not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"tau must be a finite number > 0, not {tau}")
    return SERVER_OPT_MODES.index(mode), lr, beta1, 1.0 - beta1, beta2, 1.0 - beta2, tau


def _sqrt_rn(t: torch.Tensor) -> torch.Tensor:
    """The correctly rounded float64 square root of a CPU tensor. ``torch.sqrt``'s CPU kernel goes
    through a vector maths library whose results are off by one ulp for some inputs (measured: 670
    of 100 000 uniform values against ``numpy.sqrt``), so the root — and it alone — is taken by numpy,
    which uses the processor's IEEE instruction."""
    with np.errstate(invalid="ignore"):
        r = np.sqrt(t.detach().contiguous().numpy().reshape(-1))
    return torch.from_numpy(r).reshape(t.shape)


def server_opt_update(mode: str, delta: torch.Tensor, m: torch.Tensor, v: torch.Tensor | None, lr: float,
                      beta1: float, one_minus_beta1: float, beta2: float, one_minus_beta2: float,
                      tau: float) -> tuple[torch.Tensor, torch.Tensor | None, torch.Tensor]:
    """The optimiser lines of ``fedavg_server_opt_step`` in torch, one float64 operation per line
    (DESIGN.md §5m): from the pseudo-gradient ``delta`` and the moments ``m``, ``v`` returns
    ``(m', v', u)``; the new model is ``z + u``. ``v`` and ``v'`` are ``None`` for ``"avgm"``. CPU
    tensors only (the square root is ``_sqrt_rn``)."""
    a = beta1 * m
    if mode == "avgm":
        m_new = a + delta
        return m_new, None, lr * m_new
    b = one_minus_beta1 * delta
    m_new = a + b
    q = delta * delta
    if mode == "adagrad":
        v_new = v + q
    elif mode == "adam":
        e = beta2 * v
        f = one_minus_beta2 * q
        v_new = e + f
    else:  # yogi
        g = v - q
        s = (g > 0).to(torch.float64) - (g < 0).to(torch.float64)  # +1.0, -1.0, else (NaN included) +0.0
        f = one_minus_beta2 * q
        h = f * s
        v_new = v - h
    r = _sqrt_rn(v_new)
    den = r + tau
    num = lr * m_new
    return m_new, v_new, num / den
