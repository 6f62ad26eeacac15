"""The contract of ``fedavg_lowrank_aggregate_delta`` (include/fedavg_hip.h) restated
in numpy for one tensor: plain loops over the clients and the rank index, nothing of the package."""

from __future__ import annotations

import numpy as np


def lowrank_fold(lefts, rights, weights, divisor, base):
    """``lefts[c]`` is ``[m, r]`` and ``rights[c]`` ``[r, n]`` (float64 arrays holding the factors'
    exact values), ``base`` ``[m, n]`` float64. Returns ``(out, out_ld, A)``: the float64 result with
    every product and every addition separately rounded in ascending ``(c, j)``, the same in
    ``np.longdouble``, and ``A = sum |a| |R|`` with ``a_c = fl64(w_c * L_c)``."""
    m, n = base.shape
    S = np.zeros((m, n), dtype=np.float64)
    S_ld = np.zeros((m, n), dtype=np.longdouble)
    A = np.zeros((m, n), dtype=np.float64)
    for L, R, w in zip(lefts, rights, weights):
        a = np.float64(w) * L.astype(np.float64)
        for j in range(L.shape[1]):
            S = S + a[:, j:j + 1] * R[j:j + 1, :]
            S_ld = S_ld + a[:, j:j + 1].astype(np.longdouble) * R[j:j + 1, :].astype(np.longdouble)
            A = A + np.abs(a[:, j:j + 1]) * np.abs(R[j:j + 1, :])
    out = base + S / np.float64(divisor)
    out_ld = base.astype(np.longdouble) + S_ld / np.longdouble(divisor)
    return out, out_ld, A
