"""An independent numpy restatement of the sparse delta fold and of the client-side
top-k step. It shares no code with the package: element by element, five float64 operations.

    d_i[e] = the value client i stores for e, converted exactly to float64, or +0.0
    x_i    = b[e] + d_i[e]       (performed even for +0.0)
    p_i    = x_i * w_i
    acc    = p_0, then acc = acc + p_i   (table order, no leading 0 +)
    out[e] = acc / W

numpy rounds every one of them on its own (no FMA), which is the contract.
"""

from __future__ import annotations

import numpy as np
import torch

FLAG_ACC, FLAG_RESULT, FLAG_INPUT = 0x1, 0x2, 0x8


def to_f64(values) -> np.ndarray:
    """A torch tensor (any of the four value dtypes) or an array as float64, exactly."""
    if isinstance(values, torch.Tensor):
        return values.detach().cpu().to(torch.float64).numpy()
    return np.asarray(values, dtype=np.float64)


def indices_ok(indices, numel: int) -> bool:
    i = np.asarray(indices, dtype=np.int64)
    return bool(i.size == 0 or (i[0] >= 0 and i[-1] < numel and (np.diff(i) > 0).all()))


def fold(rows, weights, divisor, base, out_dtype=np.float64):
    """``rows[i][t] = (indices, values)`` of client i and tensor t; ``base[t]`` the float64 base.
    Returns the outputs per tensor and the NaN flag bits."""
    outs, flags = [], 0
    with np.errstate(all="ignore"):
        for t, b in enumerate(base):
            b = to_f64(b).reshape(-1)
            acc = None
            for row, w in zip(rows, weights):
                idx, val = row[t]
                idx = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64)
                assert indices_ok(idx, b.size)
                d = np.zeros(b.size, dtype=np.float64)       # +0.0 where the client has no entry
                d[idx] = to_f64(val)
                x = b + d
                if np.isnan(x).any():
                    flags |= FLAG_INPUT
                p = x * np.float64(w)
                acc = p if acc is None else acc + p
            if np.isnan(acc).any():
                flags |= FLAG_ACC
            out = acc / np.float64(divisor)
            if np.isnan(out).any():
                flags |= FLAG_RESULT
            outs.append(out.astype(out_dtype))
    return outs, flags


def total_weight(weights):
    """W as FedAVGAlgorithm sums scalar weights: the first, then += the next, in arrival order."""
    W = weights[0]
    for w in weights[1:]:
        W = W + w
    return W


def topk(total: np.ndarray, k: int):
    """The k entries of largest magnitude of the flat array, ties to the lower index, the indices
    ascending; returns (indices, values, residual)."""
    flat = np.asarray(total).reshape(-1)
    order = sorted(range(flat.size), key=lambda i: (-abs(float(flat[i])), i))[:k]
    idx = np.asarray(sorted(order), dtype=np.int64)
    residual = flat.copy()
    residual[idx] = 0
    return idx, flat[idx], residual
