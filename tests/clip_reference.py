"""An independent restatement of the centred-clipping contract in numpy, written
from the document and not from the package: the fold about a point as a loop over clients of
``np.float64`` operations, the coefficient rule and the round loop. The distances are those of
``tests/geomed_reference.py`` (§5i's pinned order). Test support only (no test in this file).

Per element: d_i = x_i - z, p_i = c_i * d_i, acc = p_0 then acc + p_i in table order,
r = acc / divisor, out = z + r; each a separately rounded float64 operation (numpy's elementwise
operators never fuse), float32 output = that rounded to nearest even (``astype``).
"""

from __future__ import annotations

import math

import numpy as np

from tests import geomed_reference as geo

INF = float("inf")
FLAG_ACC, FLAG_RESULT, FLAG_INPUT = 0x1, 0x2, 0x8


def fold_about_point(clients, coefficients, divisor, point, out_dtype=np.float64):
    """``clients[i]`` is client i's tensors in layout order, ``point`` one float64 tensor per
    segment. Returns (outs, flags): one flat array per segment and the NaN flags the call latches
    (input: a NaN in a client or the point; acc: a NaN in the sum; result: a NaN in z + r)."""
    flags = 0
    outs = []
    div = np.float64(divisor)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t, z in enumerate(point):
            z = geo.as_f64(z)
            if np.isnan(z).any():
                flags |= FLAG_INPUT
            acc = None
            for row, c in zip(clients, coefficients):
                x = geo.as_f64(row[t])
                if np.isnan(x).any():
                    flags |= FLAG_INPUT
                d = x - z
                p = np.float64(c) * d
                acc = p if acc is None else acc + p
            if np.isnan(acc).any():
                flags |= FLAG_ACC
            r = acc / div
            out = z + r
            if np.isnan(out).any():
                flags |= FLAG_RESULT
            outs.append(out.astype(out_dtype))
    return outs, flags


def coefficients(dist_sq, alpha, radius):
    """coef_i = alpha_i * min(1, radius / sqrt(D_i)) written as the two-branch rule; and the count
    of clients beyond the radius."""
    coef, clipped = [], 0
    for D, a in zip(dist_sq, alpha):
        d = math.sqrt(float(D))
        if d > radius:
            clipped += 1
            coef.append(float(a) * (radius / d))
        else:
            coef.append(float(a) * 1.0)
    return coef, clipped


def centred_clipping(clients, alpha, constants: dict, dtype, radius, iterations=1, start=None,
                     out_dtype=np.float64) -> dict:
    """The whole rule on rows of tensors. ``start`` is the previous model (one float64 tensor per
    segment) or None for the FedAvg of the kept clients. Returns the result (flat arrays per
    tensor), the kept and dropped rows, and per iteration the distances, coefficients and count."""
    W = 0.0
    for a in alpha:
        W = W + float(a)
    if not W > 0:
        raise ValueError("weights add up to 0")
    norms = geo.distances_in_order(clients, None, constants, dtype)
    kept = [i for i, v in enumerate(norms) if v != INF]
    dropped = [i for i, v in enumerate(norms) if v == INF]
    if not kept:
        raise ValueError("no finite client")
    rows = [clients[i] for i in kept]
    al = [float(alpha[i]) for i in kept]
    v = [geo.as_f64(z) for z in start] if start is not None else geo.fold(rows, al)
    dists, coefs, counts = [], [], []
    for it in range(1, iterations + 1):
        D = geo.distances_in_order(rows, v, constants, dtype)
        coef, count = coefficients(D, al, radius)
        dists.append(D.tolist())
        coefs.append(coef)
        counts.append(count)
        v, flags = fold_about_point(rows, coef, W, v, out_dtype if it == iterations else np.float64)
        if flags:
            raise geo.GeomedNaN("input" if flags & FLAG_INPUT else "accumulator" if flags & FLAG_ACC else "result")
    return {"result": v, "kept": kept, "dropped": dropped, "distances": dists, "coefficients": coefs,
            "clipped": counts}
