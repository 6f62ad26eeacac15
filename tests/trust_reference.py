"""An independent restatement of the FLTrust contract in numpy, written from the
document and not from the package: the order-following dot and squared norm of every client's update
about a point, the score rule, the whole round, and an exact dot in rational arithmetic for the
error bound. The chunk order is §5i's (``tests/geomed_reference.chunk_sum``) and the step is §5j's
(``tests/clip_reference.fold_about_point``), both by import. Nothing here comes from the reference
project: FLTrust is not one of its algorithms. Test support only (no test in this file).

Per element, with v the centre and g the direction: d = x - v, q = d * d, p = d * g, each a separately
rounded float64 operation (numpy's elementwise operators never fuse). Both sums follow the pinned
order with C = "trust_chunk", L = "trust_threads", N = "trust_ae_<d>": chunks of C elements per
segment, the last one padded with x = v = g = +0.0; lane l adds the positions (k * L + l) * N + i in
ascending order from +0.0; the halving tree over 64 lanes; the waves in wave order; the chunk sums
one after another from +0.0, segment by segment in ascending offset.
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests import clip_reference as clip
from tests import geomed_reference as geo

DEFAULT_CONSTANTS = {"chunk": 4096, "threads": 256, "ae": {"f32": 4, "f16": 8, "bf16": 8, "f64": 2}}
INF = float("inf")


def native_constants(kernel_constant) -> dict:
    """The same dictionary read from the built library (``_native.kernel_constant``)."""
    return {"chunk": kernel_constant("trust_chunk"), "threads": kernel_constant("trust_threads"),
            "ae": {d: kernel_constant(f"trust_ae_{d}") for d in ("f32", "f16", "bf16", "f64")}}


def moments_in_order(clients, centre, direction, constants: dict, dtype, check: bool = True):
    """``(dots, sqnorms)`` of the contract: ``clients[i]`` is client i's tensors in layout order,
    ``centre`` one float64 tensor per segment or None (the origin), ``direction`` one float64 tensor
    per segment. With ``check`` it raises GeomedNaN like the kernel's flags; without, it returns the
    values, NaN included."""
    ae = constants["ae"][geo.dtype_tag(dtype)]
    C = constants["chunk"]
    xs = [[geo.as_f64(t) for t in c] for c in clients]
    vs = None if centre is None else [geo.as_f64(z) for z in centre]
    gs = [geo.as_f64(z) for z in direction]
    bad = [i for i, c in enumerate(xs) if any(np.isnan(t).any() for t in c)]
    if check and (bad or (vs is not None and any(np.isnan(z).any() for z in vs)) or any(np.isnan(z).any() for z in gs)):
        raise geo.GeomedNaN("input", bad)
    dots = np.zeros(len(xs), dtype=np.float64)
    sqs = np.zeros(len(xs), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, c in enumerate(xs):
            T = np.float64(0.0)
            S = np.float64(0.0)
            for t, x in enumerate(c):
                v = np.zeros_like(x) if vs is None else vs[t]
                g = gs[t]
                assert v.shape == x.shape and g.shape == x.shape
                for lo in range(0, x.size, C):
                    xc = np.zeros(C, dtype=np.float64)
                    vc = np.zeros(C, dtype=np.float64)
                    gc = np.zeros(C, dtype=np.float64)
                    m = min(C, x.size - lo)
                    xc[:m] = x[lo: lo + m]
                    vc[:m] = v[lo: lo + m]
                    gc[:m] = g[lo: lo + m]
                    d = xc - vc
                    S = S + geo.chunk_sum(d * d, constants, ae)
                    T = T + geo.chunk_sum(d * gc, constants, ae)
            dots[i] = T
            sqs[i] = S
    if check and (np.isnan(dots).any() or np.isnan(sqs).any()):
        raise geo.GeomedNaN("accumulator")
    return dots, sqs


def shuffled_dot(client, centre, direction, perm_seed: int) -> np.float64:
    """The same products added one after another in a shuffled order: what another summation order
    gives (the host tests show that it differs in bits on the order-sensitive generator)."""
    terms = []
    for t, x in enumerate(client):
        x = geo.as_f64(x)
        v = np.zeros_like(x) if centre is None else geo.as_f64(centre[t])
        terms.append((x - v) * geo.as_f64(direction[t]))
    p = np.concatenate(terms)
    p = p[np.random.default_rng(perm_seed).permutation(p.size)]
    s = np.float64(0.0)
    for a in p:
        s = s + a
    return s


def exact_dot(client, centre, direction) -> tuple[Fraction, Fraction]:
    """(sum (x - v) * g, sum |(x - v) * g|) over every element in rational arithmetic (finite values)."""
    s, a = Fraction(0), Fraction(0)
    for t, x in enumerate(client):
        x = geo.as_f64(x)
        v = np.zeros_like(x) if centre is None else geo.as_f64(centre[t])
        g = geo.as_f64(direction[t])
        for xe, ve, ge in zip(x.tolist(), v.tolist(), g.tolist()):
            p = (Fraction(xe) - Fraction(ve)) * Fraction(ge)
            s += p
            a += abs(p)
    return s, a


def coefficients(dots, sqnorms, root_sqnorm):
    """score_i = max(0, T_i / (sqrt(S_i) * sqrt(S_root))) and coef_i = score_i * (sqrt(S_root) /
    sqrt(S_i)); a client whose S_i is not finite or whose denominator is 0 gets 0 and 0."""
    n0 = math.sqrt(float(root_sqnorm))
    scores, coef = [], []
    for T, S in zip(dots, sqnorms):
        T, S = float(T), float(S)
        ni = math.sqrt(S) if math.isfinite(S) else INF
        den = ni * n0
        if ni == INF or den == 0.0:
            scores.append(0.0)
            coef.append(0.0)
            continue
        c = T / den
        s = c if c > 0 else 0.0
        scores.append(s)
        coef.append(s * (n0 / ni))
    return scores, coef


def fltrust(clients, root: int, previous, constants: dict, dtype, out_dtype=np.float64) -> dict:
    """The whole rule on rows of tensors: ``root`` is the root's row, ``previous`` the previous
    model (one float64 tensor per segment). Returns the result (flat arrays per tensor), the kept
    and dropped rows and, per kept row, the dot, the squared norm, the score and the coefficient."""
    norms = geo.distances_in_order(clients, None, constants, dtype)
    kept = [i for i, v in enumerate(norms) if v != INF]
    dropped = [i for i, v in enumerate(norms) if v == INF]
    if root not in kept:
        raise ValueError("no root")
    rows = [clients[i] for i in kept]
    v = [geo.as_f64(z) for z in previous]
    g = [geo.as_f64(x) - z for x, z in zip(clients[root], v)]
    dots, sqs = moments_in_order(rows, v, g, constants, dtype)
    pos = kept.index(root)
    if sqs[pos] == 0:
        raise ValueError("zero root")
    scores, coef = coefficients(dots, sqs, sqs[pos])
    W = 0.0
    for k, s in enumerate(scores):
        if k != pos:
            W = W + s
    if not W > 0:
        raise ValueError("no client is trusted")
    others = [k for k in range(len(kept)) if k != pos]
    out, flags = clip.fold_about_point([rows[k] for k in others], [coef[k] for k in others], W, v, out_dtype)
    if flags:
        raise geo.GeomedNaN("input" if flags & clip.FLAG_INPUT else "accumulator" if flags & clip.FLAG_ACC else "result")
    return {"result": out, "kept": kept, "dropped": dropped, "dots": dots.tolist(), "sqnorms": sqs.tolist(),
            "scores": scores, "coefficients": coef, "total_score": W}
