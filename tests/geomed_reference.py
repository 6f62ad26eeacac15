"""An independent restatement of the geometric-median contract in numpy, written
from the document and not from the package: the order-following squared distance to a point, the
finite screen, the Weiszfeld loop, and an exact distance in rational arithmetic for the error bound.
Test support only (no test in this file).

The pinned order, with C = "point_chunk", L = "point_threads", N = "point_ae_<d>" of the client
dtype: every segment is cut into chunks of C elements (the last one padded with +0.0 on both the
client's and the point's side); in a chunk, lane l owns the positions (k * L + l) * N + i for
k = 0 .. C / (N * L) - 1 and i = 0 .. N - 1 and adds (x - z)^2 over them in that order into one
accumulator that starts at +0.0; a wave is 64 consecutive lanes and is folded by
a[l] <- a[l] + a[l + off] for l < off, off = 32, 16, 8, 4, 2, 1; the waves are added in wave order;
the chunk sums are added one after another, from +0.0, segment by segment in ascending offset.
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

DEFAULT_CONSTANTS = {"chunk": 4096, "threads": 256, "ae": {"f32": 4, "f16": 8, "bf16": 8, "f64": 2}}
INF = float("inf")


class GeomedNaN(Exception):
    def __init__(self, stage: str, rows=()):
        super().__init__(stage)
        self.stage = stage
        self.rows = list(rows)


def native_constants(kernel_constant) -> dict:
    """The same dictionary read from the built library (``_native.kernel_constant``)."""
    return {"chunk": kernel_constant("point_chunk"), "threads": kernel_constant("point_threads"),
            "ae": {d: kernel_constant(f"point_ae_{d}") for d in ("f32", "f16", "bf16", "f64")}}


def as_f64(t) -> np.ndarray:
    """Any tensor or array as a flat float64 numpy array (an exact conversion for every format)."""
    if hasattr(t, "detach"):
        import torch

        t = t.detach().to("cpu").to(torch.float64).numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float64)).reshape(-1)


def dtype_tag(dtype) -> str:
    s = str(dtype).replace("torch.", "")
    return {"float32": "f32", "float16": "f16", "bfloat16": "bf16", "float64": "f64"}.get(s, s)


def order_sensitive_values(gen, numel: int, dtype):
    """float64 [numel], every value representable in the torch ``dtype``: a full-width random
    mantissa times 2^e, random sign, e over a few binades for the wide formats (every add of their
    48- or 106-bit squares rounds) and over 2^-6 .. 2^6 (float16) or 2^-30 .. 2^30 (bfloat16) for the
    narrow ones, whose squares must be spread over more than 53 bits before a sum rounds at all.
    tests/test_geomed_host.py shows that another summation order gives other bits on these values."""
    import torch

    span = {torch.float16: 6, torch.bfloat16: 30}.get(dtype, 2)
    e = torch.randint(-span, span + 1, (numel,), generator=gen).to(torch.float64)
    sign = torch.randint(0, 2, (numel,), generator=gen).to(torch.float64) * 2.0 - 1.0
    v = sign * (1.0 + torch.rand(numel, generator=gen, dtype=torch.float64)) * torch.exp2(e)
    return v.to(dtype).to(torch.float64)


def chunk_sum(q: np.ndarray, constants: dict, ae: int) -> np.float64:
    """One chunk's squares (already padded to the chunk) in the pinned lane / wave order."""
    C, L = constants["chunk"], constants["threads"]
    per_lane = C // (L * ae)
    assert per_lane * L * ae == C and L % 64 == 0
    lanes = np.zeros(L, dtype=np.float64)
    for k in range(per_lane):
        for i in range(ae):
            lanes = lanes + q[(k * L + np.arange(L)) * ae + i]
    total = None
    for w in range(L // 64):
        a = lanes[64 * w: 64 * w + 64].copy()
        off = 32
        while off:
            a[:off] = a[:off] + a[off: 2 * off]
            off //= 2
        total = a[0] if total is None else total + a[0]
    return total


def distances_in_order(clients, point, constants: dict, dtype) -> np.ndarray:
    """``out[i]`` of the contract: ``clients[i]`` is client i's tensors in layout order, ``point``
    one float64 tensor per segment or None (the origin). Raises GeomedNaN like the kernel's flags."""
    ae = constants["ae"][dtype_tag(dtype)]
    C = constants["chunk"]
    xs = [[as_f64(t) for t in c] for c in clients]
    zs = None if point is None else [as_f64(z) for z in point]
    bad = [i for i, c in enumerate(xs) if any(np.isnan(t).any() for t in c)]
    if bad or (zs is not None and any(np.isnan(z).any() for z in zs)):
        raise GeomedNaN("input", bad)
    out = np.zeros(len(xs), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, c in enumerate(xs):
            s = np.float64(0.0)
            for t, x in enumerate(c):
                z = np.zeros_like(x) if zs is None else zs[t]
                assert z.shape == x.shape
                for lo in range(0, x.size, C):
                    xc = np.zeros(C, dtype=np.float64)
                    zc = np.zeros(C, dtype=np.float64)
                    m = min(C, x.size - lo)
                    xc[:m] = x[lo: lo + m]
                    zc[:m] = z[lo: lo + m]
                    d = xc - zc
                    s = s + chunk_sum(d * d, constants, ae)
            out[i] = s
    if np.isnan(out).any():
        raise GeomedNaN("accumulator")
    return out


def exact_distance(client, point) -> Fraction:
    """sum (x - z)^2 over every element in rational arithmetic (finite values only)."""
    s = Fraction(0)
    for t, x in enumerate(client):
        x = as_f64(x)
        z = np.zeros_like(x) if point is None else as_f64(point[t])
        for a, b in zip(x.tolist(), z.tolist()):
            d = Fraction(a) - Fraction(b)
            s += d * d
    return s


def step(dist_sq, alpha, smoothing):
    """beta_i = alpha_i / max(nu, sqrt(D_i)) and G = sum alpha_i sqrt(D_i), added in arrival order."""
    beta, G = [], 0.0
    for D, a in zip(dist_sq, alpha):
        d = math.sqrt(float(D))
        beta.append(float(a) / (d if d > smoothing else smoothing))
        G = G + float(a) * d
    return beta, G


def fold(clients, weights, out_dtype=np.float64):
    """The FedAvg of the reference: per tensor acc = x * w added in arrival order, divided by the
    sequential sum of the weights; float32 is that rounded to nearest even."""
    total = 0.0
    for w in weights:
        total = total + float(w)
    outs = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(len(clients[0])):
            acc = None
            for c, w in zip(clients, weights):
                tmp = as_f64(c[t]) * np.float64(w)
                acc = tmp if acc is None else acc + tmp
            outs.append((acc / np.float64(total)).astype(out_dtype))
    return outs


def geometric_median(clients, alpha, constants: dict, dtype, max_iterations=3, smoothing=1e-6, tolerance=0.0,
                     out_dtype=np.float64) -> dict:
    """The whole rule on rows of tensors. Returns the result (flat arrays per tensor), the dropped
    rows, and per measured point the kept clients' distances, weights and objective."""
    norms = distances_in_order(clients, None, constants, dtype)
    kept = [i for i, v in enumerate(norms) if v != INF]
    dropped = [i for i, v in enumerate(norms) if v == INF]
    if not kept:
        raise ValueError("no finite client")
    rows = [clients[i] for i in kept]
    al = [float(alpha[i]) for i in kept]
    if all(a == 0 for a in al):
        raise ValueError("all weights zero")
    z = fold(rows, al)
    dists, betas, objs, folds = [], [], [], 0
    for t in range(1, max_iterations + 1):
        D = distances_in_order(rows, z, constants, dtype)
        beta, G = step(D, al, smoothing)
        dists.append(D.tolist())
        betas.append(beta)
        objs.append(G)
        if tolerance > 0 and t >= 2 and abs(objs[-2] - G) <= tolerance * G:
            break
        if all(b == 0 for b in beta):
            raise ValueError("all Weiszfeld weights zero")
        z = fold(rows, beta, out_dtype if t == max_iterations else np.float64)
        folds += 1
    return {"result": [a.astype(out_dtype) for a in z], "kept": kept, "dropped": dropped, "distances": dists,
            "betas": betas, "objectives": objs, "iterations": folds}
