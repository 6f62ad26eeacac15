"""An independent restatement of the server optimiser contract in numpy, written
from the document and not from the package: the fold about the previous model as a loop over
clients, then one numpy operation per line of the contract, no torch arithmetic. Test support only
(no test in this file).

Per element, everything float64:
    d_i = x_i - z;  p_i = c_i * d_i;  acc = p_0 then acc + p_i in table order;  delta = acc / divisor
    avgm:     a = beta1 * m;  m' = a + delta;                                 u = lr * m'
    others:   a = beta1 * m;  b = omb1 * delta;  m' = a + b;  q = delta * delta
      adagrad:  v' = v + q
      adam:     e = beta2 * v;  f = omb2 * q;  v' = e + f
      yogi:     g = v - q;  s = +1 if g > 0, -1 if g < 0, else +0;  f = omb2 * q;  h = f * s;  v' = v - h
      r = sqrt(v');  den = r + tau;  num = lr * m';  u = num / den
    out = z + u
numpy's elementwise operators never fuse, ``np.sqrt`` and ``/`` are the correctly rounded IEEE
operations, and a float32 output is ``astype`` (round to nearest even).
"""

from __future__ import annotations

import numpy as np

from tests import geomed_reference as geo

FLAG_ACC, FLAG_RESULT, FLAG_INPUT = 0x1, 0x2, 0x8
MODES = ("avgm", "adagrad", "yogi", "adam")


def one_minus(beta: float) -> float:
    """1 - beta as the host computes it once."""
    return float(np.float64(1.0) - np.float64(beta))


def step(clients, coefficients, divisor, point, m, v, mode, lr, beta1, beta2, tau, out_dtype=np.float64):
    """``clients[i]`` is client i's tensors in layout order; ``point``, ``m`` and ``v`` (``None`` for
    avgm) one float64 tensor per segment. Returns (outs, m_new, v_new, flags): flat arrays per segment
    (``v_new`` is ``None`` for avgm) and the NaN flags the call latches (input: a NaN in a client, the
    point, m or v; acc: a NaN in the sum; result: a NaN in out, m' or v')."""
    assert mode in MODES
    flags = 0
    outs, ms, vs = [], [], []
    div = np.float64(divisor)
    lr, b1, b2, tau = np.float64(lr), np.float64(beta1), np.float64(beta2), np.float64(tau)
    omb1, omb2 = np.float64(one_minus(beta1)), np.float64(one_minus(beta2))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for t, z in enumerate(point):
            z = geo.as_f64(z)
            mt = geo.as_f64(m[t])
            vt = None if mode == "avgm" else geo.as_f64(v[t])
            if np.isnan(z).any() or np.isnan(mt).any() or (vt is not None and np.isnan(vt).any()):
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
            delta = acc / div
            a = b1 * mt
            if mode == "avgm":
                m_new = a + delta
                v_new = None
                u = lr * m_new
            else:
                b = omb1 * delta
                m_new = a + b
                q = delta * delta
                if mode == "adagrad":
                    v_new = vt + q
                elif mode == "adam":
                    e = b2 * vt
                    f = omb2 * q
                    v_new = e + f
                else:
                    g = vt - q
                    s = np.where(g > 0, np.float64(1.0), np.where(g < 0, np.float64(-1.0), np.float64(0.0)))
                    f = omb2 * q
                    h = f * s
                    v_new = vt - h
                r = np.sqrt(v_new)
                den = r + tau
                num = lr * m_new
                u = num / den
            out = z + u
            if np.isnan(out).any() or np.isnan(m_new).any() or (v_new is not None and np.isnan(v_new).any()):
                flags |= FLAG_RESULT
            outs.append(out.astype(out_dtype))
            ms.append(m_new)
            vs.append(v_new)
    return outs, ms, (None if mode == "avgm" else vs), flags


def rounds(all_clients, all_weights, start, mode, lr, beta1, beta2, tau, v0=None, out_dtype=np.float64):
    """Consecutive rounds of the plugin class on rows of tensors: ``all_clients[r]`` the clients of
    round r, ``all_weights[r]`` their weights, ``start`` the model before round 0 (one tensor per
    segment); every round's result is the next round's previous model, as a server feeds it back.
    ``v0`` defaults to tau squared. Returns per round (outs, m, v)."""
    z = [geo.as_f64(t) for t in start]
    m = [np.zeros_like(t) for t in z]
    v0 = float(np.float64(tau) * np.float64(tau)) if v0 is None else float(v0)
    v = None if mode == "avgm" else [np.full_like(t, v0) for t in z]
    history = []
    for clients, weights in zip(all_clients, all_weights):
        W = 0.0
        for w in weights:
            W = W + float(w)
        outs, m, v, flags = step(clients, weights, W, z, m, v, mode, lr, beta1, beta2, tau, out_dtype)
        assert flags == 0, flags
        history.append((outs, m, v))
        z = [geo.as_f64(o) for o in outs]
    return history
