"""The two-slot table ring (csrc/call_tables.h, ``TableRing``) under the five entry points that had no
case crossing its slots with launches in flight: the Krum distances, the point distances, the fold
about a point, the moments about a point and the fused fold-and-step.

Each case makes five calls on one context and one stream with no synchronisation and no flag read
in between. The client counts come from the source (tests/ring_values.py restates the arithmetic):
the first call's tables fit a slot's first 64 KiB, the second call's outgrow them on the other slot,
the third call frees and regrows the first slot while the second call's launches are in flight, and
the fourth and fifth calls reuse the grown slots (the fifth only fits because its slot regrew). A
table that is freed or overwritten while a launch still reads it shows as wrong bits in that
launch's output. After one final synchronisation every output equals the module's numpy
restatement bit for bit and the NaN words are clear.

The layout is many tiny segments, which makes tables large while a call stays a few kilobytes per
client: segments of 8 elements (whole 16-byte vectors) and one of ``span + 5`` (a second span with
a ragged tail). Every client is a row of one buffer whose row length is odd, so the rows alternate
between 16-byte aligned and misaligned storage; every pointer is a view that ends inside its buffer.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, ModelLayout, _native
from tests import clip_reference as cref
from tests import geomed_reference as geo
from tests import krum_reference as kref
from tests import opt_reference as oref
from tests import ring_values as ring
from tests import trust_reference as tref
from tests.robust_values import assert_same_bits

pytestmark = pytest.mark.gpu

# entry -> (the span constant, segments, the five client counts); Krum takes at most 256 clients, so
# its tables outgrow 64 KiB only with more than 32 segments
CASES = {
    "krum": ("krum_chunk", 40, (4, 256, 230, 6, 215)),
    "point": ("point_chunk", 9, (3, 1024, 950, 5, 930)),
    "clip": ("clip_tile", 9, (3, 1024, 950, 5, 930)),
    "trust": ("trust_chunk", 9, (3, 1024, 950, 5, 930)),
    "opt": ("opt_tile", 9, (3, 1024, 950, 5, 930)),
}
HYPER = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)


def sizes_of(span: int, T: int) -> list[int]:
    return [8, span + 5] + [8] * (T - 2)


@functools.lru_cache(maxsize=None)
def pool(span: int, T: int, n: int, krum: bool) -> np.ndarray:
    """float32 [n, elements]: the clients every call of a case draws from (computed once and left
    unchanged). The values make the reference exact and its summation order visible."""
    total = sum(sizes_of(span, T))
    gen = torch.Generator().manual_seed(977 + span + T)
    if krum:
        v = torch.stack([kref.order_sensitive_values(gen, total) for _ in range(n)])
    else:
        v = geo.order_sensitive_values(gen, n * total, torch.float32).reshape(n, total)
    x = v.to(torch.float32)
    assert torch.equal(x.to(torch.float64), v.to(torch.float64))
    return x.numpy()


def segments(row, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [row[int(offs[t]):int(offs[t + 1])] for t in range(len(sizes))]


@functools.lru_cache(maxsize=None)
def pool_oracle(entry: str, span: int, T: int, n: int):
    """The per-client (Krum: per-pair) results over the whole pool: each is computed from its own
    client (pair) alone, so a call's expectation is the entries of its clients."""
    sizes = sizes_of(span, T)
    x = pool(span, T, n, entry == "krum")
    rows = [segments(r, sizes) for r in x]
    z, g = point_of(span, T)
    if entry == "krum":
        return kref.distances_in_order([[torch.from_numpy(s) for s in r] for r in rows], span).numpy()
    if entry == "point":
        return geo.distances_in_order(rows, segments(z, sizes), geo.native_constants(_native.kernel_constant), torch.float32)
    return tref.moments_in_order(rows, segments(z, sizes), segments(g, sizes), tref.native_constants(_native.kernel_constant),
                                 torch.float32)


@functools.lru_cache(maxsize=None)
def point_of(span: int, T: int):
    """A float64 point and direction (moments: m and v) over the layout."""
    total = sum(sizes_of(span, T))
    gen = torch.Generator().manual_seed(31 + span)
    z = geo.order_sensitive_values(gen, total, torch.float64).numpy()
    g = geo.order_sensitive_values(gen, total, torch.float64).numpy()
    return z, g


@pytest.mark.parametrize("entry", list(CASES))
def test_five_calls_back_to_back_cross_and_regrow_the_slots(hip_device, entry):
    name, T, counts = CASES[entry]
    span = _native.kernel_constant(name)
    sizes = sizes_of(span, T)
    needs = [ring.table_bytes(entry, n, T) for n in counts]
    assert ring.slot_events(needs) == ["first", "first", "regrow", "fit", "fit"], needs
    assert needs[0] <= ring.FIRST_SLOT < min(needs[1], needs[2], needs[4]), needs

    nmax = max(counts)
    host = pool(span, T, nmax, entry == "krum")
    dev = torch.from_numpy(host).to(hip_device)
    assert host.shape[1] % 4 == 1                      # odd rows start off a 16-byte boundary
    views = [segments(dev[c], sizes) for c in range(nmax)]
    z, g = point_of(span, T)
    zd, gd = (segments(torch.from_numpy(a).to(hip_device), sizes) for a in (z, g))
    zh, gh = segments(z, sizes), segments(g, sizes)
    total = host.shape[1]

    calls = []                                          # (table, clients, coefficients, expectation)
    for i, n in enumerate(counts):
        first = (7 * i) % (nmax - n + 1)                # other clients in every call
        who = list(range(first, first + n))
        coef = [1.0 + (c % 5) / 4.0 for c in who]
        table = ClientTable(T)
        for c in who:
            table.add_client(views[c], [1.0] * T)
        rows = [segments(host[c], sizes) for c in who]
        if entry == "krum":
            want = [pool_oracle(entry, span, T, nmax)[np.ix_(who, who)]]
        elif entry == "point":
            want = [pool_oracle(entry, span, T, nmax)[who]]
        elif entry == "trust":
            want = [m[who] for m in pool_oracle(entry, span, T, nmax)]
        elif entry == "clip":
            outs, flags = cref.fold_about_point(rows, coef, float(n), zh)
            assert flags == 0
            want = [np.concatenate(outs)]
        else:
            outs, ms, vs, flags = oref.step(rows, coef, float(n), zh, gh, [np.abs(a) for a in gh], "adam", **HYPER)
            assert flags == 0
            want = [np.concatenate(a) for a in (outs, ms, vs)]
        calls.append((table, n, coef, want))

    ctx = FedAvgContext(ModelLayout(names=tuple(f"t{i}" for i in range(T)), shapes=tuple((s,) for s in sizes)), hip_device)
    try:
        vd = [a.abs() for a in gd]
        fresh = [[torch.empty(total, dtype=torch.float64, device=hip_device) for _ in range(3)] for _ in calls]
        torch.cuda.synchronize(hip_device)
        got = []
        for (table, n, coef, _), bufs in zip(calls, fresh):  # back to back: no flag read, no synchronise
            if entry == "krum":
                got.append([ctx.pairwise_sqdist(table, torch.float32)])
            elif entry == "point":
                got.append([ctx.sqdist_to_point(table, torch.float32, zd)])
            elif entry == "trust":
                got.append(list(ctx.moments_about_point(table, torch.float32, zd, gd)))
            elif entry == "clip":
                ctx.fold_about_point(table, torch.float32, coef, float(n), zd, segments(bufs[0], sizes))
                got.append(bufs[:1])
            else:
                o, mo, vo = (segments(b, sizes) for b in bufs)
                ctx.server_opt_step(table, torch.float32, coef, float(n), zd, gd, vd, mo, vo, o, mode="adam", **HYPER)
                got.append(bufs)
        assert ctx.flags() == 0                         # the one synchronisation; the NaN words are clear
        for i, ((_, n, _, want), have) in enumerate(zip(calls, got)):
            assert len(have) == len(want)
            for k, (h, w) in enumerate(zip(have, want)):
                assert_same_bits(h.cpu().numpy().reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1),
                                 f"{entry}, call {i} (n = {n}), output {k}")
    finally:
        ctx.close()
