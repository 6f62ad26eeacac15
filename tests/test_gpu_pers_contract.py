"""The personalized kernel (csrc/personalized_kernels.hip, ``personalized_kernel``) and its host half
(``fedavg_pers_aggregate``) against DESIGN.md §5b: the fold that the host's proof allows on both
sides of its bound, the refold of ±0 / NaN sums, every bit pattern of the 16-bit input formats, that
nothing but the output elements is written, the LDS ring at its own edges, and the one table blob
with launches in flight. Every comparison is bit for bit with tests/pers_reference.py; no tolerance
anywhere. A NaN compares as a NaN: the same NaN mask and identical bits elsewhere, and ``check()``
must report exactly the flag bits that the reference's NaN verdicts imply.

The cases are ``tests/pers_values``'; tests/test_pers_values_host.py shows on the CPU that an exact
fused chain differs from the reference in at least a tenth of the elements of a receiver whose
weights are one bit past the bound, and that the main loop without its refold misses exactly the
planted elements of every refold case.

The kernel is driven through ``PersonalizedContext.aggregate``, so a test chooses receiver rows and
ids freely. Sizes come from the build's own geometry (``fedavg_kernel_constant``). No input asks the
kernel to read or write past a tensor: every pointer is a whole torch tensor or a view that ends
inside its buffer, and the elements around every output are checked to be untouched.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import ModelLayout, _native
from distributed_learning_simulation_lib_amd.personalized import FlatOutputs, PersonalizedContext
from tests import pers_reference as pref
from tests import pers_values as pv
from tests import robust_values as rv
from tests.robust_values import SENTINEL, Outs, assert_same_bits, bits, place

pytestmark = pytest.mark.gpu

DTYPES = rv.DTYPES
NP_OUT = {"f64": np.float64, "f32": np.float32}
VE = 4      # elements per lane (the kernel's Raw loaders move four)


def constant(name: str) -> int:
    return _native.kernel_constant(name)


def geometry() -> dict:
    return {k: constant(f"pers_{n}") for k, n in (("chunk", "chunk"), ("jb", "jb"), ("group", "group"), ("u", "u"),
                                                  ("stage", "ring_stage"), ("depth", "ring_depth"))}


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def same(got, want, what: str) -> None:
    """The same NaN mask, and the same bits wherever there is no NaN."""
    g, w = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(g), np.isnan(w)
    assert np.array_equal(gn, wn), f"{what}: NaN at {np.flatnonzero(gn).tolist()[:8]}, want {np.flatnonzero(wn).tolist()[:8]}"
    assert_same_bits(np.where(gn, 0, g), np.where(wn, 0, w), what)


class Launch:
    """The device side of one ``aggregate`` call of a case: the clients narrowed to the input
    format, and — unless the test brings its own outputs — one sentinel-filled buffer per receiver
    and one for the centralized model, every segment at a 16-byte boundary with sentinels in the
    gaps. Nothing here synchronises after ``issue``; ``collect`` reads the results back."""

    def __init__(self, case: pv.Case, code: str, device, misalign: bool = False, out: str = "f64",
                 central: str | None = "f64") -> None:
        self.case, self.code, self.out, self.central = case, code, out, central
        self.sizes = case.sizes
        self.dev = [[None if x is None else place(torch.from_numpy(x).to(DTYPES[code]), device, misalign) for x in row]
                    for row in case.clients]
        padded = [(s + 3) // 4 * 4 for s in self.sizes]
        self.offsets = [int(v) for v in np.cumsum([0] + padded[:-1])]
        M, width = len(case.receiver_ids), sum(padded)
        self.out_buf = torch.full((M, width), SENTINEL, dtype=DTYPES[out], device=device)
        self.central_buf = None if central is None else torch.full((width,), SENTINEL, dtype=DTYPES[central], device=device)
        self.mask = np.zeros(width, dtype=bool)
        for o, s in zip(self.offsets, self.sizes):
            self.mask[o:o + s] = True

    def issue(self, ctx: PersonalizedContext) -> None:
        c = self.case
        ctx.aggregate(self.dev, DTYPES[self.code], c.client_ids, c.weights, c.receiver_ids,
                      FlatOutputs([self.out_buf[j] for j in range(self.out_buf.shape[0])], self.offsets), DTYPES[self.out],
                      None if self.central is None else FlatOutputs([self.central_buf], self.offsets),
                      DTYPES[self.central or "f64"])

    def collect(self):
        """([M][T] arrays, [T] arrays or None); the gaps are checked to be untouched."""
        host = self.out_buf.cpu().numpy()
        assert (host[:, ~self.mask] == SENTINEL).all(), "a gap between two outputs was written"
        outs = [[row[o:o + s] for o, s in zip(self.offsets, self.sizes)] for row in host]
        if self.central is None:
            return outs, None
        c = self.central_buf.cpu().numpy()
        assert (c[~self.mask] == SENTINEL).all(), "a gap of the centralized buffer was written"
        return outs, [c[o:o + s] for o, s in zip(self.offsets, self.sizes)]


def check_against(ref: pref.Result, outs, central, out: str, central_code: str | None, what: str) -> None:
    for t, want in enumerate(ref.stacked):         # all receivers of a segment at once
        got = np.stack([row[t] for row in outs])
        with np.errstate(all="ignore"):
            want = want.astype(NP_OUT[out])
        gn, wn = np.isnan(got), np.isnan(want)
        if not (np.array_equal(gn, wn) and np.array_equal(bits(np.where(gn, 0, got)), bits(np.where(wn, 0, want)))):
            for j in range(len(outs)):             # name the first row that differs
                same(got[j], want[j], f"{what}: receiver row {j}, segment {t}")
            raise AssertionError(f"{what}: segment {t} differs")
    if central is not None:
        for t, got in enumerate(central):
            with np.errstate(all="ignore"):
                want = ref.central[t].astype(NP_OUT[central_code])
            same(got, want, f"{what}: centralized, segment {t}")


def run_case(ctx, case: pv.Case, code: str, device, ref: pref.Result | None = None, misalign: bool = False,
             out: str = "f64", central: str | None = "f64", what: str = ""):
    """One call, checked against the reference: every receiver, the centralized model, the flags."""
    ref = ref or case.reference()
    launch = Launch(case, code, device, misalign, out, central)
    launch.issue(ctx)
    flags = ctx.check()
    outs, cen = launch.collect()
    what = f"{what} {case.name} ({code})"
    check_against(ref, outs, cen, out, central, what)
    assert flags == (ref.flags if central is not None else ref.flags_no_central), (what, flags, ref.flags)
    return outs, cen


# ---- P1. the fold that the proof allows, on both sides of its bound --------------------------------
@pytest.mark.parametrize("code", list(pv.FOLD_BOUND))
def test_fold_at_the_bound_fused_or_not(hip_device, code):
    """(a) every weight b* = 53 - sig bits wide: the host may fuse, and the result is the
    reference's whether it does (``set_fused_fold(True)``) or is told not to. (c) the same with a
    53-bit weight on every pair that is a receiver's own update: the host skips those pairs before
    it measures a weight."""
    chunk = constant("pers_chunk")
    ctx = PersonalizedContext(layout_of([chunk + 3]), hip_device)
    try:
        for case in (pv.fold_case(code, chunk, 4, None), pv.own_wide_case(code, chunk)):
            ref = case.reference()
            assert ref.flags == 0
            for fused in (True, False):
                ctx.set_fused_fold(fused)
                run_case(ctx, case, code, hip_device, ref, what=f"fused={fused}")
    finally:
        ctx.close()


@pytest.mark.parametrize("where", ["first_row", "second_wave", "second_launch"])
@pytest.mark.parametrize("code", list(pv.FOLD_BOUND))
def test_one_bit_past_the_bound_is_folded_separately(hip_device, code, where):
    """(b) one receiver's weights are b* + 1 bits wide: its products round, so the whole call must
    take the separately rounded fold. A fused fold differs from the reference in at least a tenth of
    that receiver's elements (tests/test_pers_values_host.py)."""
    chunk, jb, group = constant("pers_chunk"), constant("pers_jb"), constant("pers_group")
    row = {"first_row": 0, "second_wave": jb, "second_launch": group}[where]
    case = pv.fold_case(code, chunk, group + 1, row)
    ctx = PersonalizedContext(layout_of([chunk + 3]), hip_device)
    try:
        ref = case.reference()
        assert ref.flags == 0
        run_case(ctx, case, code, hip_device, ref, what=where)
    finally:
        ctx.close()


@pytest.mark.parametrize("ring", [None, "1"])
def test_fp64_inputs_are_never_fused(hip_device, ring, monkeypatch):
    """(d) ``sig_bits`` of fp64 is 53 and a non-zero weight has at least one bit, so fp64 inputs
    always take the separately rounded fold — with integer weights 1 to 500 too, and with the ring
    asked for (``personalized_kernel<double, PF_FMA, *>`` is unreachable)."""
    if ring is None:
        monkeypatch.delenv("FEDAVG_PERS_RING", raising=False)
    else:
        monkeypatch.setenv("FEDAVG_PERS_RING", ring)   # read when the native context is created
    chunk, jb = constant("pers_chunk"), constant("pers_jb")
    sizes = [chunk, chunk + 3]
    case = pv.table_case("f64", "int", 9, jb + 1, sizes, seed=4500)
    assert case.weights.min() >= 1 and case.weights.max() <= 500
    ctx = PersonalizedContext(layout_of(sizes), hip_device)
    try:
        run_case(ctx, case, "f64", hip_device)
    finally:
        ctx.close()


@pytest.mark.parametrize("code", list(pv.FOLD_BOUND))
def test_weights_beyond_the_proofs_exponent_range(hip_device, code):
    """(e) 2^900 and 2^-900: ``weight_bits`` refuses them (``tame`` is false)."""
    chunk = constant("pers_chunk")
    case = pv.untame_case(code, chunk)
    ctx = PersonalizedContext(layout_of([chunk + 3]), hip_device)
    try:
        run_case(ctx, case, code, hip_device)
    finally:
        ctx.close()


# ---- P2. the refold --------------------------------------------------------------------------------
def refold_sizes() -> list[int]:
    chunk = constant("pers_chunk")
    return [3, chunk, chunk + 1]


@functools.lru_cache(maxsize=None)
def refold_cases_with_reference(code: str, kind: str, sizes: tuple, jb: int, group: int, part: str):
    """Built once and shared by the aligned, the misaligned and the ring runs; left unchanged."""
    return [(case, case.reference()) for case in pv.refold_cases(code, kind, list(sizes), jb, group, part)]


def check_refold(ctx, code: str, kind: str, device, misalign: bool, part: str) -> None:
    sizes = refold_sizes()
    for case, ref in refold_cases_with_reference(code, kind, tuple(sizes), constant("pers_jb"), constant("pers_group"), part):
        outs, _ = run_case(ctx, case, code, device, ref, misalign, what=f"{kind} misalign={misalign}")
        for j, t, idx, value in case.expect:       # the sign of a zero, spelled out
            assert_same_bits(outs[j][t][idx], np.full(len(idx), value), f"{case.name}: row {j}, segment {t}")
        for j in case.finite_rows:
            assert all(np.isfinite(o).all() for o in outs[j]), (case.name, j)
        for j, t, idx in case.planted:
            assert not len(pref.differing(outs[j][t][idx], ref.outs[j][t][idx])), (case.name, j, t)


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("kind", ["int", "frac"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_zero_and_nan_sums_are_refolded(hip_device, code, kind, misalign):
    """The cases of ``pers_values.refold_cases`` with a handful of receivers: (i) a -0.0 sum beside
    an own update of +1.0, and beside padding clients; (ii) an own update of +inf, -inf and NaN with
    one receiver: finite, no flag; (iv) x and -x: +0.0; (v) an absent tensor of a client whose other
    segment holds inf. Integer weights take the fused fold (but for fp64), the fractional ones the
    separately rounded fold."""
    ctx = PersonalizedContext(layout_of(refold_sizes()), hip_device)
    try:
        check_refold(ctx, code, kind, hip_device, misalign, "few")
    finally:
        ctx.close()


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("kind", ["int", "frac"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_poisoned_own_update_in_every_wave_and_launch(hip_device, code, kind, misalign):
    """(iii) the receiver of (ii) at rows 0, jb - 1, jb, group - 1 and group among group + 1: that
    row equals the reference and is finite; the others, which weigh the poisoned client with a real
    weight, carry the reference's inf / NaN, and the flags are the reference's verdict."""
    ctx = PersonalizedContext(layout_of(refold_sizes()), hip_device)
    try:
        check_refold(ctx, code, kind, hip_device, misalign, "many")
    finally:
        ctx.close()


@pytest.mark.parametrize("part", ["few", "many"])
def test_zero_and_nan_sums_are_refolded_on_the_ring(hip_device, part, monkeypatch):
    monkeypatch.setenv("FEDAVG_PERS_RING", "1")   # read when the native context is created
    ctx = PersonalizedContext(layout_of(refold_sizes()), hip_device)
    try:
        check_refold(ctx, "f32", "int", hip_device, False, part)
    finally:
        ctx.close()


# ---- P3. every 16-bit pattern widens exactly -------------------------------------------------------
@pytest.mark.parametrize("weight", [1.0, 3.0])
@pytest.mark.parametrize("code", ["f16", "bf16"])
def test_all_16_bit_patterns_widen_exactly(hip_device, code, weight):
    """One client and one receiver with another id: out = x * w / w, exact for w = 1 and w = 3 (a
    two-bit weight: the fused fold), so the fp64 output is the exact widening of every non-NaN
    pattern — infinities, zeros of both signs (through the refold) and subnormals included."""
    t, replaced = rv.all_patterns_16(DTYPES[code])
    assert replaced == {"f16": 2046, "bf16": 254}[code] and t.numel() == 65536
    ctx = PersonalizedContext(layout_of([t.numel()]), hip_device)
    try:
        out = torch.full((t.numel(),), SENTINEL, dtype=torch.float64, device=hip_device)
        ctx.aggregate([[t.to(hip_device)]], DTYPES[code], [0], np.array([[weight]]), [pv.OUTSIDER], [[out]])
        assert ctx.check() == 0
        assert_same_bits(out, t.to(torch.float64), f"{code} widening, weight {weight}")
    finally:
        ctx.close()


# ---- P4. nothing else is touched -------------------------------------------------------------------
class FlatGuarded:
    """One sentinel-filled buffer per row; segment 0 starts after four guard elements, segment 1 at
    an odd element (no output of the call is 16-byte aligned: every chunk takes the guarded path),
    and every gap and the tail hold sentinels."""

    def __init__(self, rows: int, sizes, dtype, device) -> None:
        self.sizes = sizes
        self.offsets, at = [], 4
        for i, s in enumerate(sizes):
            if i == 1 and at % 2 == 0:
                at += 1
            self.offsets.append(at)
            at += s + 2
        assert self.offsets[1] % 2 == 1
        self.bufs = [torch.full((at + 2,), SENTINEL, dtype=dtype, device=device) for _ in range(rows)]
        self.mask = np.zeros(at + 2, dtype=bool)
        for o, s in zip(self.offsets, sizes):
            self.mask[o:o + s] = True
        self.arg = FlatOutputs(self.bufs, self.offsets)

    def guards_untouched(self) -> bool:
        return all(bool((b.cpu().numpy()[~self.mask] == SENTINEL).all()) for b in self.bufs)

    def rows(self):
        return [[b.cpu().numpy()[o:o + s] for o, s in zip(self.offsets, self.sizes)] for b in self.bufs]


class SeparateGuarded:
    """One guarded tensor per row and segment (``robust_values.Outs``), 16-byte aligned."""

    def __init__(self, rows: int, sizes, dtype, device) -> None:
        self.outs = [Outs(sizes, dtype, device, False) for _ in range(rows)]
        self.arg = [o.views for o in self.outs]

    def guards_untouched(self) -> bool:
        return all(o.guards_untouched() for o in self.outs)

    def rows(self):
        return [o.numpy() for o in self.outs]


@pytest.mark.parametrize("central", ["f64", "f32", None])
@pytest.mark.parametrize("out", ["f64", "f32"])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("code", ["f32", "f16"])
def test_only_the_output_elements_are_written(hip_device, code, flat, out, central):
    chunk = constant("pers_chunk")
    case, (who, seg, at), new = pv.isolation_case(code, chunk, VE)
    sizes, M = case.sizes, len(case.receiver_ids)
    dev = [[torch.from_numpy(x).to(DTYPES[code]).to(hip_device) for x in row] for row in case.clients]
    before = [[bits(t).copy() for t in row] for row in dev]
    kind = FlatGuarded if flat else SeparateGuarded
    ctx = PersonalizedContext(layout_of(sizes), hip_device)
    try:
        def run(ref):
            o = kind(M, sizes, DTYPES[out], hip_device)
            c = None if central is None else kind(1, sizes, DTYPES[central], hip_device)
            ctx.aggregate(dev, DTYPES[code], case.client_ids, case.weights, case.receiver_ids, o.arg, DTYPES[out],
                          None if c is None else (c.arg if flat else c.arg[0]), DTYPES[central or "f64"])
            assert ctx.check() == 0
            assert o.guards_untouched() and (c is None or c.guards_untouched())
            outs, cen = o.rows(), None if c is None else c.rows()[0]
            check_against(ref, outs, cen, out, central, f"{code} flat={flat}")
            return outs, cen

        outs, cen = run(case.reference())
        for row, b in zip(dev, before):
            for t, w in zip(row, b):
                assert np.array_equal(bits(t), w), "a client tensor changed"
        # one element of one client changes: exactly that element follows in every receiver that
        # weighs the client, and in the centralized model; its own receiver does not see it
        changed = pv.Case(case.name, [[x.copy() for x in row] for row in case.clients], case.client_ids, case.weights,
                          case.receiver_ids)
        changed.clients[who][seg][at] = new
        dev[who][seg][at] = new
        outs2, cen2 = run(changed.reference())
        follows = [j for j in range(M) if case.receiver_ids[j] != case.client_ids[who] and case.weights[j, who] != 0]
        assert sorted(set(range(M)) - set(follows)) == [2, 4]
        for j in range(M):
            for t in range(len(sizes)):
                differs = np.flatnonzero(bits(outs2[j][t]) != bits(outs[j][t])).tolist()
                assert differs == ([at] if t == seg and j in follows else []), (j, t, differs)
        if cen is not None:
            for t in range(len(sizes)):
                differs = np.flatnonzero(bits(cen2[t]) != bits(cen[t])).tolist()
                assert differs == ([at] if t == seg else []), (t, differs)
    finally:
        ctx.close()


# ---- P5. the ring at its own edges -----------------------------------------------------------------
@pytest.mark.parametrize("i", range(9))
def test_ring_edges_equal_the_reference_and_the_register_pipeline(hip_device, i, monkeypatch):
    """``FEDAVG_PERS_RING=1``, fp32, integer weights 1 to 500: client count i of
    ``pers_values.ring_client_counts`` (1 stage, 2, ``depth``, ``depth + 1`` stages, one full wrap of
    the ring) with one wave, with two, and with three or four (``ring_pairs``). [chunk,
    2 * chunk + 5] elements: whole aligned chunks on the ring and a ragged chunk on the guarded path
    in one launch; the last client did not send segment 0 (the zero block is DMAed); every receiver
    that can be is a client. Each result equals the reference and, bit for bit, what a context
    created with ``FEDAVG_PERS_RING=0`` returns for the same tables."""
    geo = geometry()
    counts = pv.ring_client_counts(geo["stage"], geo["depth"])
    assert len(counts) == 9
    sizes = [geo["chunk"], 2 * geo["chunk"] + 5]
    monkeypatch.setenv("FEDAVG_PERS_RING", "1")   # read when the native context is created
    ring = PersonalizedContext(layout_of(sizes), hip_device)
    monkeypatch.setenv("FEDAVG_PERS_RING", "0")
    plain = PersonalizedContext(layout_of(sizes), hip_device)
    try:
        for n, m in [p for p in pv.ring_pairs(geo["jb"], geo["stage"], geo["depth"]) if p[0] == counts[i]]:
            case = pv.table_case("f32", "int", n, m, sizes, seed=4600 + 64 * i + m)
            ref = case.reference()
            assert ref.flags == 0
            a, ca = run_case(ring, case, "f32", hip_device, ref, what=f"ring {n} x {m}")
            b, cb = run_case(plain, case, "f32", hip_device, ref, what=f"registers {n} x {m}")
            for t in range(len(sizes)):
                assert_same_bits(np.stack([r[t] for r in a]), np.stack([r[t] for r in b]),
                                 f"{n} x {m}: ring against registers, segment {t}")
                assert_same_bits(ca[t], cb[t], f"{n} x {m}: ring against registers, centralized, segment {t}")
    finally:
        ring.close()
        plain.close()


# ---- P6. the one table blob with launches in flight ------------------------------------------------
def test_five_tables_back_to_back_without_a_synchronisation(hip_device):
    """One pinned and one device blob serve every call: the host waits for the previous call's copy
    (``blob_done``), not for its kernels, before it rewrites the pinned image, and the device copy
    of the next call is ordered behind those kernels by the stream alone. A call that outgrows the
    blob frees and regrows it. From the source (``pers_values.blob_bytes``): the first blob is
    64 KiB; call 1 (4 clients, 3 receivers) fits, call 2 (40 clients, group + 1 receivers: two launch
    groups) does not and regrows it to twice its need, which the later calls fit. Calls 2 to 4 have
    more than one launch group and share ``d_carry``. Five calls with nothing between them that reads
    a flag or synchronises; every call has its own outputs; all are checked at the end."""
    geo = geometry()
    group = geo["group"]
    sizes = [geo["chunk"] + 1, 7]
    plan = [(4, 3), (40, group + 1), (5, 2 * group + 1), (40, group + 1), (4, 3)]
    need = [pv.blob_bytes(n, m, len(sizes), geo) for n, m in plan]
    assert need[0] <= pv.FIRST_BLOB < need[1], need            # the second call regrows, not the first
    assert max(need[2:]) <= 2 * need[1], need                  # ... and nobody after it
    assert [m > group for _, m in plan] == [False, True, True, True, False]
    ctx = PersonalizedContext(layout_of(sizes), hip_device)
    try:
        cases = [pv.table_case("f32", "frac" if i % 2 else "int", n, m, sizes, seed=4700 + i, own_rows=3)
                 for i, (n, m) in enumerate(plan)]
        refs = [c.reference() for c in cases]
        assert all(r.flags == 0 for r in refs)
        launches = [Launch(c, "f32", hip_device) for c in cases]
        torch.cuda.synchronize(hip_device)
        for launch in launches:                                # back to back: no flag read, no synchronise
            launch.issue(ctx)
        assert ctx.check() == 0
        for i, (launch, ref) in enumerate(zip(launches, refs)):
            outs, cen = launch.collect()
            check_against(ref, outs, cen, "f64", "f64", f"call {i + 1} {plan[i]}")
    finally:
        ctx.close()
