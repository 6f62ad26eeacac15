"""CPU proofs about the inputs of tests/test_gpu_fold_contract.py, with tests/pers_reference.py and the
pinned oracle alone (no GPU): a suite that compares bit for bit only catches a wrong fold if its
inputs tell the right one from the wrong one.

1. all weights at the bound: the exactly fused chain IS the two-rounding chain; one bit past it they
   differ in at least a tenth of the elements (six clients);
2. one wide weight among five at the bound, at a middle or the last client: at least 16 of 512
   elements differ; at client 0 none does (``fma(x, w, -0.0)`` is ``round(x * w)``);
3. the width of a weight as ``note_weight`` measures it, and what it calls tame;
4. a chain started from +0.0 differs from the oracle at exactly the planted elements of every
   signed-zero case.
"""

from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import nnadq_oracle
from tests import fold_values as fv
from tests import pers_reference as pref
from tests.pers_values import FOLD_BOUND, SIG, odd_weights
from tests.robust_values import bits

PROOF = 512


def chains(case: fv.Case, t: int = 0):
    xs, ws = case.chain_inputs(t)
    return pref.fused_chain(xs, ws), pref.separate_chain(xs, ws)


# ---- 1. the bound, all weights ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", fv.VARIANTS)
@pytest.mark.parametrize("code", fv.FUSABLE)
def test_at_the_bound_the_fused_chain_is_the_reference(code, variant):
    case = fv.bound_case(code, "at", variant, [PROOF])
    assert fv.fusable(case)
    fused, separate = chains(case)
    assert len(pref.differing(fused, separate)) == 0


@pytest.mark.parametrize("variant", fv.VARIANTS)
@pytest.mark.parametrize("code", fv.FUSABLE)
def test_one_bit_past_the_bound_a_tenth_of_the_elements_differ(code, variant):
    case = fv.bound_case(code, "past", variant, [PROOF])
    assert not fv.fusable(case)
    fused, separate = chains(case)
    assert len(pref.differing(fused, separate)) >= PROOF // 10 + 1


def test_fp64_inputs_two_bit_weights_differ_and_powers_of_two_cannot():
    for kind in ("pow2", "two_bit"):
        assert not fv.fusable(fv.f64_case(kind, [PROOF]))
    fused, separate = chains(fv.f64_case("two_bit", [PROOF]))
    assert len(pref.differing(fused, separate)) >= PROOF // 10 + 1
    fused, separate = chains(fv.f64_case("pow2", [PROOF]))       # exact products: nothing to tell apart
    assert len(pref.differing(fused, separate)) == 0


# ---- 2. the lone wide weight -----------------------------------------------------------------------
@pytest.mark.parametrize("place", fv.LONE_PLACES)
@pytest.mark.parametrize("code", fv.FUSABLE)
def test_a_lone_wide_weight_shows_in_16_of_512_elements(code, place):
    case = fv.lone_wide_case(code, place, [PROOF])
    assert not fv.fusable(case)
    widths = [fv.weight_bits(w) for w in case.weights[:, 0]]
    b = FOLD_BOUND[code]
    assert widths == {"middle_first": [b, b, b, b + 1, b, b], "last_last": [b] * 5 + [b + 1],
                      "cache": [b, b, b + 1, b + 1, b, b]}[place]
    if place == "cache":   # narrow, the same narrow, wide, the same wide, narrow
        w = case.weights[:, 0]
        assert w[0] == w[1] and w[2] == w[3] and len({w[1], w[2], w[4], w[5]}) == 4
    fused, separate = chains(case)
    assert len(pref.differing(fused, separate)) >= 16


@pytest.mark.parametrize("code", fv.FUSABLE)
def test_a_wide_weight_at_client_0_cannot_show(code):
    case = fv.lone_wide_case(code, "client0", [PROOF])
    assert not fv.fusable(case)
    fused, separate = chains(case)
    assert len(pref.differing(fused, separate)) == 0


def test_the_lone_wide_weight_sits_in_one_entry_of_a_large_tensor():
    for code in fv.FUSABLE:
        sizes = fv.bound_sizes(code)
        assert min(sizes[0], sizes[-1]) >= fv.geometry(code)["tile"]
        for place, entries in (("middle_first", [(3, 0)]), ("last_last", [(5, len(sizes) - 1)]), ("cache", [(2, 0), (3, 0)])):
            case = fv.lone_wide_case(code, place, sizes)
            wide = [(k, t) for k in range(fv.CLIENTS) for t in range(len(sizes))
                    if fv.weight_bits(case.weights[k, t]) > FOLD_BOUND[code]]
            assert wide == entries


# ---- 3. the width of a weight ----------------------------------------------------------------------
def test_weight_width_agrees_with_the_builder():
    rng = np.random.default_rng(11)
    for b in (1, 2, 13, 14, 28, 29, 30, 41, 42, 43, 44, 45, 46, 52, 53):
        for w in odd_weights(rng, 8, b):
            for v in (w, -w, w * 2.0 ** 40, w * 2.0 ** -40, -w * 2.0 ** 700, w * 2.0 ** -700):
                assert fv.weight_bits(float(v)) == b and fv.tame(float(v))
    assert fv.weight_bits(0.0) == 0 and fv.weight_bits(-0.0) == 0 and fv.tame(0.0) and fv.tame(-0.0)
    assert [fv.weight_bits(x) for x in (1.0, 0.5, 3.0, 0.75, 5.0, 0.1)] == [1, 1, 2, 2, 3, 52]


def test_what_is_not_tame():
    for w in (2.0 ** 900, 2.0 ** -900, -(2.0 ** 900), math.inf, -math.inf, math.nan, 5e-324, 2.0 ** -1030, 2.0 ** 800):
        assert not fv.tame(w), w
    for w in (2.0 ** 799, 2.0 ** -801, 1.0, -3.5, 2.0 ** 799 * 1.5):
        assert fv.tame(w), w
    assert fv.weight_bits(fv.BIG) == 1 and fv.weight_bits(fv.SMALL) == 1      # the bound alone would fuse them


@pytest.mark.parametrize("code", fv.FUSABLE)
def test_untame_case_overflows_separately_and_not_fused(code):
    sizes = [PROOF, 7]
    case = fv.untame_case(code, sizes)
    ws = case.weights[:, 0]
    assert [fv.tame(w) for w in ws] == [True, False, False, True, False, True]
    assert SIG[code] + max(fv.weight_bits(w) for w in ws) == 53 and not fv.fusable(case)
    ref = case.reference()
    if code in fv.OVERFLOWS:
        (t, at, value), = case.expect
        assert np.array_equal(np.flatnonzero(~np.isfinite(ref[0])), at) and (ref[0][at] == value).all()
        for e in at:
            assert fv.exact_fused_overflow_free(case.clients[1][0][e], case.clients[4][0][e], fv.BIG)
    else:
        assert not case.expect
    assert all(np.isfinite(r).all() for r in ref[1:]) and case.verdict() is None


def test_nnadq_values_have_full_significands():
    sizes = [300, 7]
    for codec, sig in (("float32", 24), ("float64", 53)):
        recs, dense = fv.nnadq_rows(codec, sizes)
        for rrow, drow in zip(recs, dense):
            for rec, x, s in zip(rrow, drow, sizes):
                lo, step, levels, codes = nnadq_oracle.parse(rec, s)
                assert levels == 255 and codes.min() == 0 and codes.max() == 255
                assert x.dtype == (np.float32 if sig == 24 else np.float64)
                assert all(fv.weight_bits(float(v)) == sig for v in x)
    # 29-bit weights may fuse with 24-bit values, 30-bit ones may not; fp64 values never
    assert 24 + 29 <= 53 < 24 + 30


# ---- 4. the start value ----------------------------------------------------------------------------
def zero_layout(code):
    sizes = fv.zero_sizes(code)
    return sizes, fv.zero_spots(code, sizes)


@pytest.mark.parametrize("kind", ["int", "frac"])
@pytest.mark.parametrize("code", list(fv.DTYPES))
def test_a_plus_zero_start_misses_exactly_the_planted_elements(code, kind):
    sizes, spots = zero_layout(code)
    g = fv.geometry(code)
    assert spots[0][1] < g["wide"] <= spots[0][2] < g["wide"] + 2 * g["lv"] <= spots[0][3] < spots[0][4] == sizes[0] - 1
    for which in fv.ZERO_CASES:
        case = fv.zero_case(which, code, kind, sizes, spots)
        for base in (None, fv.delta_base(sizes, 77, list(enumerate(spots)))):
            ref, wrong = case.reference(base), fv.plus_zero_chain(case, base)
            planted = {t: idx for t, idx in case.planted}
            for t in range(len(sizes)):
                want = planted.get(t, np.array([], dtype=np.int64))
                assert np.array_equal(pref.differing(wrong[t], ref[t]), want), (which, t, base is not None)
            for t, idx, value in case.expect:       # the sign of every zero, spelled out
                assert np.array_equal(pref.bits64(ref[t][idx]), pref.bits64(np.full(len(idx), value))), (which, t)
            assert case.verdict(base) is None
        assert (which in ("minus_then_plus", "plus_then_minus", "cancel")) == (not case.planted)


@pytest.mark.parametrize("code", list(fv.DTYPES))
def test_nonfinite_cases_have_the_verdict_they_are_named_for(code):
    sizes, spots = zero_layout(code)
    want = {"inf_times_zero": "accumulator", "inf_minus_inf": "accumulator", "nan_first": "input", "nan_last": "input",
            "zero_total": "result"}
    for which in fv.NONFINITE_CASES:
        case = fv.nonfinite_case(which, code, sizes, spots)
        stage, bad = case.verdict()
        assert stage == want[which], which
        n = len(case.clients)
        assert bad == {"nan_first": [0], "nan_last": [n - 1]}.get(which, [])
        ref = case.reference()
        if which.startswith("inf_") or which == "zero_total":
            for t in range(len(sizes)):
                assert np.array_equal(np.flatnonzero(np.isnan(ref[t])), spots[t]), (which, t)
        if which.startswith("nan_"):
            assert n == fv.geometry(code)["group"] + 1
            assert np.flatnonzero(np.isnan(ref[0])).tolist() == [spots[0][1]] and not np.isnan(ref[1]).any()
        if which == "zero_total":
            assert case.totals() == [0.0, 0.0]
    assert fv.zero_weights_case(code, sizes).verdict() == ("result", [])


# ---- the patterns, the guarded buffer, the slots ---------------------------------------------------
def test_pattern_tensors_cover_what_they_claim():
    for code in ("f16", "bf16", "f32"):
        case, t = fv.pattern_case(code, "one")
        x = case.clients[1][0]
        wide = fv.geometry(code)["wide"]
        assert x.size > wide and x.size % wide == 5 and not np.isnan(x).any()
        assert int(fv.is_subnormal(x, code).sum()) >= fv.MIN_SUBNORMALS
        assert np.isinf(x).any() or code == "f32"
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        if code == "f32":
            fmax = float(np.finfo(np.float32).max)
            assert {fmax, -fmax, 2.0 ** -149, -(2.0 ** -149)} <= set(x[:6].tolist())
        else:
            # every non-NaN pattern once (1.5, which stands in for the NaNs, is one of them)
            assert len(set(bits(t[:65536]).tolist())) == 65536 - {"f16": 2046, "bf16": 254}[code]
        assert fv.fusable(case) and not fv.fusable(fv.pattern_case(code, "w53")[0])
        ref = case.reference()[0]                       # weights 1, 1, 2 around the identity: x / 4, exact
        assert np.array_equal(pref.bits64(ref), pref.bits64(x / 4.0))


def test_guarded_outputs_have_sentinels_on_both_sides_of_every_view():
    import torch

    for dtype in (torch.float32, torch.float64):
        for mis in (None, 0, 2):
            g = fv.Guarded([5, 1, 8, 3], dtype, "cpu", mis)
            per16 = 16 // dtype.itemsize
            for i, (o, v) in enumerate(zip(g.offsets, g.views)):
                assert not g.mask[o - per16 + (1 if i == mis else 0):o].any() and not g.mask[o + v.numel()]
            assert not g.mask[-per16:].any() and g.gaps_untouched()
            g.views[2].fill_(1.0)
            assert g.gaps_untouched()
            g.buf[g.offsets[2] - 1] = 0.0
            assert not g.gaps_untouched()


def test_the_seven_calls_cross_the_first_slot_capacity_and_regrow_twice():
    needs = [fv.blob_bytes(fv.SLOT_T, k) for k in fv.SLOT_CLIENTS]
    assert len(needs) == 7 > fv.SLOTS and len(fv.slot_sizes()) == fv.SLOT_T
    assert max(needs[:fv.SLOTS]) <= fv.FIRST_SLOT < min(needs[fv.SLOTS:])
    assert fv.slot_regrows(needs) == [4, 5, 6]
    # BlobLayout by hand for T = 2, K = 3: 48 + 48 pointers and weights, 16 + 16 + 16 + 16 + 16, to 256
    assert fv.blob_bytes(2, 3) == 256 and fv.blob_bytes(2, 0) == fv.blob_bytes(2, 1)
    assert fv.blob_bytes(64, 70) == 2 * 8 * 64 * 70 + 256 + 256 + 3 * 512
