"""The inputs of the personalized kernel's contract suite discriminate — shown with the restatement
alone (tests/pers_reference.py), never with the code under test. No GPU.

* The restatement equals ``oracle.personalized_oracle`` (itself pinned to the reference's own
  outputs) bit for bit.
* **The fold bound.** ``fedavg_pers_aggregate`` fuses the fold when every folded product is exact:
  ``sig(dtype) + bits(weight) <= 53``, i.e. weights of at most b* = 29 (fp32), 42 (fp16), 45 (bf16)
  bits. On ``pers_values.fold_case`` an exact fused chain equals the separately rounded chain in
  every element at b*, and differs from it in at least ``BAR`` = 10 % of the elements of a receiver
  whose weights are b* + 1 bits wide: a condition on the inputs, not a measurement. A kernel that
  fused one bit too early would therefore fail tests/test_gpu_pers_contract.py in a tenth of that
  receiver's elements.
* **The refold.** The kernel's main loop restated without its refold differs from the reference at
  exactly the planted elements of every refold case, and nowhere else: each planted element needs
  the refold, and nothing else does.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle.fedavg_oracle import OracleMessage
from oracle.personalized_oracle import OraclePersonalizedFedAvg
from tests import pers_reference as pref
from tests import pers_values as pv

BAR = 0.10
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
GEO = pv.DEFAULT
REFOLD_SIZES = [3, GEO["chunk"], GEO["chunk"] + 1]


# ---- the generators ------------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(pv.SIG))
def test_full_values_are_exact_in_their_format_with_the_low_bit_set(code):
    v = pv.full_values(np.random.default_rng(1), 4096, code)
    t = torch.from_numpy(v)
    assert bool((t.to(TORCH[code]).to(torch.float64) == t).all())
    m, e = np.frexp(np.abs(v))                                 # m in [0.5, 1)
    ints = m * 2.0 ** pv.SIG[code]
    assert (ints == np.floor(ints)).all() and (ints % 2 == 1).all() and (ints >= 2.0 ** (pv.SIG[code] - 1)).all()
    assert (v < 0).any() and (v > 0).any() and e.min() == -3 + 1 and e.max() == 3 + 1


@pytest.mark.parametrize("b", [1, 2, 29, 30, 42, 43, 45, 46, 53])
def test_odd_weights_have_exactly_b_bits(b):
    w = pv.odd_weights(np.random.default_rng(b), 500, b)
    assert (w % 2 == 1).all() and (w >= 2.0 ** (b - 1)).all() and (w < 2.0 ** b).all()
    assert (w == np.floor(w)).all()


def test_fold_bounds():
    assert pv.FOLD_BOUND == {"f32": 29, "f16": 42, "bf16": 45}


# ---- the restatement against the pinned oracle -----------------------------------------------------
def oracle_of(case: pv.Case):
    o = OraclePersonalizedFedAvg()
    ww = {rid: {cid: float(case.weights[j, k]) for k, cid in enumerate(case.client_ids) if case.weights[j, k] != 0}
          for j, rid in enumerate(case.receiver_ids)}
    o.set_worker_weights(ww)                     # an omitted weight is ``.get(i, 0)``: a real zero
    for k, cid in enumerate(case.client_ids):
        o.process_worker_data(cid, OracleMessage(parameter={f"t{t}": x.astype(np.float32)
                                                            for t, x in enumerate(case.clients[k]) if x is not None}))
    return o.aggregate_worker_data()


@pytest.mark.parametrize("which", ["dense", "sparse", "missing"])
def test_restatement_equals_the_oracle(which):
    case = pv.table_case("f32", "frac", 7, 9, [5, 33], seed=60, absent=which == "missing")
    if which == "sparse":
        rng = np.random.default_rng(61)
        case.weights[rng.random(case.weights.shape) < 0.4] = 0.0
        case.weights[:, 3:5] = [1.5, 0.75]       # nobody's total is zero: every row folds client 3 or 4
        assert (case.weights == 0).any()
    got, want = case.reference(), oracle_of(case)
    assert got.flags == 0
    for j, rid in enumerate(case.receiver_ids):
        for t in range(2):
            assert np.array_equal(pref.bits64(got.outs[j][t]), pref.bits64(want.worker_data[rid].parameter[f"t{t}"])), (j, t)
    for t in range(2):
        assert np.array_equal(pref.bits64(got.central[t]), pref.bits64(want.centralized_parameter[f"t{t}"])), t


# ---- the fold bound --------------------------------------------------------------------------------
def chains_of(case: pv.Case, row: int):
    ks = pref.folded(case.clients, case.client_ids, case.receiver_ids[row], 0)
    xs, ws = [case.clients[k][0] for k in ks], [case.weights[row, k] for k in ks]
    return pref.separate_chain(xs, ws), pref.fused_chain(xs, ws)


@pytest.mark.parametrize("code", list(pv.FOLD_BOUND))
def test_at_the_bound_the_fused_chain_is_the_separate_chain(code):
    case = pv.fold_case(code, GEO["chunk"], 4, None)
    for row in range(4):
        sep, fused = chains_of(case, row)
        assert np.array_equal(pref.bits64(sep), pref.bits64(fused)), (code, row)
    case = pv.own_wide_case(code, GEO["chunk"])
    for row in range(4):
        sep, fused = chains_of(case, row)                      # the 53-bit weights are on no folded pair
        assert np.array_equal(pref.bits64(sep), pref.bits64(fused)), (code, row)


@pytest.mark.parametrize("wide_row", [0, GEO["jb"], GEO["group"]])
@pytest.mark.parametrize("code", list(pv.FOLD_BOUND))
def test_one_bit_past_the_bound_the_chains_differ_in_a_tenth(code, wide_row):
    case = pv.fold_case(code, GEO["chunk"], GEO["group"] + 1, wide_row)
    b = pv.FOLD_BOUND[code]
    assert (case.weights[wide_row] >= 2.0 ** b).all() and (np.delete(case.weights, wide_row, 0) < 2.0 ** b).all()
    sep, fused = chains_of(case, wide_row)
    frac = float((pref.bits64(sep) != pref.bits64(fused)).mean())
    print(f"{code}, wide row {wide_row}: fused differs from separate in {frac:.3f}")
    assert frac >= BAR, (code, wide_row, frac)
    other = (wide_row + 1) % (GEO["group"] + 1)                # a receiver at b* beside it stays exact
    sep, fused = chains_of(case, other)
    assert np.array_equal(pref.bits64(sep), pref.bits64(fused))


@pytest.mark.parametrize("code", list(pv.FOLD_BOUND))
def test_untame_weights_keep_the_reference_finite(code):
    case = pv.untame_case(code, GEO["chunk"])
    assert set(np.unique(case.weights)) == {2.0 ** -900, 2.0 ** 900}
    ref = case.reference()
    assert ref.flags == 0 and all(np.isfinite(o[0]).all() and (o[0] != 0).all() for o in ref.outs)


# ---- the refold ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "frac"])
@pytest.mark.parametrize("code", list(pv.SIG))
def test_main_loop_without_the_refold_misses_exactly_the_planted_elements(code, kind):
    pad = max(GEO["u"], GEO["stage"])
    for case in pv.refold_cases(code, kind, REFOLD_SIZES, GEO["jb"], GEO["group"]):
        ref = case.reference()
        model = pv.main_loop_without_refold(case, pad)
        planted = {(j, t): set(int(i) for i in idx) for j, t, idx in case.planted}
        for j in range(len(case.receiver_ids)):
            for t in range(len(REFOLD_SIZES)):
                got = set(pref.differing(model[j][t], ref.outs[j][t]).tolist())
                assert got == planted.get((j, t), set()), (code, kind, case.name, j, t, sorted(got))
        for j, t, idx, value in case.expect:
            want = np.full(len(idx), value)
            assert np.array_equal(pref.bits64(ref.outs[j][t][idx]), pref.bits64(want)), (case.name, j, t)
        for j in case.finite_rows:
            assert all(np.isfinite(o).all() for o in ref.outs[j]), (case.name, j)
        if "own_poison_among_many" in case.name:   # the other receivers fold the poisoned client
            assert ref.flags == pref.FLAG_ACC_NAN | pref.FLAG_RESULT_NAN | pref.FLAG_CENTRAL_NAN
        else:
            assert ref.flags == 0, case.name
    few, many = (pv.refold_cases(code, kind, REFOLD_SIZES, GEO["jb"], GEO["group"], part) for part in ("few", "many"))
    assert len(few) == 5 and len(many) == 5 and sum(bool(c.planted) for c in few + many) == 9   # all but (iv)


# ---- the ring and the blob -------------------------------------------------------------------------
def test_ring_pairs_cover_every_count_with_one_and_two_waves():
    jb, stage, depth = GEO["jb"], GEO["stage"], GEO["depth"]
    pairs = pv.ring_pairs(jb, stage, depth)
    waves = lambda m: (m + jb - 1) // jb                      # noqa: E731
    for n in pv.ring_client_counts(stage, depth):
        assert {1, 2} <= {waves(m) for c, m in pairs if c == n}
    for m in pv.ring_receivers(jb):
        assert any(r == m for _, r in pairs)
    assert sorted({waves(m) for m in pv.ring_receivers(jb)}) == [1, 2, 3, 4]
    pad = max(GEO["u"], stage)
    stages = sorted({(n + pad - 1) // pad * pad // stage for n in pv.ring_client_counts(stage, depth)})
    assert stages == [1, 2, depth, depth + 1, depth + 2, depth + 3]
    for n, m in pairs:                                         # every receiver has somebody to fold
        pv.table_case("f32", "int", n, m, [2, 3], seed=1).reference()


def test_blob_bytes_by_hand():
    # 4 clients, 3 receivers, 2 segments: 256 (pointers) + 4096 (weights) + 256 (masks) + 3 * 2048
    # (totals, outputs, reciprocals) + 256 (centralized pointers) + 2048 (zero block)
    assert pv.blob_bytes(4, 3, 2) == 256 + 4096 + 256 + 3 * 2048 + 256 + 2048
    assert pv.blob_bytes(40, 129, 2) == 768 + 2 * (40960 + 1280 + 3 * 2048) + 256 + 2048
