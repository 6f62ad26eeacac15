"""The dense fold (csrc/fedavg_kernels.hip: ``fedavg_tile_kernel`` / ``tile_body``) and its host half
(``note_weight``, ``fma_exact_call``, ``build_blob``, ``stage_tables``) against DESIGN.md §6: the fold
that the host's proof allows on both sides of its bound, the ``-0.0`` identity and signed zeros, absent
tensors, every bit pattern of the 16-bit input formats and fp32 subnormals, that nothing but the output
elements is written, and the table slots with launches in flight. Every comparison is bit for bit with
``oracle.fedavg_oracle.fedavg_flat`` (a delta call: ``base + x`` in fp64 first); no tolerance anywhere.
A NaN compares as a NaN: the same NaN mask and identical bits elsewhere, and ``raise_on_nan`` must
report exactly the stage that the reference's verdict implies.

The cases are ``tests/fold_values``'; tests/test_fold_values_host.py shows on the CPU that an exactly
fused chain differs from the reference in at least a tenth of the elements when every weight is one
bit past the bound, in at least 16 of 512 with one such weight, and that a chain started from +0.0
misses exactly the planted elements of every signed-zero case.

The kernel is driven through ``FedAvgContext``. Sizes come from the build's own geometry
(``fedavg_kernel_constant``). No input asks the kernel to read or write past a tensor: every pointer
is a whole torch tensor or a view that ends inside its buffer.

Out of scope: the split-client kernel (opt-in, toleranced), the dynamic-wave kernel (always the
separately rounded fold), the per-element-weight kernels, QSGD (its table products are separately
rounded), and the multi-device and windowed paths.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import NaNAggregationError
from distributed_learning_simulation_lib_amd.fedavg import ClientTable, FedAvgContext, ModelLayout
from distributed_learning_simulation_lib_amd.quantized import NNADQ_F32, NNADQ_F64, QuantizedTensor
from oracle.fedavg_oracle import fedavg_flat
from tests import fold_values as fv
from tests.pers_values import full_values, odd_weights
from tests.robust_values import DTYPES, SENTINEL, Outs, assert_same_bits, bits, place

pytestmark = pytest.mark.gpu

NP_OUT = {"f64": np.float64, "f32": np.float32}


def layout_of(sizes) -> ModelLayout:
    return ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))), shapes=tuple((s,) for s in sizes))


def make_ctx(sizes, device, balance: str, monkeypatch) -> FedAvgContext:
    """``always``: the balanced whole-layout tile orders for every layout (read when the context is made)."""
    if balance == "always":
        monkeypatch.setenv("FEDAVG_BALANCE_ALWAYS", "1")
    else:
        monkeypatch.delenv("FEDAVG_BALANCE_ALWAYS", raising=False)
    return FedAvgContext(layout_of(sizes), device)


def same(got, want, what: str) -> None:
    """The same NaN mask, and the same bits wherever there is no NaN."""
    g, w = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(g), np.isnan(w)
    assert np.array_equal(gn, wn), f"{what}: NaN at {np.flatnonzero(gn).tolist()[:8]}, want {np.flatnonzero(wn).tolist()[:8]}"
    assert_same_bits(np.where(gn, 0, g), np.where(wn, 0, w), what)


def narrow(x: np.ndarray, code: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).to(DTYPES[code])


def device_rows(case: fv.Case, device, misalign: bool = False) -> list:
    return [[None if x is None else place(narrow(x, case.code), device, misalign) for x in row] for row in case.clients]


def device_base(base, device, misalign: bool = False) -> list:
    return [place(torch.from_numpy(b), device, misalign) for b in base]


def table_of(rows, weights, T: int) -> ClientTable:
    t = ClientTable(T)
    for row, w in zip(rows, weights):
        t.add_client(row, [float(v) for v in w])
    return t


def fold(ctx, tabs, dt, outs, out_dtype, base=None) -> None:
    """Every table but the last is a wave into the accumulator; the last one ends the round."""
    for t in tabs[:-1]:
        if base is None:
            ctx.accumulate(t, dt)
        else:
            ctx.accumulate_delta(t, dt, base)
    if base is None:
        ctx.aggregate(tabs[-1], dt, outs, out_dtype)
    else:
        ctx.aggregate_delta(tabs[-1], dt, base, outs, out_dtype)


def expect_verdict(ctx, tabs, dt, verdict) -> None:
    pairs = [(t, dt) for t in tabs]
    if verdict is None:
        ctx.raise_on_nan(pairs)
        return
    with pytest.raises(NaNAggregationError) as ei:
        ctx.raise_on_nan(pairs)
    assert (ei.value.stage, list(ei.value.bad_clients)) == (verdict[0], list(verdict[1]))


def run(ctx, case: fv.Case, dev, device, ref, *, waves=None, out: str = "f64", base=None, verdict=None,
        entry: str = "fold", what: str = ""):
    """One round of a case through one entry point, checked against ``ref``: the outputs (inside
    sentinel guards), and what ``raise_on_nan`` reports. Returns the outputs."""
    T, dt, od = len(case.sizes), DTYPES[case.code], DTYPES[out]
    tabs = [table_of(dev[a:b], case.weights[a:b], T) for a, b in (waves or [(0, len(dev))])]
    outs = Outs(case.sizes, od, device, False)
    what = f"{what} {case.name} {entry} waves={waves} out={out} delta={base is not None}"
    if entry == "fold":
        fold(ctx, tabs, dt, outs.views, od, base)
    elif entry == "plan":                      # the prepared call, twice
        plan = ctx.plan(tabs[0], dt, outs.views, od)
        plan.run()
        ctx.raise_on_nan()
        first = outs.numpy()
        for v in outs.views:
            v.fill_(SENTINEL)
        plan.run()
        for t, (a, w) in enumerate(zip(first, ref)):
            same(a, w.astype(NP_OUT[out]), f"{what}: first run, segment {t}")
        plan.close()
    elif entry == "partial":                   # two tile ranges into the accumulator, then the division
        nt = ctx.num_tiles
        assert nt >= 2
        ctx.partial(tabs[0], dt, True, 0, nt // 2)
        ctx.partial(tabs[0], dt, True, nt // 2, nt)
        ctx.set_accumulated(case.totals())
        ctx.finalize_range(outs.views, od)
    else:
        raise ValueError(entry)
    expect_verdict(ctx, tabs, dt, verdict)
    assert outs.guards_untouched(), what
    got = outs.numpy()
    with np.errstate(all="ignore"):
        for t, (a, w) in enumerate(zip(got, ref)):
            same(a, w.astype(NP_OUT[out]), f"{what}: segment {t}")
    ctx.reset()
    return got


# ---- B. the fused-fold bound -----------------------------------------------------------------------
@pytest.mark.parametrize("balance", ["auto", "always"])
@pytest.mark.parametrize("where", ["at", "past"])
@pytest.mark.parametrize("code", fv.FUSABLE)
def test_all_weights_at_and_past_the_bound(hip_device, code, where, balance, monkeypatch):
    """Six clients, every weight ``53 - sig`` bits wide (the host may fuse) or one bit wider (it must
    not: a fused fold differs in at least a tenth of the elements) — positive, negative and scaled by
    2^40 and 2^-40; through the vector path and through misaligned clients (the scalar path); with the
    fused fold allowed and forbidden; fp64 and fp32 outputs."""
    sizes = fv.bound_sizes(code)
    ctx = make_ctx(sizes, hip_device, balance, monkeypatch)
    try:
        for variant in fv.VARIANTS:
            case = fv.bound_case(code, where, variant, sizes)
            assert fv.fusable(case) == (where == "at")
            ref = case.reference()
            for misalign in (False, True):
                dev = device_rows(case, hip_device, misalign)
                for fused in (True, False):
                    ctx.set_fused_fold(fused)
                    run(ctx, case, dev, hip_device, ref, out="f32" if fused == misalign else "f64",
                        what=f"fused={fused} misalign={misalign}")
    finally:
        ctx.close()


@pytest.mark.parametrize("place_", fv.LONE_PLACES)
@pytest.mark.parametrize("code", fv.FUSABLE)
def test_one_wide_weight_in_one_entry_forbids_the_fused_fold(hip_device, code, place_):
    """One (client, tensor) entry one bit past the bound among entries at it — a middle client of the
    first tensor, the last client of the last tensor, and right behind a repeated weight (the repeat
    cache of ``note_weight`` must not hide it): the whole call folds separately."""
    sizes = fv.bound_sizes(code)
    case = fv.lone_wide_case(code, place_, sizes)
    assert not fv.fusable(case)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        dev, ref = device_rows(case, hip_device), case.reference()
        run(ctx, case, dev, hip_device, ref)
        ctx.set_fused_fold(False)
        run(ctx, case, dev, hip_device, ref, out="f32", what="fused=False")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["pow2", "two_bit"])
def test_fp64_inputs_are_never_fused(hip_device, kind):
    sizes = fv.bound_sizes("f64")
    case = fv.f64_case(kind, sizes)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        ref = case.reference()
        for misalign in (False, True):
            dev = device_rows(case, hip_device, misalign)
            for fused in (True, False):
                ctx.set_fused_fold(fused)
                run(ctx, case, dev, hip_device, ref, out="f32" if fused else "f64", what=f"fused={fused}")
    finally:
        ctx.close()


@pytest.mark.parametrize("code", list(DTYPES))
def test_all_zero_weights(hip_device, code):
    """x * 0 = ±0 throughout and a total of 0: every element is 0 / 0, and the stage is the result's."""
    sizes = fv.bound_sizes(code)
    case = fv.zero_weights_case(code, sizes)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        ref, dev = case.reference(), device_rows(case, hip_device)
        assert all(np.isnan(r).all() for r in ref)
        for fused in (True, False):
            ctx.set_fused_fold(fused)
            run(ctx, case, dev, hip_device, ref, verdict=("result", []), what=f"fused={fused}")
    finally:
        ctx.close()


@pytest.mark.parametrize("code", fv.FUSABLE)
def test_untame_weights_forbid_the_fused_fold(hip_device, code):
    """2^900 and 2^-900 have 1-bit significands, but a product with them can leave the fp64 range:
    ``weights_tame`` is false. fp32 and bf16: x * 2^900 overflows where the fused sum would not."""
    sizes = fv.bound_sizes(code)
    case = fv.untame_case(code, sizes)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        ref = case.reference()
        for misalign in (False, True):
            got = run(ctx, case, device_rows(case, hip_device, misalign), hip_device, ref, what=f"misalign={misalign}")
            for t, idx, value in case.expect:
                assert (got[t][idx] == value).all()
    finally:
        ctx.close()


def _joined(first: fv.Case, second: fv.Case) -> fv.Case:
    return fv.Case(f"{first.name} + {second.name}", first.code, first.clients + second.clients,
                   np.concatenate([first.weights, second.weights]))


ENTRIES = ("at_then_past", "past_then_at", "plan", "partial", "delta")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("code", fv.FUSABLE)
def test_the_bound_at_every_entry_point(hip_device, code, entry):
    """The fold is chosen per call: a wave at the bound and a wave past it, in both orders; a plan run
    twice; two ranged partials and a ranged finalize; and delta calls with weights at the bound, which
    are never fused (``base + x`` has 53 bits)."""
    sizes = fv.bound_sizes(code)
    at, past = fv.bound_case(code, "at", "pos", sizes), fv.bound_case(code, "past", "up", sizes)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        for fused in (True, False):
            ctx.set_fused_fold(fused)
            out = "f64" if fused else "f32"
            if entry in ("at_then_past", "past_then_at"):
                case = _joined(at, past) if entry == "at_then_past" else _joined(past, at)
                run(ctx, case, device_rows(case, hip_device), hip_device, case.reference(),
                    waves=[(0, fv.CLIENTS), (fv.CLIENTS, 2 * fv.CLIENTS)], out=out, what=f"fused={fused}")
            elif entry in ("plan", "partial"):
                for case in (at, past):
                    run(ctx, case, device_rows(case, hip_device), hip_device, case.reference(), entry=entry, out=out,
                        what=f"fused={fused}")
            else:
                base = fv.delta_base(sizes, 31)
                bdev, dev, ref = device_base(base, hip_device), device_rows(at, hip_device), at.reference(base)
                for waves in (None, [(0, 3), (3, fv.CLIENTS)]):
                    run(ctx, at, dev, hip_device, ref, waves=waves, base=bdev, out=out, what=f"fused={fused}")
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["f32_29", "f32_30", "f64_int"])
def test_nnadq_records_at_and_past_the_bound(hip_device, which):
    """``FEDAVG_NNADQ_F32`` counts as 24 bits: 29-bit weights may fuse, 30-bit ones may not; the fp64
    codec's values have 53 bits and never fuse, with small integer weights too."""
    codec, fmt = ("float64", NNADQ_F64) if which == "f64_int" else ("float32", NNADQ_F32)
    sizes = [fv.K("nnadq_tile") + 5, 7]
    recs, dense = fv.nnadq_rows(codec, sizes)
    rng = np.random.default_rng(61)
    weights = [float(w) for w in (rng.integers(1, 250, fv.CLIENTS) * 2 + 1 if which == "f64_int"
                                  else odd_weights(rng, fv.CLIENTS, 29 if which == "f32_29" else 30))]
    with np.errstate(all="ignore"):
        ref = [fedavg_flat([dense[k][t] for k in range(fv.CLIENTS)], weights) for t in range(len(sizes))]
    table = ClientTable(len(sizes))
    for k, row in enumerate(recs):
        qts = [QuantizedTensor(torch.from_numpy(r).to(hip_device), (n,), fmt) for r, n in zip(row, sizes)]
        table.add_client([q.record for q in qts], [weights[k]] * len(sizes))
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        for fused in (True, False):
            ctx.set_fused_fold(fused)
            for out in ("f64", "f32"):
                outs = Outs(sizes, DTYPES[out], hip_device, False)
                ctx.aggregate(table, fmt, outs.views, DTYPES[out])
                ctx.raise_on_nan([(table, fmt)])
                assert outs.guards_untouched()
                for t, (a, w) in enumerate(zip(outs.numpy(), ref)):
                    same(a, w.astype(NP_OUT[out]), f"{which} fused={fused} out={out}: segment {t}")
    finally:
        ctx.close()


# ---- C. signed zeros, the identity, absent tensors -------------------------------------------------
@pytest.mark.parametrize("balance", ["auto", "always"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_signed_zeros_and_absent_tensors(hip_device, code, balance, monkeypatch):
    """The cases of ``fold_values.ZERO_CASES`` — every product -0.0 (from negative zeros, from negative
    weights on positive zeros, from a -0.0 weight), -0.0 then +0.0 and the reverse, x * w + (-x) * w, a
    tensor absent from the first, a middle or the last wave only, a tensor of one client alone — planted
    inside a full tile, inside whole lane vectors, in the ragged tail and at both ends; in one launch
    and in three waves (the clients that matter then sit in different waves); integer weights with the
    fused fold allowed and forbidden, fractional weights; plain and delta calls."""
    sizes = fv.zero_sizes(code)
    spots = fv.zero_spots(code, sizes)
    base = fv.delta_base(sizes, 77, list(enumerate(spots)))
    ctx = make_ctx(sizes, hip_device, balance, monkeypatch)
    try:
        bdev = device_base(base, hip_device)
        for which in fv.ZERO_CASES:
            for kind, settings in (("int", (True, False)), ("frac", (True,))):
                case = fv.zero_case(which, code, kind, sizes, spots)
                dev, ref, dref = device_rows(case, hip_device), case.reference(), case.reference(base)
                for fused in settings:
                    ctx.set_fused_fold(fused)
                    for waves, out in ((None, "f64"), (fv.WAVES3, "f32")):
                        for b, r in ((None, ref), (bdev, dref)):
                            got = run(ctx, case, dev, hip_device, r, waves=waves, out=out, base=b, what=f"fused={fused}")
                            for t, idx, value in case.expect:     # the sign of a zero, spelled out
                                assert_same_bits(got[t][idx], np.full(len(idx), value, dtype=NP_OUT[out]),
                                                 f"{case.name}: segment {t}")
    finally:
        ctx.close()


@pytest.mark.parametrize("code", list(DTYPES))
def test_inf_and_nan_name_the_stage(hip_device, code):
    """inf * 0 and inf - inf across two waves (the accumulator), a NaN in the first and in the last
    client of ``group + 1`` (the input, with its table row), a total weight of 0 (the result): the NaN
    mask, the bits elsewhere, and the stage that ``raise_on_nan`` names."""
    sizes = fv.zero_sizes(code)
    spots = fv.zero_spots(code, sizes)
    base = fv.delta_base(sizes, 78, list(enumerate(spots)))
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        bdev = device_base(base, hip_device)
        for which in fv.NONFINITE_CASES:
            case = fv.nonfinite_case(which, code, sizes, spots)
            dev = device_rows(case, hip_device)
            for fused, out in ((True, "f64"), (False, "f32")):
                ctx.set_fused_fold(fused)
                run(ctx, case, dev, hip_device, case.reference(), waves=case.waves, out=out, verdict=case.verdict(),
                    what=f"fused={fused}")
            run(ctx, case, dev, hip_device, case.reference(base), waves=case.waves, base=bdev, verdict=case.verdict(base))
    finally:
        ctx.close()


# ---- D. every bit pattern --------------------------------------------------------------------------
@pytest.mark.parametrize("weight", fv.PATTERN_WEIGHTS)
@pytest.mark.parametrize("code", ["f16", "bf16", "f32"])
def test_every_pattern_widens_exactly(hip_device, code, weight):
    """All 65536 fp16 / bf16 patterns (fp32: random patterns with subnormals, both zeros and the largest
    finite values) as the middle client of three, the others the identity: with weight 1 (fused) the
    fp64 result is the pattern / 4 exactly; with a 53-bit weight the separately rounded fold. Through
    the vector loader, through misaligned storage (the scalar loader) and as a delta."""
    case, t = fv.pattern_case(code, weight)
    size = t.numel()
    assert int(fv.is_subnormal(case.clients[1][0], code).sum()) >= fv.MIN_SUBNORMALS
    ctx = FedAvgContext(layout_of([size]), hip_device)
    try:
        ident = narrow(case.clients[0][0], code)
        for way in ("vector", "scalar", "delta"):
            mis = way == "scalar"
            dev = [[place(ident, hip_device, mis)], [place(t, hip_device, mis)], [place(ident, hip_device, mis)]]
            assert np.array_equal(bits(dev[1][0]), bits(t))
            base = fv.pattern_base(size, 91) if way == "delta" else None
            run(ctx, case, dev, hip_device, case.reference(base), base=None if base is None else device_base(base, hip_device),
                what=way)
    finally:
        ctx.close()


# ---- E. nothing else is written --------------------------------------------------------------------
@pytest.mark.parametrize("balance", ["auto", "always"])
@pytest.mark.parametrize("code", list(DTYPES))
def test_nothing_but_the_outputs_is_written(hip_device, code, balance, monkeypatch):
    """Outputs are slices of one sentinel-filled buffer, over the lengths of the geometry suite: with
    every pointer 16-byte aligned, with one output, one client tensor or (a delta call) the base alone
    misaligned — ``st.aligned`` without ``st.clients_aligned`` and with it. The gaps keep the sentinel,
    the clients and the base keep their bits, and the results are the reference's."""
    from tests.test_gpu_geometry import fedavg_lengths

    lengths = fedavg_lengths(code)
    at = len(lengths) - 2                         # a segment of more than one wide tile
    rng = np.random.default_rng(fv.seed_of("guards", code))
    n = 3
    case = fv.Case(f"guards {code}", code, [[full_values(rng, s, code) for s in lengths] for _ in range(n)],
                   np.repeat(np.array([[3.0], [0.37], [1234.0]]), len(lengths), axis=1))
    base = fv.delta_base(lengths, 79)
    ref = {False: case.reference(), True: case.reference(base)}
    ctx = make_ctx(lengths, hip_device, balance, monkeypatch)
    try:
        dev = device_rows(case, hip_device)
        dev_mis = [list(row) for row in dev]
        dev_mis[1][at] = place(narrow(case.clients[1][at], code), hip_device, True)
        bdev = device_base(base, hip_device)
        bdev_mis = list(bdev)
        bdev_mis[at] = place(torch.from_numpy(base[at]), hip_device, True)
        want_bits = [[bits(narrow(x, code)) for x in row] for row in case.clients]
        dt = DTYPES[code]
        for variant in ("aligned", "out", "client", "base"):
            for out in ("f64", "f32"):
                for delta in (False, True):
                    if variant == "base" and not delta:
                        continue
                    rows = dev_mis if variant == "client" else dev
                    b = None if not delta else bdev_mis if variant == "base" else bdev
                    g = fv.Guarded(lengths, DTYPES[out], hip_device, at if variant == "out" else None)
                    fold(ctx, [table_of(rows, case.weights, len(lengths))], dt, g.views, DTYPES[out], b)
                    ctx.raise_on_nan()
                    what = f"{variant} out={out} delta={delta}"
                    assert g.gaps_untouched(), what
                    for k, row in enumerate(rows):
                        for t, x in enumerate(row):
                            assert np.array_equal(bits(x), want_bits[k][t]), f"{what}: client {k}, tensor {t} changed"
                    for t, x in enumerate(b or []):
                        assert np.array_equal(bits(x), bits(base[t])), f"{what}: the base changed, tensor {t}"
                    for t, (a, w) in enumerate(zip(g.numpy(), ref[delta])):
                        same(a, w.astype(NP_OUT[out]), f"{what}: segment {t} ({lengths[t]})")
    finally:
        ctx.close()


# ---- F. table slots and blob reuse -----------------------------------------------------------------
def test_seven_calls_back_to_back_cross_the_slots_and_their_regrowth(hip_device):
    """Seven ``aggregate`` calls on one context and one stream with nothing between them that reads back
    or synchronises: more calls than the four table slots, and client counts that outgrow the 64 KiB
    first capacity of three slots (tests/test_fold_values_host.py). Every call has its own clients,
    weights and outputs; all are read back at the end."""
    sizes = fv.slot_sizes()
    T, total = len(sizes), sum(sizes)
    stride = (total + 3) // 4 * 4
    offsets = [int(v) for v in np.cumsum([0] + sizes[:-1])]
    needs = [fv.blob_bytes(T, n) for n in fv.SLOT_CLIENTS]
    assert len(fv.slot_regrows(needs)) >= 2
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        calls = []
        for i, n in enumerate(fv.SLOT_CLIENTS):
            rng = np.random.default_rng(800 + i)
            flat = full_values(rng, n * stride, "f32").reshape(n, stride)
            w = [float(v) for v in (rng.integers(1, 5000, n) if i % 2 else rng.uniform(0.01, 3.0, n))]
            with np.errstate(all="ignore"):
                ref = fedavg_flat([flat[k, :total] for k in range(n)], w)
            d = torch.from_numpy(flat).to(torch.float32).to(hip_device)
            table = ClientTable(T)
            for k in range(n):
                table.add_client([d[k, o:o + s] for o, s in zip(offsets, sizes)], [w[k]] * T)
            out = torch.full((stride,), SENTINEL, dtype=torch.float64, device=hip_device)
            calls.append((table, out, ref, d))
        torch.cuda.synchronize(hip_device)
        for table, out, _, _ in calls:                           # back to back
            ctx.aggregate(table, torch.float32, [out[o:o + s] for o, s in zip(offsets, sizes)], torch.float64)
        ctx.raise_on_nan()
        for i, (_, out, ref, _) in enumerate(calls):
            host = out.cpu().numpy()
            assert (host[total:] == SENTINEL).all()
            assert_same_bits(host[:total], ref, f"call {i + 1} ({fv.SLOT_CLIENTS[i]} clients)")
    finally:
        ctx.close()


def _reuse_setup(device):
    sizes = [fv.geometry("f32")["wide"] + 5, 9]
    rng = np.random.default_rng(900)
    def make():
        return fv.Case("reuse", "f32", [[full_values(rng, s, "f32") for s in sizes] for _ in range(4)],
                       np.repeat(np.array([[17.0], [0.3], [4999.0], [2.5]]), len(sizes), axis=1))
    return sizes, make(), make()


def test_an_identical_table_sees_new_client_contents_and_new_outputs(hip_device):
    """The upload is skipped when a call's table blob equals the last one byte for byte. The same table,
    weights and outputs after the client tensors were overwritten in place: the second result is that of
    the new contents. Then the same table with new outputs: they are written, and the old ones keep
    what they held."""
    sizes, old, new = _reuse_setup(hip_device)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        dev = device_rows(old, hip_device)
        table = table_of(dev, old.weights, len(sizes))
        outs = Outs(sizes, torch.float64, hip_device, False)
        ctx.aggregate(table, torch.float32, outs.views, torch.float64)
        first = [v.clone() for v in outs.views]
        for row, src in zip(dev, new.clients):
            for x, s in zip(row, src):
                x.copy_(narrow(s, "f32"))
        ctx.aggregate(table, torch.float32, outs.views, torch.float64)
        outs2 = Outs(sizes, torch.float64, hip_device, False)
        ctx.aggregate(table, torch.float32, outs2.views, torch.float64)
        ctx.raise_on_nan()
        assert outs.guards_untouched() and outs2.guards_untouched()
        for t in range(len(sizes)):
            assert_same_bits(first[t], old.reference()[t], f"first call, segment {t}")
            assert_same_bits(outs.views[t], new.reference()[t], f"same table, new contents, segment {t}")
            assert_same_bits(outs2.views[t], new.reference()[t], f"same table, new outputs, segment {t}")
    finally:
        ctx.close()


@pytest.mark.parametrize("last", ["empty", "table"])
def test_an_identical_table_accumulated_again_folds_again(hip_device, last):
    """``accumulate`` of one table twice, then ``aggregate`` with no table or with the same one a third
    time: the rows are folded two or three times. The first wave starts the accumulator and the second
    continues it — ``acc_in`` is part of the compared blob, the tables differ in nothing else."""
    sizes, case, _ = _reuse_setup(hip_device)
    ctx = FedAvgContext(layout_of(sizes), hip_device)
    try:
        table = table_of(device_rows(case, hip_device), case.weights, len(sizes))
        outs = Outs(sizes, torch.float64, hip_device, False)
        ctx.accumulate(table, torch.float32)
        ctx.accumulate(table, torch.float32)
        ctx.aggregate(None if last == "empty" else table, torch.float32, outs.views, torch.float64)
        ctx.raise_on_nan()
        times = 2 if last == "empty" else 3
        folded = fv.Case("again", "f32", case.clients * times, np.concatenate([case.weights] * times))
        assert outs.guards_untouched()
        for t, w in enumerate(folded.reference()):
            assert_same_bits(outs.views[t], w, f"{times} folds, segment {t}")
    finally:
        ctx.close()
