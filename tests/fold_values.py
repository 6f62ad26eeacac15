"""Inputs for the contract suite of the dense fold (csrc/fedavg_kernels.hip: ``fedavg_tile_kernel`` /
``tile_body`` and the host half ``note_weight``, ``fma_exact_call``, ``build_blob``, ``stage_tables``):
builders in plain numpy / torch and the cases that tests/test_gpu_fold_contract.py runs. Test support
only (no test in this file); nothing here runs on a GPU. tests/test_fold_values_host.py proves with
tests/pers_reference.py alone that these inputs discriminate.

* ``bound_case`` / ``lone_wide_case`` / ``f64_case`` / ``untame_case`` / ``nnadq_rows``: the cases about
  the fused-fold proof (``significand_bits(in) + max_weight_bits <= 53`` and ``weights_tame``).
* ``weight_bits`` / ``tame``: ``note_weight`` restated.
* ``zero_cases`` / ``nonfinite_cases``: signed zeros, the ``-0.0`` identity, absent tensors, inf and NaN;
  ``plus_zero_chain`` is the fold with the wrong start value.
* ``pattern_case``: every 16-bit pattern, and fp32 patterns with subnormals.
* ``Guarded``: outputs as slices of one sentinel-filled buffer.
* ``blob_bytes`` / ``slot_regrows``: ``BlobLayout`` and the slot rotation of ``stage_tables`` restated.

A case holds float64 arrays that are exact in its input format; the GPU suite narrows them. Sizes come
from the built library (``fedavg_kernel_constant``), never from a number written here.
"""

from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

from oracle import nnadq_oracle
from oracle.fedavg_oracle import fedavg_flat
from tests import pers_reference as pref
from tests.pers_values import FOLD_BOUND, SIG, full_values, odd_weights
from tests.robust_values import DTYPES, SENTINEL, all_patterns_16, random_patterns

CLIENTS = 6                       # six clients: two bf16 clients differ in under 8 % of the elements
FUSABLE = tuple(FOLD_BOUND)       # f32, f16, bf16: fp64 inputs never fuse
VARIANTS = ("pos", "neg", "up", "down")   # positive, negative, 2^40- and 2^-40-scaled weights
WAVES3 = [(0, 2), (2, 4), (4, 6)]


def K(name: str) -> int:
    from distributed_learning_simulation_lib_amd import _native

    return _native.kernel_constant(name)


def geometry(code: str) -> dict:
    """The build's sizes for inputs of ``code``: ``n`` elements per 16-byte lane vector, ``lv`` elements
    per lane-vector row of a whole-layout tile, ``tile`` (ranged launches, fp64 inputs) and ``wide`` (the
    whole-layout tile of 2- and 4-byte inputs; ``tile`` for fp64), the load group and pipeline stage."""
    n = 16 // DTYPES[code].itemsize
    tile = K("tile")
    wide = tile if code == "f64" else (K("tile_wide") or tile)
    return {"n": n, "lv": K(f"lanes_{code}") * n, "tile": tile, "wide": wide, "group": K(f"group_{code}"),
            "pipe": K(f"pipe_{code}")}


def seed_of(*parts) -> int:
    return zlib.crc32("/".join(str(p) for p in parts).encode())


@dataclass
class Case:
    name: str
    code: str
    clients: list                 # [N][T] float64 arrays (exact in ``code``) or None: an absent tensor
    weights: np.ndarray           # [N][T] float64, one per (client, tensor) entry
    planted: list = field(default_factory=list)   # (segment, indices): what a +0.0 start value gets wrong
    expect: list = field(default_factory=list)    # (segment, indices, value): results known in closed form
    waves: list | None = None     # a split into waves that the case is about (None: any)

    @property
    def sizes(self) -> list[int]:
        T = len(self.clients[0])
        return [next(row[t].size for row in self.clients if row[t] is not None) for t in range(T)]

    def present(self, t: int) -> list[int]:
        return [k for k, row in enumerate(self.clients) if row[t] is not None]

    def chain_inputs(self, t: int, base=None):
        ks = self.present(t)
        with np.errstate(all="ignore"):
            xs = [self.clients[k][t] if base is None else base[t] + self.clients[k][t] for k in ks]
        return xs, [float(self.weights[k, t]) for k in ks]

    def reference(self, base=None) -> list[np.ndarray]:
        """[T] float64: ``fedavg_flat`` over the clients that sent the tensor, in table order; a delta
        call restores ``base + x`` in fp64 first."""
        with np.errstate(all="ignore"):
            return [fedavg_flat(*self.chain_inputs(t, base)) for t in range(len(self.sizes))]

    def totals(self) -> list[float]:
        out = []
        for t in range(len(self.sizes)):
            ws = self.chain_inputs(t)[1]
            tot = ws[0]
            for w in ws[1:]:
                tot += w
            out.append(tot)
        return out

    def verdict(self, base=None):
        """What ``raise_on_nan`` must report: None, or (stage, bad client rows) — ``input`` when a client
        tensor holds a NaN, else ``accumulator`` when a weighted sum is NaN, else ``result``."""
        bad = [k for k, row in enumerate(self.clients) if any(x is not None and np.isnan(x).any() for x in row)]
        if bad:
            return "input", bad
        accs = [pref.separate_chain(*self.chain_inputs(t, base)) for t in range(len(self.sizes))]
        if any(np.isnan(a).any() for a in accs):
            return "accumulator", []
        if any(np.isnan(r).any() for r in self.reference(base)):
            return "result", []
        return None


def plus_zero_chain(case: Case, base=None) -> list[np.ndarray]:
    """The fold started from +0.0 instead of the identity -0.0 (what ``acc[i] = 0.0`` would compute)."""
    out = []
    with np.errstate(all="ignore"):
        for t, size in enumerate(case.sizes):
            xs, ws = case.chain_inputs(t, base)
            acc = np.zeros(size)
            for x, w in zip(xs, ws):
                acc = acc + x * np.float64(w)
            out.append(acc / case.totals()[t])
    return out


def delta_base(sizes, seed: int, identity_at=()) -> list[np.ndarray]:
    """A base model of 53-bit values; -0.0 (``-0.0 + x == x`` for every x) at ``identity_at[t]``."""
    rng = np.random.default_rng(seed)
    base = [rng.standard_normal(s) for s in sizes]
    for t, idx in identity_at:
        base[t][idx] = -0.0
    return base


def _rows(rng, n: int, sizes, code: str) -> list:
    return [[full_values(rng, s, code) for s in sizes] for _ in range(n)]


def _spread(w, T: int) -> np.ndarray:
    return np.repeat(np.asarray(w, dtype=np.float64)[:, None], T, axis=1)


# ---- B. the fused-fold bound ---------------------------------------------------------------------
def bound_sizes(code: str) -> list[int]:
    """A ragged tile first and the wide tile + 1 last (the lone wide weights sit in these two), and
    between them one lane vector -1 / +1 and the wide tile - 1."""
    g = geometry(code)
    return [g["tile"] + 77, max(1, g["n"] - 1), g["n"] + 1, g["wide"] - 1, g["wide"] + 1]


def _vary(w: np.ndarray, variant: str) -> np.ndarray:
    return {"pos": w, "neg": -w, "up": w * 2.0 ** 40, "down": w * 2.0 ** -40}[variant]


def bound_case(code: str, where: str, variant: str, sizes) -> Case:
    """Six clients of full values; every weight ``FOLD_BOUND`` (``at``) or one bit more (``past``) wide."""
    b = FOLD_BOUND[code] + {"at": 0, "past": 1}[where]
    rng = np.random.default_rng(seed_of("bound", code, where, variant))
    clients = _rows(rng, CLIENTS, sizes, code)
    w = _vary(odd_weights(rng, CLIENTS, b), variant)
    return Case(f"bound {code} {where} {variant}", code, clients, _spread(w, len(sizes)))


LONE_PLACES = ("middle_first", "last_last", "cache")


def lone_wide_case(code: str, place: str, sizes) -> Case:
    """Weights at the bound, one per client, but for one entry one bit past it: client 3 of the first
    tensor (``middle_first``), client 5 of the last (``last_last``), or — ``cache`` — the first tensor's
    entries run narrow a, a, wide W, W, narrow, narrow: the wide one follows a repeat.
    ``client0`` (host proof only): the first fold rounds its product either way."""
    b = FOLD_BOUND[code]
    rng = np.random.default_rng(seed_of("lone", code, place))
    clients = _rows(rng, CLIENTS, sizes, code)
    w = _spread(odd_weights(rng, CLIENTS, b), len(sizes))
    wide = float(odd_weights(rng, (), b + 1))
    if place == "middle_first":
        w[3, 0] = wide
    elif place == "last_last":
        w[5, -1] = wide
    elif place == "cache":
        w[1, 0] = w[0, 0]
        w[2, 0] = w[3, 0] = wide
    elif place == "client0":
        w[0, 0] = wide
    else:
        raise ValueError(place)
    return Case(f"lone {code} {place}", code, clients, w)


def f64_case(kind: str, sizes) -> Case:
    """fp64 inputs (53-bit values) with power-of-two weights or 2-bit weights 3 * 2^j."""
    rng = np.random.default_rng(seed_of("f64", kind))
    clients = _rows(rng, CLIENTS, sizes, "f64")
    j = rng.integers(-3, 6, CLIENTS).astype(np.float64)
    w = np.exp2(j) * {"pow2": 1.0, "two_bit": 3.0}[kind]
    return Case(f"f64 {kind}", "f64", clients, _spread(w, len(sizes)))


def zero_weights_case(code: str, sizes) -> Case:
    rng = np.random.default_rng(seed_of("zero weights", code))
    return Case(f"zero weights {code}", code, _rows(rng, CLIENTS, sizes, code), np.zeros((CLIENTS, len(sizes))))


BIG, SMALL = 2.0 ** 900, 2.0 ** -900
OVERFLOWS = ("f32", "bf16")       # formats that reach 2^124: fp16 ends at 65504


def untame_case(code: str, sizes) -> Case:
    """Weights 2^900 (clients 1 and 4) and 2^-900 (client 2) among weights at the bound: 1-bit
    significands, which the bound alone would let fuse. For fp32 and bf16 three elements of tensor 0
    hold -1.5 * 2^123 in client 1 and 2^124 in client 4 (0 elsewhere): the second product overflows on
    its own (inf, the reference) and does not once fused with the sum (2^1022)."""
    rng = np.random.default_rng(seed_of("untame", code))
    clients = _rows(rng, CLIENTS, sizes, code)
    w = odd_weights(rng, CLIENTS, FOLD_BOUND[code])
    w[1] = w[4] = BIG
    w[2] = SMALL
    case = Case(f"untame {code}", code, clients, _spread(w, len(sizes)))
    if code in OVERFLOWS:
        at = spots_of(sizes[0])
        for k in range(CLIENTS):
            clients[k][0][at] = {1: -1.5 * 2.0 ** 123, 4: 2.0 ** 124}.get(k, 0.0)
        case.expect = [(0, at, np.inf)]
    return case


def nnadq_rows(codec: str, sizes, n: int = CLIENTS):
    """[n][T] records of ``nnadq_oracle.quantize`` whose dequantised values have full significands with
    the lowest bit set: x = lo + code * step with lo = ±(1 + ulp) or so and step = 2 ulp, every code
    0 .. 255 present. And the dequantised values, [n][T] arrays of the codec's dtype."""
    dt = np.float32 if codec == "float32" else np.float64
    ulp = 2.0 ** -23 if codec == "float32" else 2.0 ** -52
    rng = np.random.default_rng(seed_of("nnadq", codec))
    recs, dense = [], []
    for k in range(n):
        lo = (1.0 + ulp) if k % 2 == 0 else -(2.0 - ulp)
        rrow, drow = [], []
        for s in sizes:
            codes = rng.integers(0, 256, s)
            codes[:2] = (0, 255) if s >= 2 else 0
            x = (lo + codes * (2.0 * ulp)).astype(dt)
            rec = nnadq_oracle.quantize(x, 1e-30)     # a step far below the range: all 255 levels
            rrow.append(rec)
            drow.append(nnadq_oracle.dequantize(rec, s, dt))
        recs.append(rrow)
        dense.append(drow)
    return recs, dense


# ---- note_weight restated ------------------------------------------------------------------------
def weight_bits(w: float) -> int:
    """Bits between the leading and the trailing one of w's significand: 53 - ctz(significand); 0 for
    zero (and for inf / NaN, which are not tame anyway)."""
    if w == 0 or not math.isfinite(w):
        return 0
    m, _ = math.frexp(abs(w))
    sig = int(m * 2 ** 53)
    return 53 - ((sig & -sig).bit_length() - 1)


def tame(w: float) -> bool:
    """Zero, or finite, normal and |w| = m * 2^e (m in [0.5, 1)) with -800 <= e <= 800."""
    if w == 0:
        return True
    if not math.isfinite(w) or abs(w) < 2.0 ** -1022:
        return False
    return -800 <= math.frexp(w)[1] <= 800


def fusable(case: Case) -> bool:
    """``fma_exact_call`` over every entry of a call."""
    ws = [float(case.weights[k, t]) for t in range(len(case.sizes)) for k in case.present(t)]
    return all(tame(w) for w in ws) and SIG[case.code] + max(weight_bits(w) for w in ws) <= 53


# ---- C. signed zeros, the identity, absent tensors -----------------------------------------------
def spots_of(size: int) -> np.ndarray:
    return np.array(sorted({0, size // 2, size - 1}))


def zero_sizes(code: str) -> list[int]:
    """One whole-layout tile, two lane-vector rows and a ragged tail of 3; and a tensor of 5."""
    g = geometry(code)
    return [g["wide"] + 2 * g["lv"] + 3, 5]


def zero_spots(code: str, sizes) -> list[np.ndarray]:
    """Tensor 0: its first element, one inside the full tile, one inside the whole lane vectors behind
    it, two of the ragged tail (the last element among them); tensor 1: first and last."""
    g = geometry(code)
    big = sizes[0]
    assert big == g["wide"] + 2 * g["lv"] + 3
    return [np.array([0, g["wide"] // 2 + 1, g["wide"] + g["lv"] // 2, big - 2, big - 1]), np.array([0, sizes[1] - 1])]


ZERO_CASES = ("neg_zeros", "pos_zeros_neg_weights", "neg_zero_weight", "minus_then_plus", "plus_then_minus", "cancel",
              "absent_first_wave", "absent_middle_wave", "absent_last_wave", "single_client")


def zero_case(which: str, code: str, kind: str, sizes, spots) -> Case:
    """One signed-zero case (see ``ZERO_CASES``); ``kind``: ``int`` weights 1 .. 500 or ``frac`` ones.
    Every case is meant for one launch and for the three waves ``WAVES3`` alike: the clients it is about
    (1 and 4; 0; an absent pair) then sit in different waves."""
    rng = np.random.default_rng(seed_of("zero", which, code, kind))
    T = range(len(sizes))
    clients = _rows(rng, CLIENTS, sizes, code)
    w = rng.integers(1, 501, CLIENTS).astype(np.float64) if kind == "int" else rng.uniform(0.01, 3.0, CLIENTS)

    def fill(value, only=None):
        for k in range(CLIENTS):
            for t in T:
                if only is None or k in only:
                    clients[k][t][spots[t]] = value

    planted = [(t, spots[t]) for t in T]
    expect = None
    if which == "neg_zeros":                       # -0.0 * w = -0.0 throughout: -0.0 / W = -0.0
        fill(-0.0)
        expect = -0.0
    elif which == "pos_zeros_neg_weights":         # +0.0 * -w = -0.0 throughout: -0.0 / -W = +0.0
        fill(0.0)
        w = -w
        expect = 0.0
    elif which == "neg_zero_weight":               # client 2: x * -0.0 = -0.0 for its positive values
        fill(-0.0)
        for t in T:
            clients[2][t][spots[t]] = np.abs(full_values(rng, len(spots[t]), code))
        w[2] = -0.0
        expect = -0.0
    elif which == "minus_then_plus":               # -0.0 + +0.0 = +0.0, and it stays
        fill(-0.0)
        fill(0.0, only=(4,))
        planted, expect = [], 0.0
    elif which == "plus_then_minus":               # the first fold: fma(+0.0, w, -0.0) = +0.0
        fill(-0.0)
        fill(0.0, only=(0,))
        planted, expect = [], 0.0
    elif which == "cancel":                        # x * w + (-x) * w = +0.0
        fill(-0.0)
        for t in T:
            clients[1][t][spots[t]] = np.abs(full_values(rng, len(spots[t]), code))
            clients[4][t][spots[t]] = -clients[1][t][spots[t]]
        w[4] = w[1]
        planted, expect = [], 0.0
    elif which.startswith("absent_"):              # tensor 0 missing from one whole wave
        fill(-0.0)
        a, b = WAVES3[("absent_first_wave", "absent_middle_wave", "absent_last_wave").index(which)]
        for k in range(a, b):
            clients[k][0] = None
        expect = -0.0
    elif which == "single_client":                 # tensor 1 in client 3 alone: one fold into the identity
        fill(-0.0)
        for k in range(CLIENTS):
            if k != 3:
                clients[k][1] = None
        expect = -0.0
    else:
        raise ValueError(which)
    case = Case(f"{which} {code} {kind}", code, clients, _spread(w, len(sizes)), planted=planted)
    case.expect = [(t, spots[t], expect) for t in T]
    return case


NONFINITE_CASES = ("inf_times_zero", "inf_minus_inf", "nan_first", "nan_last", "zero_total")


def nonfinite_case(which: str, code: str, sizes, spots) -> Case:
    """inf * 0 (NaN in the sum), +inf and -inf in two waves, a NaN in the first and in the last client of
    ``group + 1`` (the last load group holds one client), and a total weight of exactly 0 with sums of
    exactly 0 at the spots (0 / 0) and x / 0 elsewhere."""
    rng = np.random.default_rng(seed_of("nonfinite", which, code))
    T = range(len(sizes))
    n = geometry(code)["group"] + 1 if which.startswith("nan_") else CLIENTS
    clients = _rows(rng, n, sizes, code)
    w = rng.integers(1, 501, n).astype(np.float64)
    waves = None
    if which == "inf_times_zero":
        w[2] = 0.0
        for t in T:
            clients[2][t][spots[t]] = np.inf
    elif which == "inf_minus_inf":
        for t in T:
            clients[1][t][spots[t]] = np.inf
            clients[4][t][spots[t]] = -np.inf
        waves = [(0, 3), (3, 6)]
    elif which in ("nan_first", "nan_last"):
        k = 0 if which == "nan_first" else n - 1
        clients[k][0][spots[0][1]] = np.nan
    elif which == "zero_total":
        w[1::2] = -w[0::2]
        for t in T:
            for k in range(1, n):
                clients[k][t][spots[t]] = clients[0][t][spots[t]]
    else:
        raise ValueError(which)
    return Case(f"{which} {code}", code, clients, _spread(w, len(sizes)), waves=waves)


# ---- D. every bit pattern ------------------------------------------------------------------------
PATTERN_WEIGHTS = ("one", "w53")
MIN_SUBNORMALS = 64


def pattern_tensor(code: str) -> torch.Tensor:
    """fp16 / bf16: all 65536 patterns (NaNs replaced) and five more subnormals behind them — whole
    wide tiles and a ragged tail; fp32: random patterns over two wide tiles + 5, the first elements
    both zeros, the largest finite values and the smallest subnormals."""
    dt = DTYPES[code]
    if code in ("f16", "bf16"):
        t, replaced = all_patterns_16(dt)
        assert replaced == {"f16": 2046, "bf16": 254}[code]
        return torch.cat([t, t[1:6]])
    assert code == "f32"
    gen = torch.Generator().manual_seed(seed_of("patterns", code))
    t, _ = random_patterns(gen, 2 * geometry(code)["wide"] + 5, dt)
    fmax, tiny = float(np.finfo(np.float32).max), 2.0 ** -149
    t[:6] = torch.tensor([0.0, -0.0, fmax, -fmax, tiny, -tiny], dtype=torch.float64).to(dt)
    return t


def is_subnormal(x: np.ndarray, code: str) -> np.ndarray:
    smallest_normal = {"f32": 2.0 ** -126, "f16": 2.0 ** -14, "bf16": 2.0 ** -126}[code]
    return (x != 0) & (np.abs(x) < smallest_normal)


def pattern_case(code: str, weight: str) -> tuple[Case, torch.Tensor]:
    """Three clients over one tensor: the patterns in the middle one, -0.0 (the identity) in the others.
    ``one``: weights 1, 1, 2 (fused; the result is the pattern / 4, exact); ``w53``: a 53-bit weight on
    the patterns (the separately rounded fold). And the pattern tensor in its own dtype."""
    t = pattern_tensor(code)
    x = t.to(torch.float64).numpy()
    rng = np.random.default_rng(seed_of("pattern weight", code))
    mid = 1.0 if weight == "one" else float(odd_weights(rng, (), 53)) * 2.0 ** -52
    w = np.array([[1.0], [mid], [2.0]])
    return Case(f"patterns {code} {weight}", code, [[np.full(x.size, -0.0)], [x], [np.full(x.size, -0.0)]], w), t


def pattern_base(size: int, seed: int) -> list[np.ndarray]:
    """-0.0 at the even elements (``base + x`` is x exactly), 53-bit values at the odd ones."""
    return delta_base([size], seed, [(0, np.arange(0, size, 2))])


# ---- E. nothing else is written ------------------------------------------------------------------
class Guarded:
    """One output view per segment inside ONE sentinel-filled buffer: every view starts at a 16-byte
    boundary — but ``misalign_at``, which starts one element behind one — with at least 16 bytes of
    sentinels before it, between two of them and behind the last. Plain torch: any device."""

    def __init__(self, sizes, dtype: torch.dtype, device, misalign_at: int | None = None) -> None:
        per16 = 16 // dtype.itemsize
        self.offsets, at = [], per16
        for i, s in enumerate(sizes):
            off = at + (1 if i == misalign_at else 0)
            self.offsets.append(off)
            at = (off + s + per16 - 1) // per16 * per16 + per16
        self.buf = torch.full((at,), SENTINEL, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + s] for o, s in zip(self.offsets, sizes)]
        self.mask = np.zeros(at, dtype=bool)
        for o, s in zip(self.offsets, sizes):
            assert not self.mask[o - 1] and not self.mask[o:o + s].any()
            self.mask[o:o + s] = True
        for i, v in enumerate(self.views):
            assert (v.data_ptr() % 16 != 0) == (i == misalign_at) and v.is_contiguous()

    def gaps_untouched(self) -> bool:
        return bool((self.buf.cpu().numpy()[~self.mask] == SENTINEL).all())

    def numpy(self) -> list[np.ndarray]:
        host = self.buf.cpu().numpy()
        return [host[o:o + v.numel()] for o, v in zip(self.offsets, self.views)]


# ---- F. table slots ------------------------------------------------------------------------------
SLOTS = 4                    # fedavg_ctx::kSlots
FIRST_SLOT = 64 * 1024       # a slot's first capacity; one that is too small regrows to twice the need


def blob_bytes(T: int, Kc: int) -> int:
    """``BlobLayout(T, max(K, 1)).bytes``: [T][K] pointers and weights, then per tensor the client count,
    the accumulator flag, the output, the total and the base; every section 16-byte aligned, the blob
    rounded up to 256 bytes."""
    def up(x, a):
        return (x + a - 1) // a * a
    kr = max(Kc, 1)
    off = up(8 * T * kr, 16)              # pointers
    off = up(off + 8 * T * kr, 16)        # weights
    off = up(off + 4 * T, 16)             # kseg
    off = up(off + 4 * T, 16)             # acc_in
    off = up(off + 8 * T, 16)             # outs
    off = up(off + 8 * T, 16)             # wtot
    return up(off + 8 * T, 256)           # base


def slot_regrows(needs) -> list[int]:
    """The calls (by index) at which ``stage_tables`` frees and regrows a slot, for a fresh context
    whose every call uploads: call i takes slot i % SLOTS."""
    caps, out = [0] * SLOTS, []
    for i, b in enumerate(needs):
        s = i % SLOTS
        if caps[s] < b:
            if caps[s]:
                out.append(i)
            caps[s] = max(2 * b, FIRST_SLOT)
    return out


SLOT_T = 64
SLOT_CLIENTS = (3, 8, 20, 40, 70, 100, 150)     # seven calls: the last three outgrow their slots


def slot_sizes() -> list[int]:
    """64 short tensors (whole 16-byte vectors but the last, which is ragged)."""
    return [36] * (SLOT_T - 1) + [41]


def exact_fused_overflow_free(x1: float, x4: float, w: float) -> bool:
    """For the planted elements of ``untame_case``: x4 * w alone leaves the fp64 range, x1 * w + x4 * w
    does not."""
    limit = Fraction(2) ** 1024
    return abs(Fraction(x4) * Fraction(w)) >= limit > abs(Fraction(x1) * Fraction(w) + Fraction(x4) * Fraction(w))
