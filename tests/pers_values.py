"""Inputs for the contract suite of the personalized kernel (csrc/personalized_kernels.hip):
generators in plain numpy and the cases that tests/test_gpu_pers_contract.py runs. Test support only
(no test in this file); nothing is imported from the package. tests/test_pers_values_host.py proves
with tests/pers_reference.py alone that these inputs discriminate.

* ``full_values``: values with a full significand of the input format whose lowest significand bit
  is 1, so a product with a b-bit odd weight is exactly ``sig + b`` (or one less) bits wide.
* ``odd_weights``: odd integers in [2^(b-1), 2^b): weights of an exact significand width.
* ``fold_case`` / ``own_wide_case`` / ``untame_case``: the cases about the fused-fold proof.
* ``refold_cases``: sums that come out as ±0 or NaN in the kernel's branch-free main loop and need
  its refold; ``main_loop_without_refold`` is that loop restated.
* ``ring_*``: the client and receiver counts at the edges of the LDS ring.
* ``blob_bytes``: the size of a call's table blob, from the host half's own arithmetic.

A case holds float64 arrays that are exact in its input format; the GPU suite narrows them.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import pers_reference as pref

SIG = {"f32": 24, "f16": 11, "bf16": 8, "f64": 53}           # significand bits, the hidden one included
FOLD_BOUND = {c: 53 - SIG[c] for c in ("f32", "f16", "bf16")}  # b*: 29, 42, 45
# the documented geometry; the GPU suite takes its own from the built library
DEFAULT = {"chunk": 256, "jb": 16, "group": 128, "u": 2, "stage": 4, "depth": 3}
OUTSIDER = 1000   # ids from here on belong to no client


@dataclass
class Case:
    name: str
    clients: list            # [N][T] float64 arrays or None
    client_ids: list
    weights: np.ndarray      # [M][N] float64
    receiver_ids: list
    # (row, segment, indices): elements that the main loop alone gets wrong (they need the refold)
    planted: list = field(default_factory=list)
    # (row, segment, indices, value): elements whose result is known in closed form
    expect: list = field(default_factory=list)
    finite_rows: list = field(default_factory=list)   # rows whose whole result must be finite

    @property
    def sizes(self) -> list[int]:
        row = next(r for r in self.clients if all(x is not None for x in r))
        return [x.size for x in row]

    def reference(self) -> pref.Result:
        return pref.reduce(self.clients, self.client_ids, self.weights, self.receiver_ids)


def full_values(rng: np.random.Generator, numel: int, code: str, exps=(-3, 3)) -> np.ndarray:
    """float64 [numel], exact in the format ``code``: ±m·2^(e - sig + 1) with m a random odd integer
    of exactly ``sig`` bits and e uniform over ``exps`` (inclusive). Finite, normal, non-zero."""
    sig = SIG[code]
    m = rng.integers(2 ** (sig - 1), 2 ** sig, size=numel, dtype=np.int64) | 1
    e = rng.integers(exps[0], exps[1] + 1, size=numel)
    sign = rng.integers(0, 2, size=numel) * 2.0 - 1.0
    return sign * np.ldexp(m.astype(np.float64), e - (sig - 1))


def odd_weights(rng: np.random.Generator, shape, b: int) -> np.ndarray:
    """float64 odd integers in [2^(b-1), 2^b): significands of exactly b bits (b <= 53)."""
    assert 1 <= b <= 53
    lo = 2 ** (b - 1)
    return (rng.integers(lo, 2 ** b, size=shape, dtype=np.int64) | 1).astype(np.float64)


def weights_of(rng: np.random.Generator, shape, kind: str) -> np.ndarray:
    """``int``: integers 1 .. 500 (every product exact: the fused fold); ``frac``: uniform in
    [0.01, 3) (53-bit significands: the separately rounded fold)."""
    if kind == "int":
        return rng.integers(1, 501, size=shape).astype(np.float64)
    return rng.uniform(0.01, 3.0, size=shape)


def receiver_ids_of(M: int, own: dict[int, int]) -> list[int]:
    """Row j has the id ``own[j]`` (a client's), every other row an id of its own."""
    return [own.get(j, OUTSIDER + j) for j in range(M)]


# ---- the fused-fold proof ------------------------------------------------------------------------
FOLD_CLIENTS = 6


def fold_case(code: str, chunk: int, M: int, wide_row: int | None) -> Case:
    """Six clients of full values over [chunk + 3] elements; every weight b* bits wide but for
    ``wide_row`` (if any), whose weights are all b* + 1 bits wide. Rows 0 to 2 are clients 0 to 2
    (own update excluded), the others fold all six."""
    b = FOLD_BOUND[code]
    rng = np.random.default_rng(4100 + 10 * list(SIG).index(code) + (0 if wide_row is None else 1 + wide_row % 5))
    clients = [[full_values(rng, chunk + 3, code)] for _ in range(FOLD_CLIENTS)]
    w = odd_weights(rng, (M, FOLD_CLIENTS), b)
    if wide_row is not None:
        w[wide_row] = odd_weights(rng, FOLD_CLIENTS, b + 1)
    return Case(f"fold {code} wide={wide_row}", clients, list(range(FOLD_CLIENTS)), w,
                receiver_ids_of(M, {0: 0, 1: 1, 2: 2}))


def own_wide_case(code: str, chunk: int) -> Case:
    """``fold_case`` at b* with a 53-bit weight on every pair that is a receiver's own update — the
    pairs nobody folds, so they do not count for the proof."""
    case = fold_case(code, chunk, 4, None)
    rng = np.random.default_rng(4200)
    for j in range(3):
        case.weights[j, j] = odd_weights(rng, (), 53)
    case.name = f"own-wide {code}"
    return case


def untame_case(code: str, chunk: int) -> Case:
    """Weights 2^900 and 2^-900 (a product with them could leave the fp64 range, so no proof
    holds): row 0 all 2^900, row 1 all 2^-900, rows 2 and 3 mixed. With values near 1 every product
    and sum stays finite and normal, so the result is the reference's whichever fold runs: the case
    records that such weights are served, not which fold serves them."""
    rng = np.random.default_rng(4300 + list(SIG).index(code))
    clients = [[full_values(rng, chunk + 3, code)] for _ in range(FOLD_CLIENTS)]
    big, small = 2.0 ** 900, 2.0 ** -900
    w = np.empty((4, FOLD_CLIENTS))
    w[0], w[1] = big, small
    w[2] = [big, small] * (FOLD_CLIENTS // 2)
    w[3] = [small, big] * (FOLD_CLIENTS // 2)
    return Case(f"untame {code}", clients, list(range(FOLD_CLIENTS)), w, receiver_ids_of(4, {0: 0, 1: 1}))


# ---- the refold ----------------------------------------------------------------------------------
def spots(size: int) -> np.ndarray:
    """Three elements of a segment: its first, its middle and its last."""
    return np.array(sorted({0, size // 2, size - 1}) if size >= 3 else range(size))


def _rows(rng, n, sizes, code):
    return [[full_values(rng, s, code) for s in sizes] for _ in range(n)]


def refold_case(which: str, code: str, kind: str, sizes, jb: int, group: int, row: int = 0) -> Case:
    """One case of the refold (see ``refold_cases``)."""
    rng = np.random.default_rng(5000 + 97 * list(SIG).index(code) + 13 * ("int", "frac").index(kind)
                                + sum(map(ord, which)) + row)
    T = range(len(sizes))
    at = [spots(s) for s in sizes]
    if which == "own_plus_one":
        # (i) every folded value is -0.0 where the receiver's own update holds +1.0: x * 0 = +0.0
        # turns the -0.0 sum into +0.0. Four clients: no padding client takes part.
        clients = _rows(rng, 4, sizes, code)
        for k in range(4):
            for t in T:
                clients[k][t][at[t]] = 1.0 if k == 2 else -0.0
        case = Case(which, clients, [0, 1, 2, 3], weights_of(rng, (3, 4), kind), [2, 0, OUTSIDER])
        case.planted = [(0, t, at[t]) for t in T]
        case.expect = [(0, t, at[t], -0.0) for t in T]
    elif which == "padding":
        # every client holds -0.0: the padding clients (0 * 0 = +0.0) alone flip the sign
        clients = _rows(rng, 5, sizes, code)
        for k in range(5):
            for t in T:
                clients[k][t][at[t]] = -0.0
        case = Case(which, clients, [0, 1, 2, 3, 4], weights_of(rng, (2, 5), kind), [OUTSIDER, 3])
        case.planted = [(j, t, at[t]) for j in range(2) for t in T]
        case.expect = [(j, t, at[t], -0.0) for j in range(2) for t in T]
    elif which == "own_poison":
        # (ii) the only receiver's own update holds +inf, -inf and NaN: nobody folds them
        clients = _rows(rng, 4, sizes, code)
        for t in T:
            clients[1][t][at[t]] = np.array([np.inf, -np.inf, np.nan])[:len(at[t])]
        case = Case(which, clients, [0, 1, 2, 3], weights_of(rng, (1, 4), kind), [1])
        case.planted = [(0, t, at[t]) for t in T]
        case.finite_rows = [0]
    elif which == "own_poison_among_many":
        # (iii) that receiver at ``row`` among group + 1; every other receiver folds the poisoned
        # client with a real weight and gets the reference's inf / NaN
        M = group + 1
        clients = _rows(rng, 6, sizes, code)
        for t in T:
            clients[0][t][at[t]] = np.array([np.inf, -np.inf, np.nan])[:len(at[t])]
        own = {row: 0}
        for k, j in zip(range(1, 6), [j for j in range(M) if j != row]):
            own[j] = k
        w = weights_of(rng, (M, 6), kind)
        assert (w[:, 0] != 0).all()
        case = Case(f"{which} row {row}", clients, list(range(6)), w, receiver_ids_of(M, own))
        case.planted = [(row, t, at[t]) for t in T]
        case.finite_rows = [row]
    elif which == "cancel":
        # (iv) x and -x with equal weights and a non-zero own update: +0.0, with or without the
        # refold (it runs, and must not change the sign)
        clients = _rows(rng, 3, sizes, code)
        for t in T:
            clients[2][t][at[t]] = -clients[1][t][at[t]]
        w = weights_of(rng, (2, 3), kind)
        w[0, 2] = w[0, 1]
        case = Case(which, clients, [0, 1, 2], w, [0, OUTSIDER])
        case.expect = [(0, t, at[t], 0.0) for t in T]
    elif which == "absent":
        # (v) client 2 did not send segment 0 — it folds as the zero block, +0.0 * w, into sums
        # that are -0.0 — and holds +inf in segment 1
        clients = _rows(rng, 4, sizes, code)
        for k in range(4):
            clients[k][0][at[0]] = -0.0
        clients[2][0] = None
        clients[2][1][min(5, sizes[1] - 1)] = np.inf
        case = Case(which, clients, [0, 1, 2, 3], weights_of(rng, (2, 4), kind), [OUTSIDER, 0])
        case.planted = [(j, 0, at[0]) for j in range(2)]
        case.expect = [(j, 0, at[0], -0.0) for j in range(2)]
    else:
        raise ValueError(which)
    return case


def poison_rows(jb: int, group: int) -> list[int]:
    return [0, jb - 1, jb, group - 1, group]


def refold_cases(code: str, kind: str, sizes, jb: int, group: int, part: str = "all") -> list[Case]:
    """``few``: the cases with a handful of receivers, (i), (ii), (iv), (v) and the padding one;
    ``many``: (iii), the poisoned own update at each of ``poison_rows`` among group + 1 receivers."""
    out = []
    if part in ("all", "few"):
        out += [refold_case(w, code, kind, sizes, jb, group)
                for w in ("own_plus_one", "padding", "own_poison", "cancel", "absent")]
    if part in ("all", "many"):
        out += [refold_case("own_poison_among_many", code, kind, sizes, jb, group, r) for r in poison_rows(jb, group)]
    return out


def main_loop_without_refold(case: Case, pad: int) -> list[list[np.ndarray]]:
    """The kernel's main loop restated, with no refold behind it: the accumulator starts at -0.0,
    every client of the list padded to a multiple of ``pad`` is folded — a receiver's own update
    and a padding client with weight 0, an absent tensor and a padding client as zeros — and the
    sum is divided by the reference's total. [M][T] float64."""
    N = len(case.clients)
    npad = (N + pad - 1) // pad * pad
    totals = case.reference().totals
    outs = []
    with np.errstate(all="ignore"):
        for j, rid in enumerate(case.receiver_ids):
            row = []
            for t, size in enumerate(case.sizes):
                acc = np.full(size, -0.0)
                for k in range(npad):
                    x = case.clients[k][t] if k < N and case.clients[k][t] is not None else np.zeros(size)
                    w = case.weights[j, k] if k < N and case.client_ids[k] != rid else 0.0
                    acc = acc + x * np.float64(w)
                row.append(acc / totals[j, t])
            outs.append(row)
    return outs


# ---- the ring ------------------------------------------------------------------------------------
def ring_receivers(jb: int) -> list[int]:
    return [1, jb, jb + 1, 2 * jb + 1, 3 * jb + 1]          # 1, 1, 2, 3 and 4 waves


def ring_client_counts(stage: int, depth: int) -> list[int]:
    """1 stage, 2 stages, ``depth`` and ``depth + 1`` stages (the ring's look-ahead and one more),
    and one full wrap of its ``depth + 2`` stages, each with and without a started next stage."""
    return [1, 2, stage, stage + 1, depth * stage, depth * stage + 1, (depth + 2) * stage,
            (depth + 2) * stage + 1, (depth + 3) * stage]


def ring_pairs(jb: int, stage: int, depth: int) -> list[tuple[int, int]]:
    """(clients, receivers): every client count once with one wave (1 and ``jb`` receivers in turn),
    once with two waves, and the counts cycled over the 3- and 4-wave receiver counts."""
    recv = ring_receivers(jb)
    pairs = []
    for i, n in enumerate(ring_client_counts(stage, depth)):
        pairs += [(n, recv[i % 2]), (n, recv[2]), (n, recv[3 + i % 2])]
    return pairs


def table_case(code: str, kind: str, N: int, M: int, sizes, seed: int, absent: bool = True,
               own_rows: int | None = None) -> Case:
    """A round of full values. As many receivers as the ids allow (or ``own_rows`` of them) are
    clients too (their own update is excluded): row j is client N - 1 - j while j < N, with N >= 3;
    with two clients only row 0 is one, with one client nobody can be (a receiver needs somebody to
    fold). The last client did not send segment 0 (``absent``, from two clients on)."""
    rng = np.random.default_rng(seed)
    clients = _rows(rng, N, sizes, code)
    if absent and N >= 2:
        clients[N - 1][0] = None
    rows_own = 0 if N == 1 else 1 if N == 2 else min(M, N, N if own_rows is None else own_rows)
    own = {j: N - 1 - j for j in range(rows_own)}
    return Case(f"table {N}x{M}", clients, list(range(N)), weights_of(rng, (M, N), kind), receiver_ids_of(M, own))


def isolation_case(code: str, chunk: int, ve: int = 4):
    """Five clients that are the five receivers, over [ve + 1, chunk + 3, chunk - 1] elements, with
    two real zero weights; and the element that the test changes: client 2's element ``chunk + 1``
    of segment 1 becomes 2^15. Receiver 2 is that client and receiver 4 weighs it 0: neither may
    change."""
    sizes = [ve + 1, chunk + 3, chunk - 1]
    case = table_case(code, "frac", 5, 5, sizes, seed=4400 + list(SIG).index(code), absent=False)
    case.receiver_ids = list(case.client_ids)
    case.weights[4, 2] = 0.0
    case.weights[1, 3] = 0.0
    return case, (2, 1, chunk + 1), 2.0 ** 15


# ---- the table blob ------------------------------------------------------------------------------
def blob_bytes(N: int, M: int, T: int, geo: dict = DEFAULT) -> int:
    """Bytes of a call's table blob (``fedavg_pers_aggregate``): [T][Npad] client pointers; per
    launch group Npad x group weights, N x (group / jb) int32 masks, group x T totals, outputs and
    reciprocals; [T] centralized outputs — each rounded up to 256 bytes — and the zero block."""
    def up(x):
        return (x + 255) // 256 * 256
    pad = max(geo["u"], geo["stage"])
    npad = (N + pad - 1) // pad * pad
    groups = (M + geo["group"] - 1) // geo["group"]
    per_group = (up(8 * npad * geo["group"]) + up(4 * N * (geo["group"] // geo["jb"]))
                 + 3 * up(8 * geo["group"] * T))
    return up(8 * T * npad) + per_group * groups + up(8 * T) + 8 * geo["chunk"]


FIRST_BLOB = 64 * 1024   # the capacity of the first blob; a call that needs more regrows it to twice its need
