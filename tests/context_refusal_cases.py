"""The refusals of ``FedAvgContext``'s side-kernel wrappers (``robust_aggregate`` to
``server_opt_step``, ``sparse_aggregate_delta`` and ``SparseTable`` included) as one table of cases,
shared by ``tests/test_context_refusals_host.py`` (a CPU context over a recording stand-in for the
library) and ``tests/test_gpu_context_refusals.py`` (a real context, device tensors).

A case is ``(id, call, exception type, full message)``: ``call(env)`` builds its operands on
``env.device`` and calls the wrapper, which must raise exactly that exception with exactly that text
(``{device}`` and ``{index}`` stand for the context's device and its index) before anything reaches
the library. A case whose id ends in ``-first`` holds two refused conditions at once and pins which
one is reported. The layout has two tensors of 5 and 3 elements; tables hold 2 clients unless the
case is about the count.
"""

from __future__ import annotations

from collections.abc import Callable
from typing import Any, NamedTuple

import torch

from distributed_learning_simulation_lib_amd import _native
from distributed_learning_simulation_lib_amd.fedavg import ClientTable, FedAvgContext, ModelLayout, SparseTable
from distributed_learning_simulation_lib_amd.quantized import QSGD_F32
from distributed_learning_simulation_lib_amd.sparse import SparseDelta

NUMELS = (5, 3)
LAYOUT = ModelLayout(names=("w", "b"), shapes=((5,), (3,)))
OTHER_LAYOUT = ModelLayout(names=("w", "b"), shapes=((5,), (4,)))
F32, F64, F16, I32, U8 = torch.float32, torch.float64, torch.float16, torch.int32, torch.uint8
INF, NAN = float("inf"), float("nan")
QSGD, QSGD64, NNADQ, NNADQ64 = _native.QSGD_F32, _native.QSGD_F64, _native.NNADQ_F32, _native.NNADQ_F64
POINT_MAX, KRUM_MAX = _native.POINT_MAX_CLIENTS, _native.KRUM_MAX_CLIENTS


class Case(NamedTuple):
    id: str
    call: Callable[[Env], Any]
    exc: type[BaseException]
    message: str


class Env:
    """The operands of the cases for one context. ``client_ptr(k, t)`` is the address a client
    table records for client ``k``, tensor ``t``: made up on the host, a real fp32 buffer of the
    segment's size on the GPU. ``names`` maps the address of every tensor made here to a name."""

    def __init__(self, ctx: FedAvgContext, client_ptr: Callable[[int, int], int], index: int) -> None:
        self.ctx = ctx
        self.device = ctx.device
        self.client_ptr = client_ptr
        self.index = index
        self.names: dict[int, str] = {}
        self._keep: list[torch.Tensor] = []

    def table(self, n: int = 2, holes: tuple = (), numels: tuple = NUMELS) -> ClientTable:
        """n fp32 clients; ``holes`` are the absent ``(client, tensor)`` entries."""
        tab = ClientTable(len(numels))
        for k in range(n):
            gone = [(k, t) in holes for t in range(len(numels))]
            tab.add_resident_client([0 if g else self.client_ptr(k, t) for t, g in enumerate(gone)],
                                    [0.0 if g else 1.0 for g in gone],
                                    [-1 if g else m for m, g in zip(numels, gone)], 4, self.index, [])
        return tab

    def flat(self, name: str, numel: int, dtype: torch.dtype = F64, device: Any = None,
             strided: bool = False) -> torch.Tensor:
        device = self.device if device is None else device
        z = torch.zeros(2 * numel, dtype=dtype, device=device)[::2] if strided else \
            torch.zeros(numel, dtype=dtype, device=device)
        if numel:
            self.names[z.data_ptr()] = name
        self._keep.append(z)
        return z

    def segs(self, name: str, dtype: torch.dtype = F64, numels: tuple = NUMELS, device: Any = None,
             strided: int | None = None) -> list[torch.Tensor]:
        """One tensor per segment, named ``name0``, ``name1``; ``strided``: that one is not contiguous."""
        return [self.flat(f"{name}{t}", m, dtype, device, strided == t) for t, m in enumerate(numels)]

    def sparse(self, name: str, numel: int, nnz: int, dtype: torch.dtype = F32, strided: bool = False) -> SparseDelta:
        return SparseDelta(self.flat(f"{name}.i", nnz, I32, strided=strided), self.flat(f"{name}.v", nnz, dtype),
                           (numel,))

    def rows(self, n: int = 2, dtype: torch.dtype = F32) -> list[list[SparseDelta]]:
        """Client k's sparse deltas ``d{k}0`` (2 entries of 5) and ``d{k}1`` (none of 3)."""
        return [[self.sparse(f"d{k}0", 5, 2, dtype), self.sparse(f"d{k}1", 3, 0, dtype)] for k in range(n)]


# -- the wrappers with every operand valid unless the case overrides it -----------------------------
def robust(e, table=None, in_dtype=F32, mode="median", trim=0.0, outs=None, out_dtype=F64):
    return e.ctx.robust_aggregate(e.table() if table is None else table, in_dtype, mode, trim,
                                  e.segs("out", out_dtype) if outs is None else outs, out_dtype)


def mam(e, table=None, in_dtype=F32, keep=1, outs=None, out_dtype=F64):
    return e.ctx.mean_around_median(e.table() if table is None else table, in_dtype, keep,
                                    e.segs("out", out_dtype) if outs is None else outs, out_dtype)


def pairwise(e, table=None, in_dtype=F32, out_dtype=None):
    return e.ctx.pairwise_sqdist(e.table() if table is None else table, in_dtype)


def sqdist(e, table=None, in_dtype=F32, point="point", out_dtype=None):
    return e.ctx.sqdist_to_point(e.table() if table is None else table, in_dtype,
                                 e.segs(point) if isinstance(point, str) else point)


def moments(e, table=None, in_dtype=F32, centre="centre", direction="direction", out_dtype=None):
    return e.ctx.moments_about_point(e.table() if table is None else table, in_dtype,
                                     e.segs(centre) if isinstance(centre, str) else centre,
                                     e.segs(direction) if isinstance(direction, str) else direction)


def fold(e, table=None, in_dtype=F32, coef=(1.0, 2.0), divisor=2.0, point=None, outs=None, out_dtype=F64):
    return e.ctx.fold_about_point(e.table() if table is None else table, in_dtype, coef, divisor,
                                  e.segs("point") if point is None else point,
                                  e.segs("out", out_dtype) if outs is None else outs, out_dtype)


def opt(e, table=None, in_dtype=F32, coef=(1.0, 2.0), divisor=2.0, point=None, m_in=None, v_in="v_in", m_out=None,
        v_out="v_out", outs=None, out_dtype=F64, mode="adam", lr=0.5, beta1=0.9, beta2=0.99, tau=0.001):
    return e.ctx.server_opt_step(
        e.table() if table is None else table, in_dtype, coef, divisor, e.segs("point") if point is None else point,
        e.segs("m_in") if m_in is None else m_in, e.segs(v_in) if isinstance(v_in, str) else v_in,
        e.segs("m_out") if m_out is None else m_out, e.segs(v_out) if isinstance(v_out, str) else v_out,
        e.segs("out", out_dtype) if outs is None else outs, out_dtype, mode=mode, lr=lr, beta1=beta1, beta2=beta2,
        tau=tau)


def sparse_fold(e, rows=None, weights=(1.0, 3.0), divisor=4.0, base=None, outs=None, out_dtype=F64):
    return e.ctx.sparse_aggregate_delta(e.rows() if rows is None else rows, weights, divisor,
                                        e.segs("base") if base is None else base,
                                        e.segs("out", out_dtype) if outs is None else outs, out_dtype)


def encode(e, codec=QSGD, tensors=None, records=None, sizes=(7, 17), dtype=F32, need=(48, 64), **kw):
    return e.ctx.quant_encode(codec, e.segs("x", dtype, sizes) if tensors is None else tensors,
                              e.segs("rec", U8, need) if records is None else records, **kw)


def decode(e, codec=QSGD, records=None, outs=None, outs64=None, sizes=(7, 17), dtype=F32, need=(48, 64)):
    return e.ctx.quant_decode(codec, e.segs("rec", U8, need) if records is None else records,
                              e.segs("out", dtype, sizes) if outs is None else outs, outs64)


def noise(e, tensors=None, outs=None, sizes=(7, 17), dtype=F32, **kw):
    return e.ctx.dp_noise(e.segs("x", dtype, sizes) if tensors is None else tensors,
                          e.segs("out", dtype, sizes) if outs is None else outs, 1.0, 0.5, **kw)


def topk(e, deltas=None, errors="err", keeps=(3, 0), indices=None, values=None, residuals=None, sizes=(7, 17),
         dtype=F32):
    return e.ctx.topk_sparsify(
        e.segs("delta", dtype, sizes) if deltas is None else deltas,
        e.segs(errors, dtype, sizes) if isinstance(errors, str) else errors, keeps,
        e.segs("idx", I32, tuple(keeps)[:2]) if indices is None else indices,
        e.segs("val", dtype, tuple(keeps)[:2]) if values is None else values,
        e.segs("res", dtype, sizes) if residuals is None else residuals)


def _fp64(what: str, t: int, device: str = "{device}") -> str:
    return f"{what} tensor {t}: contiguous fp64 of {NUMELS[t]} elements on {device} is required"


def _out(t: int, dtype: torch.dtype = F64) -> str:
    return f"output tensor {t}: contiguous {dtype} of {NUMELS[t]} elements on {{device}} is required"


def _flat(what: str, dtype: Any, size: str = "") -> str:
    return f"{what}: a contiguous {dtype} tensor{size} on {{device}} is required"


NOT_OUT = "aggregated output dtype must be float32 or float64, not torch.float16"
NOT_IN = "no HIP FedAvg kernel for input dtype torch.int32"
NOT_LAYOUT = "client table does not match the layout"
NOT_SIZED = ("client 0, tensor 0: 5 elements of 4 bytes on device {index}; the layout and input format need 5 of 2 "
             "bytes on device {index}")
DIVISOR = "the divisor must be a finite number > 0, not "
PING_PONG = "the step is not in-place, ping-pong two buffers"
SEED = "the seed is a uint64 and the draw a uint32"
IDS = "one stream id per tensor is required"
V, N, T_ = ValueError, NotImplementedError, TypeError

REFUSALS: list[Case] = []


def case(id: str, call: Callable[[Env], Any], exc: type[BaseException], message: str) -> None:
    REFUSALS.append(Case(id, call, exc, message))


# -- the per-element sort rules ---------------------------------------------------------------------
SORT_LIMIT = ("tensor 0 was sent by 65 clients: the register-resident sort holds at most 64 values per element")
case("robust-mode", lambda e: robust(e, mode="mean"), V,
     "robust aggregation mode must be one of ('trimmed_mean', 'median'), not 'mean'")
case("robust-trim-half", lambda e: robust(e, mode="trimmed_mean", trim=0.5), V,
     "trim must satisfy 0 <= trim < 0.5 (the kept range must not be empty), not 0.5")
case("robust-trim-negative", lambda e: robust(e, mode="trimmed_mean", trim=-0.1), V,
     "trim must satisfy 0 <= trim < 0.5 (the kept range must not be empty), not -0.1")
case("robust-trim-nan", lambda e: robust(e, mode="trimmed_mean", trim=NAN), V,
     "trim must satisfy 0 <= trim < 0.5 (the kept range must not be empty), not nan")
case("robust-empty", lambda e: robust(e, e.table(0)), V, "robust aggregation of no clients")
case("robust-65", lambda e: robust(e, e.table(65)), N, SORT_LIMIT)
case("robust-unsent", lambda e: robust(e, e.table(2, holes=((0, 1), (1, 1)))), V, "tensor 1 was sent by no client")
case("robust-records", lambda e: robust(e, in_dtype=QSGD_F32), N,
     "robust aggregation reads dense tensors: dequantise records first")
case("robust-in-dtype", lambda e: robust(e, in_dtype=I32), T_, NOT_IN)
case("robust-layout", lambda e: robust(e, e.table(2, numels=(5, 3, 1))), V, NOT_LAYOUT)
case("robust-sized", lambda e: robust(e, in_dtype=F16), V, NOT_SIZED)
case("robust-outs-count", lambda e: robust(e, outs=e.segs("out")[:1]), V, "one output tensor per segment is required")
case("robust-outs-size", lambda e: robust(e, outs=e.segs("out", F64, (5, 4))), V,
     "output tensors must be contiguous, on the context device, of the layout size")
case("robust-out-dtype", lambda e: robust(e, out_dtype=F16), T_, NOT_OUT)
case("robust-mode-empty-first", lambda e: robust(e, e.table(0), mode="mean"), V,
     "robust aggregation mode must be one of ('trimmed_mean', 'median'), not 'mean'")
case("robust-65-records-first", lambda e: robust(e, e.table(65), in_dtype=QSGD_F32), N, SORT_LIMIT)
case("robust-records-layout-first", lambda e: robust(e, e.table(2, numels=(5,)), in_dtype=QSGD_F32), N,
     "robust aggregation reads dense tensors: dequantise records first")
case("robust-sized-outs-first", lambda e: robust(e, in_dtype=F16, outs=[]), V, NOT_SIZED)

case("mam-keep-count", lambda e: mam(e, keep=[1, 1, 1]), V, "keep has 3 entries for 2 tensors")
case("mam-empty", lambda e: mam(e, e.table(0)), V, "robust aggregation of no clients")
case("mam-65", lambda e: mam(e, e.table(65)), N, SORT_LIMIT)
case("mam-unsent", lambda e: mam(e, e.table(2, holes=((0, 0), (1, 0)))), V, "tensor 0 was sent by no client")
case("mam-keep-zero", lambda e: mam(e, keep=0), V, "tensor 0: keep 0 is not in [1, 2]")
case("mam-keep-over", lambda e: mam(e, e.table(2, holes=((1, 1),)), keep=[2, 2]), V,
     "tensor 1: keep 2 is not in [1, 1]")
case("mam-records", lambda e: mam(e, in_dtype=QSGD_F32), N,
     "the mean around the median reads dense tensors: dequantise records first")
case("mam-in-dtype", lambda e: mam(e, in_dtype=I32), T_, NOT_IN)
case("mam-layout", lambda e: mam(e, e.table(2, numels=(5, 3, 1)), keep=[1, 1, 1]), V, NOT_LAYOUT)
case("mam-sized", lambda e: mam(e, in_dtype=F16), V, NOT_SIZED)
case("mam-outs-count", lambda e: mam(e, outs=[]), V, "one output tensor per segment is required")
case("mam-out-dtype", lambda e: mam(e, out_dtype=F16), T_, NOT_OUT)
case("mam-keep-count-empty-first", lambda e: mam(e, e.table(0), keep=[1]), V, "keep has 1 entries for 2 tensors")
case("mam-65-keep-first", lambda e: mam(e, e.table(65), keep=0), N, SORT_LIMIT)
case("mam-keep-records-first", lambda e: mam(e, keep=3, in_dtype=QSGD_F32), V, "tensor 0: keep 3 is not in [1, 2]")

# -- the five whole-update wrappers: one prologue, five wordings ------------------------------------
WHOLE = (
    ("pairwise", pairwise, "pairwise distances", "take", "read", KRUM_MAX, "distances compare"),
    ("sqdist", sqdist, "distances to a point", "take", "read", POINT_MAX, "distances compare"),
    ("moments", moments, "moments about a point", "take", "read", POINT_MAX, "moments compare"),
    ("fold", fold, "the fold about a point", "takes", "reads", POINT_MAX, "the fold about a point takes"),
    ("opt", opt, "the server optimiser step", "takes", "reads", POINT_MAX, "the server optimiser step takes"),
)
for name, fn, what, take, read, limit, whole in WHOLE:
    over, records = f"{limit + 1} clients: {what} {take} at most {limit}", f"{what} {read} dense tensors: " \
        "dequantise records first"
    case(f"{name}-empty", lambda e, fn=fn: fn(e, e.table(0)), V, f"{what} of no clients")
    case(f"{name}-over", lambda e, fn=fn, limit=limit: fn(e, e.table(limit + 1)), N, over)
    case(f"{name}-records", lambda e, fn=fn: fn(e, in_dtype=QSGD_F32), N, records)
    case(f"{name}-in-dtype", lambda e, fn=fn: fn(e, in_dtype=I32), T_, NOT_IN)
    case(f"{name}-layout", lambda e, fn=fn: fn(e, e.table(2, numels=(5, 3, 1))), V, NOT_LAYOUT)
    case(f"{name}-sized", lambda e, fn=fn: fn(e, in_dtype=F16), V, NOT_SIZED)
    case(f"{name}-hole", lambda e, fn=fn: fn(e, e.table(2, holes=((1, 1),))), V,
         f"client 1 lacks tensor 1: {whole} whole updates")
    case(f"{name}-empty-records-first", lambda e, fn=fn: fn(e, e.table(0), in_dtype=QSGD_F32), V,
         f"{what} of no clients")
    case(f"{name}-over-records-first", lambda e, fn=fn, limit=limit: fn(e, e.table(limit + 1), in_dtype=QSGD_F32), N,
         over)
    case(f"{name}-records-layout-first", lambda e, fn=fn: fn(e, e.table(2, numels=(5,)), in_dtype=QSGD_F32), N,
         records)
    case(f"{name}-sized-hole-first", lambda e, fn=fn: fn(e, e.table(2, holes=((0, 1),)), in_dtype=F16), V, NOT_SIZED)
    if name in ("fold", "opt"):
        case(f"{name}-out-dtype", lambda e, fn=fn: fn(e, out_dtype=F16), T_, NOT_OUT)
        case(f"{name}-records-out-dtype-first", lambda e, fn=fn: fn(e, in_dtype=QSGD_F32, out_dtype=F16), N, records)
        case(f"{name}-out-dtype-layout-first", lambda e, fn=fn: fn(e, e.table(2, numels=(5,)), out_dtype=F16), T_,
             NOT_OUT)
        case(f"{name}-coef-count", lambda e, fn=fn: fn(e, coef=(1.0, 2.0, 3.0)), V,
             "one coefficient per client is required: 3 for 2 clients")
        case(f"{name}-coef-inf", lambda e, fn=fn: fn(e, coef=(1.0, INF)), V, "the coefficients must be finite")
        case(f"{name}-coef-nan", lambda e, fn=fn: fn(e, coef=(NAN, 1.0)), V, "the coefficients must be finite")
        for bad in (0.0, -1.0, INF, NAN):
            case(f"{name}-divisor-{bad}", lambda e, fn=fn, bad=bad: fn(e, divisor=bad), V, DIVISOR + str(bad))
        case(f"{name}-hole-coef-first", lambda e, fn=fn: fn(e, e.table(2, holes=((0, 0),)), coef=()), V,
             f"client 0 lacks tensor 0: {whole} whole updates")
        case(f"{name}-coef-divisor-first", lambda e, fn=fn: fn(e, coef=(1.0, INF), divisor=0.0), V,
             "the coefficients must be finite")
        case(f"{name}-out-size", lambda e, fn=fn: fn(e, outs=e.segs("out", F64, (5, 4))), V, _out(1))
        case(f"{name}-out-dtype-mismatch", lambda e, fn=fn: fn(e, outs=e.segs("out", F32)), V, _out(0))
        case(f"{name}-out-f32-size", lambda e, fn=fn: fn(e, outs=e.segs("out", F32, (4, 3)), out_dtype=F32), V,
             _out(0, F32))
        case(f"{name}-out-strided", lambda e, fn=fn: fn(e, outs=e.segs("out", strided=1)), V, _out(1))
        case(f"{name}-point-size", lambda e, fn=fn: fn(e, point=e.segs("point", F64, (6, 3))), V, _fp64("point", 0))
        case(f"{name}-point-dtype", lambda e, fn=fn: fn(e, point=e.segs("point", F32)), V, _fp64("point", 0))
        case(f"{name}-point-strided", lambda e, fn=fn: fn(e, point=e.segs("point", strided=1)), V, _fp64("point", 1))

        def aliased(e, fn=fn, t=1):
            point, outs = e.segs("point"), e.segs("out")
            outs[t] = point[t]
            return fn(e, point=point, outs=outs)

        def aliased_f32(e, fn=fn):
            point = e.segs("point")
            return fn(e, point=point, outs=[z.view(F32)[: z.numel()] for z in point], out_dtype=F32)

        case(f"{name}-out-is-point", aliased, V, f"output tensor 1 is its point: {PING_PONG}")
        case(f"{name}-out-f32-is-point", aliased_f32, V, f"output tensor 0 is its point: {PING_PONG}")

case("sqdist-point-count", lambda e: sqdist(e, point=e.segs("point")[:1]), V, "one point tensor per segment is required")
case("sqdist-point-size", lambda e: sqdist(e, point=e.segs("point", F64, (5, 2))), V, _fp64("point", 1))
case("sqdist-point-dtype", lambda e: sqdist(e, point=e.segs("point", F32)), V, _fp64("point", 0))
case("sqdist-point-strided", lambda e: sqdist(e, point=e.segs("point", strided=0)), V, _fp64("point", 0))
case("sqdist-hole-point-first", lambda e: sqdist(e, e.table(2, holes=((0, 0),)), point=[]), V,
     "client 0 lacks tensor 0: distances compare whole updates")

case("moments-no-direction", lambda e: moments(e, direction=None), V, "the direction is required")
case("moments-centre-count", lambda e: moments(e, centre=[]), V, "one centre tensor per segment is required")
case("moments-direction-count", lambda e: moments(e, direction=e.segs("direction")[:1]), V,
     "one direction tensor per segment is required")
case("moments-centre-size", lambda e: moments(e, centre=e.segs("centre", F64, (5, 2))), V, _fp64("centre", 1))
case("moments-centre-dtype", lambda e: moments(e, centre=e.segs("centre", F16)), V, _fp64("centre", 0))
case("moments-direction-size", lambda e: moments(e, direction=e.segs("direction", F64, (4, 3))), V,
     _fp64("direction", 0))
case("moments-direction-strided", lambda e: moments(e, centre=None, direction=e.segs("direction", strided=1)), V,
     _fp64("direction", 1))
case("moments-hole-direction-first", lambda e: moments(e, e.table(2, holes=((1, 0),)), direction=None), V,
     "client 1 lacks tensor 0: moments compare whole updates")
case("moments-direction-centre-first", lambda e: moments(e, centre=[], direction=None), V, "the direction is required")
case("moments-centre-direction-first", lambda e: moments(e, centre=e.segs("centre", F64, (5, 2)), direction=[]), V,
     _fp64("centre", 1))

case("fold-count", lambda e: fold(e, point=e.segs("point")[:1]), V,
     "one point tensor and one output tensor per segment are required")
case("fold-outs-count", lambda e: fold(e, outs=[]), V, "one point tensor and one output tensor per segment are required")
case("fold-divisor-count-first", lambda e: fold(e, divisor=0.0, outs=[]), V, DIVISOR + "0.0")
case("fold-out0-point1-first", lambda e: fold(e, point=e.segs("point", F64, (5, 2)), outs=e.segs("out", F64, (4, 3))), V,
     _out(0))
case("fold-point0-out0-first", lambda e: fold(e, point=e.segs("point", F64, (4, 3)), outs=e.segs("out", F64, (4, 3))), V,
     _fp64("point", 0))

# -- the server optimiser step ---------------------------------------------------------------------
case("opt-mode", lambda e: opt(e, mode="sgd"), V, "mode must be one of ('avgm', 'adagrad', 'yogi', 'adam'), not 'sgd'")
case("opt-lr-zero", lambda e: opt(e, lr=0.0), V, "the learning rate must be a finite number > 0, not 0.0")
case("opt-lr-inf", lambda e: opt(e, lr=INF), V, "the learning rate must be a finite number > 0, not inf")
case("opt-beta1", lambda e: opt(e, beta1=1.0), V, "beta1 must lie in [0, 1), not 1.0")
case("opt-beta2", lambda e: opt(e, beta2=-0.1), V, "beta2 must lie in [0, 1), not -0.1")
case("opt-tau", lambda e: opt(e, tau=0.0), V, "tau must be a finite number > 0, not 0.0")
case("opt-tau-nan-yogi", lambda e: opt(e, mode="yogi", tau=NAN), V, "tau must be a finite number > 0, not nan")
case("opt-out-dtype-mode-first", lambda e: opt(e, out_dtype=F16, mode="sgd"), T_, NOT_OUT)
case("opt-mode-layout-first", lambda e: opt(e, e.table(2, numels=(5,)), mode="sgd"), V,
     "mode must be one of ('avgm', 'adagrad', 'yogi', 'adam'), not 'sgd'")
case("opt-lr-hole-first", lambda e: opt(e, e.table(2, holes=((0, 0),)), lr=-1.0), V,
     "the learning rate must be a finite number > 0, not -1.0")
case("opt-no-v-in", lambda e: opt(e, v_in=None), V, "mode 'adam' needs second-moment tensors")
case("opt-no-v-out", lambda e: opt(e, v_out=None, mode="adagrad"), V, "mode 'adagrad' needs second-moment tensors")
case("opt-divisor-no-v-first", lambda e: opt(e, divisor=NAN, v_in=None), V, DIVISOR + "nan")
PER_SEGMENT = "one point, moment and output tensor per segment are required"
case("opt-point-count", lambda e: opt(e, point=[]), V, PER_SEGMENT)
case("opt-m-in-count", lambda e: opt(e, m_in=e.segs("m_in")[:1]), V, PER_SEGMENT)
case("opt-v-out-count", lambda e: opt(e, v_out=e.segs("v_out")[:1]), V, PER_SEGMENT)
case("opt-outs-count", lambda e: opt(e, outs=[]), V, PER_SEGMENT)
case("opt-no-v-count-first", lambda e: opt(e, v_in=None, outs=[]), V, "mode 'adam' needs second-moment tensors")
case("opt-m-in-size", lambda e: opt(e, m_in=e.segs("m_in", F64, (5, 2))), V, _fp64("first-moment input", 1))
case("opt-m-out-dtype", lambda e: opt(e, m_out=e.segs("m_out", F32)), V, _fp64("first-moment output", 0))
case("opt-v-in-strided", lambda e: opt(e, v_in=e.segs("v_in", strided=1)), V, _fp64("second-moment input", 1))
case("opt-v-out-size", lambda e: opt(e, v_out=e.segs("v_out", F64, (6, 3))), V, _fp64("second-moment output", 0))
case("opt-point1-m-in0-first", lambda e: opt(e, point=e.segs("point", F64, (5, 2)), m_in=e.segs("m_in", F64, (4, 3))), V,
     _fp64("point", 1))
case("opt-m-out1-out0-first", lambda e: opt(e, m_out=e.segs("m_out", F64, (5, 2)), outs=e.segs("out", F64, (4, 3))), V,
     _fp64("first-moment output", 1))


def _opt_moment_alias(which: str, mode: str = "adam") -> Callable[[Env], Any]:
    def call(e):
        m, v = e.segs("m"), e.segs("v")
        return opt(e, m_in=m, m_out=[e.flat("m_out0", 5), m[1]] if which == "m" else None, v_in=v,
                   v_out=[v[0], e.flat("v_out1", 3)] if which == "v" else "v_out", mode=mode)
    return call


def _opt_point_and_moment(e):
    point, m = e.segs("point"), e.segs("m")
    return opt(e, point=point, outs=[e.flat("out0", 5), point[1]], m_in=m, m_out=[m[0], e.flat("m_out1", 3)])


case("opt-m-out-is-m-in", _opt_moment_alias("m"), V, f"moment tensor 1: {PING_PONG}")
case("opt-v-out-is-v-in", _opt_moment_alias("v"), V, f"moment tensor 0: {PING_PONG}")
case("opt-moment0-point1-first", _opt_point_and_moment, V, f"moment tensor 0: {PING_PONG}")

# -- the sparse fold -------------------------------------------------------------------------------
SPARSE_SIZED = "client 1, tensor 0: a contiguous sparse delta of 5 elements on {device} is required"


def _sparse_table_cases(prefix: str, run: Callable[[Env, Any], Any]) -> None:
    case(f"{prefix}-empty", lambda e: run(e, []), V, "the sparse fold of no clients")
    case(f"{prefix}-over", lambda e: run(e, e.rows(1) * (POINT_MAX + 1)), N,
         f"{POINT_MAX + 1} clients: the sparse fold takes at most {POINT_MAX}")
    case(f"{prefix}-row-count", lambda e: run(e, [e.rows(1)[0][:1]]), V,
         "client 0: one sparse delta per segment is required")
    case(f"{prefix}-not-sparse", lambda e: run(e, [[e.sparse("d", 5, 1), e.flat("x", 3)]]), T_,
         "client 0, tensor 1: a SparseDelta is required, not Tensor")
    case(f"{prefix}-numel", lambda e: run(e, e.rows(1) + [[e.sparse("a", 4, 1), e.sparse("b", 3, 1)]]), V, SPARSE_SIZED)
    case(f"{prefix}-strided", lambda e: run(e, e.rows(1) + [[e.sparse("a", 5, 2, strided=True), e.sparse("b", 3, 1)]]),
         V, SPARSE_SIZED)
    case(f"{prefix}-dtypes", lambda e: run(e, e.rows(1) + e.rows(1, F16)), V,
         "the sparse deltas of one call share one value dtype, not ['torch.float16', 'torch.float32']")
    case(f"{prefix}-over-row-count-first", lambda e: run(e, [[]] * (POINT_MAX + 1)), N,
         f"{POINT_MAX + 1} clients: the sparse fold takes at most {POINT_MAX}")


_sparse_table_cases("sparse-table", lambda e, rows: SparseTable(rows, LAYOUT, e.device))
_sparse_table_cases("sparse", lambda e, rows: sparse_fold(e, rows, weights=[1.0] * len(rows)))
case("sparse-out-dtype", lambda e: sparse_fold(e, out_dtype=F16), T_, NOT_OUT)
case("sparse-out-dtype-empty-first", lambda e: sparse_fold(e, [], out_dtype=F16), T_, NOT_OUT)
case("sparse-other-layout", lambda e: sparse_fold(e, SparseTable(
    [[e.sparse("a", 5, 1), e.sparse("b", 4, 1)]], OTHER_LAYOUT, e.device), weights=[1.0]), V,
    "the sparse table was built for another layout or device")
case("sparse-weight-count", lambda e: sparse_fold(e, weights=(1.0,)), V,
     "one weight per client is required: 1 for 2 clients")
case("sparse-weight-inf", lambda e: sparse_fold(e, weights=(1.0, -INF)), V, "the weights must be finite")
case("sparse-weight-nan", lambda e: sparse_fold(e, weights=(NAN, 1.0)), V, "the weights must be finite")
for bad in (0.0, -1.0, INF, NAN):
    case(f"sparse-divisor-{bad}", lambda e, bad=bad: sparse_fold(e, divisor=bad), V, DIVISOR + str(bad))
case("sparse-empty-weights-first", lambda e: sparse_fold(e, [], weights=(INF,)), V, "the sparse fold of no clients")
case("sparse-weights-divisor-first", lambda e: sparse_fold(e, weights=(1.0, INF), divisor=0.0), V,
     "the weights must be finite")
case("sparse-divisor-count-first", lambda e: sparse_fold(e, divisor=-2.0, outs=[]), V, DIVISOR + "-2.0")
case("sparse-base-count", lambda e: sparse_fold(e, base=[]), V,
     "one base tensor and one output tensor per segment are required")
case("sparse-outs-count", lambda e: sparse_fold(e, outs=e.segs("out")[:1]), V,
     "one base tensor and one output tensor per segment are required")
case("sparse-base-size", lambda e: sparse_fold(e, base=e.segs("base", F64, (5, 4))), V, _fp64("base", 1))
case("sparse-base-dtype", lambda e: sparse_fold(e, base=e.segs("base", F32)), V, _fp64("base", 0))
case("sparse-base-strided", lambda e: sparse_fold(e, base=e.segs("base", strided=0)), V, _fp64("base", 0))
case("sparse-out-size", lambda e: sparse_fold(e, outs=e.segs("out", F64, (5, 2))), V, _out(1))
case("sparse-out-dtype-mismatch", lambda e: sparse_fold(e, outs=e.segs("out", F64), out_dtype=F32), V, _out(0, F32))
case("sparse-out0-base1-first", lambda e: sparse_fold(e, base=e.segs("base", F64, (5, 2)),
                                                      outs=e.segs("out", F64, (4, 3))), V, _out(0))


def _sparse_aliased(e):
    base = e.segs("base")
    return sparse_fold(e, base=base, outs=[base[0], e.flat("out1", 3)])


case("sparse-out-is-base", _sparse_aliased, V, "output tensor 0 is its base: the sparse fold is not in-place")

# -- the layout-free calls: tensors of 0, 7 and 17 elements -----------------------------------------
# record sizes: QSGD 16 + align16(n) + align16(ceil(n / 8)), NNADQ 32 + align16(n)
QSGD_NEED = {0: 16, 7: 48, 17: 64}
NNADQ_NEED = {0: 32, 7: 48, 17: 64}


def _record(t: int, need: int) -> str:
    return f"record {t}: a contiguous uint8 tensor of {need} bytes on {{device}} is required"


case("encode-codec", lambda e: encode(e, codec=_native.F32), V, "codec 0 is not a record format")
case("encode-none", lambda e: encode(e, tensors=[], records=[]), V,
     "one record per tensor and at least one tensor are required")
case("encode-record-count", lambda e: encode(e, records=e.segs("rec", U8, (48,))), V,
     "one record per tensor and at least one tensor are required")
case("encode-seed-negative", lambda e: encode(e, seed=-1), V, SEED)
case("encode-seed-over", lambda e: encode(e, seed=1 << 64), V, SEED)
case("encode-draw-over", lambda e: encode(e, draw=1 << 32), V, SEED)
case("encode-ids", lambda e: encode(e, tensor_ids=[4]), V, IDS)
case("encode-dtype", lambda e: encode(e, dtype=F64), V, _flat("tensor 0", F32))
case("encode-dtype-f64", lambda e: encode(e, codec=NNADQ64), V, _flat("tensor 0", F64))
case("encode-strided", lambda e: encode(e, tensors=[e.flat("x0", 7, F32), e.flat("x1", 17, F32, strided=True)]), V,
     _flat("tensor 1", F32))
for n, scheme, codec, table in [(n, s, c, t) for s, c, t in (("qsgd", QSGD, QSGD_NEED), ("nnadq", NNADQ, NNADQ_NEED))
                                for n in (0, 7, 17)]:
    case(f"encode-{scheme}-record-{n}", lambda e, n=n, codec=codec, table=table: encode(
        e, codec, sizes=(7, n), need=(table[7], table[n] + 16)), V, _record(1, table[n]))
    case(f"decode-{scheme}-record-{n}", lambda e, n=n, codec=codec, table=table: decode(
        e, codec, sizes=(n, 7), need=(table[n] - 16, table[7])), V, _record(0, table[n]))
case("encode-record-dtype", lambda e: encode(e, records=e.segs("rec", torch.int8, (48, 64))), V, _record(0, 48))
case("encode-record-strided", lambda e: encode(e, records=e.segs("rec", U8, (48, 64), strided=1)), V, _record(1, 64))
case("encode-codec-none-first", lambda e: encode(e, codec=8, tensors=[], records=[]), V,
     "codec 8 is not a record format")
case("encode-count-seed-first", lambda e: encode(e, records=[], seed=-1), V,
     "one record per tensor and at least one tensor are required")
case("encode-seed-ids-first", lambda e: encode(e, draw=-1, tensor_ids=[]), V, SEED)
case("encode-ids-dtype-first", lambda e: encode(e, dtype=F64, tensor_ids=[1, 2, 3]), V, IDS)
case("encode-tensor0-record0-first", lambda e: encode(e, dtype=F16, need=(47, 64)), V, _flat("tensor 0", F32))
case("encode-record0-tensor1-first", lambda e: encode(
    e, tensors=[e.flat("x0", 7, F32), e.flat("x1", 17, F64)], need=(47, 64)), V, _record(0, 48))

FP64_COPY = "the fp64 copy is offered for the fp32 codecs: an fp64 codec's output is fp64"
case("decode-codec", lambda e: decode(e, codec=_native.F64), V, "codec 3 is not a record format")
case("decode-none", lambda e: decode(e, records=[], outs=[]), V,
     "one output per record and at least one record are required")
case("decode-outs-count", lambda e: decode(e, outs=e.segs("out", F32, (7,))), V,
     "one output per record and at least one record are required")
case("decode-outs64-count", lambda e: decode(e, outs64=e.segs("wide", F64, (7,))), V,
     "one output per record and at least one record are required")
case("decode-outs64-f64", lambda e: decode(e, QSGD64, dtype=F64, outs64=e.segs("wide", F64, (7, 17))), V, FP64_COPY)
case("decode-out-dtype", lambda e: decode(e, dtype=F64), V, _flat("output 0", F32))
case("decode-out-strided", lambda e: decode(e, NNADQ64, outs=[e.flat("out0", 7, F64), e.flat("out1", 17, F64, strided=True)]),
     V, _flat("output 1", F64))
case("decode-record-dtype", lambda e: decode(e, records=e.segs("rec", torch.int8, (48, 64))), V, _record(0, 48))
case("decode-outs64-size", lambda e: decode(e, outs64=e.segs("wide", F64, (7, 16))), V,
     _flat("fp64 output 1", F64, " of 17 elements"))
case("decode-outs64-dtype", lambda e: decode(e, outs64=e.segs("wide", F32, (7, 17))), V,
     _flat("fp64 output 0", F64, " of 7 elements"))
case("decode-codec-none-first", lambda e: decode(e, codec=-1, records=[], outs=[]), V,
     "codec -1 is not a record format")
case("decode-count-f64-first", lambda e: decode(e, QSGD64, dtype=F64, outs64=[]), V,
     "one output per record and at least one record are required")
case("decode-out0-record0-first", lambda e: decode(e, dtype=F64, need=(47, 64)), V, _flat("output 0", F32))
case("decode-record0-outs64-first", lambda e: decode(e, need=(47, 64), outs64=e.segs("wide", F32, (7, 17))), V,
     _record(0, 48))
case("decode-outs64-0-out1-first", lambda e: decode(
    e, outs=[e.flat("out0", 7, F32), e.flat("out1", 17, F64)], outs64=e.segs("wide", F64, (6, 17))), V,
    _flat("fp64 output 0", F64, " of 7 elements"))

NOISE_DTYPE = "the clip-and-noise pass takes fp32, fp16, bf16 or fp64 tensors, not torch.int32"
case("noise-none", lambda e: noise(e, tensors=[], outs=[]), V,
     "one output per tensor and at least one tensor are required")
case("noise-outs-count", lambda e: noise(e, outs=e.segs("out", F32, (7,))), V,
     "one output per tensor and at least one tensor are required")
case("noise-seed", lambda e: noise(e, seed=1 << 64), V, SEED)
case("noise-draw", lambda e: noise(e, draw=-1), V, SEED)
case("noise-ids", lambda e: noise(e, tensor_ids=[[0, 1]]), V, IDS)
case("noise-dtype", lambda e: noise(e, dtype=I32), T_, NOISE_DTYPE)
case("noise-mixed", lambda e: noise(e, tensors=[e.flat("x0", 7, F16), e.flat("x1", 17, F32)], dtype=F16), V,
     _flat("tensor 1", F16))
case("noise-strided", lambda e: noise(e, tensors=[e.flat("x0", 7, F32, strided=True), e.flat("x1", 17, F32)]), V,
     _flat("tensor 0", F32))
case("noise-out-size", lambda e: noise(e, outs=e.segs("out", F32, (7, 0)), sizes=(7, 17)), V,
     _flat("output 1", F32, " of 17 elements"))
case("noise-out-size-empty", lambda e: noise(e, outs=e.segs("out", F32, (7, 7)), sizes=(0, 7)), V,
     _flat("output 0", F32, " of 0 elements"))
case("noise-out-dtype", lambda e: noise(e, outs=e.segs("out", F64, (7, 17))), V,
     _flat("output 0", F32, " of 7 elements"))
case("noise-count-seed-first", lambda e: noise(e, outs=[], seed=-1), V,
     "one output per tensor and at least one tensor are required")
case("noise-seed-ids-first", lambda e: noise(e, seed=-1, tensor_ids=[0]), V, SEED)
case("noise-ids-dtype-first", lambda e: noise(e, dtype=I32, tensor_ids=[0]), V, IDS)
case("noise-dtype-outs-first", lambda e: noise(e, tensors=e.segs("x", I32, (7, 17)), outs=e.segs("out", F32, (7, 17))),
     T_, NOISE_DTYPE)
case("noise-out0-tensor1-first", lambda e: noise(e, tensors=[e.flat("x0", 7, F32), e.flat("x1", 17, F64)],
                                                 outs=e.segs("out", F32, (6, 17))), V,
     _flat("output 0", F32, " of 7 elements"))

TOPK_COUNT = "one keep count, index, value and residual tensor per delta and at least one delta are required"
TOPK_DTYPE = "the top-k step takes fp32, fp16, bf16 or fp64 tensors, not torch.int32"
case("topk-none", lambda e: topk(e, deltas=[], errors=None, keeps=(), indices=[], values=[], residuals=[]), V, TOPK_COUNT)
case("topk-keeps-count", lambda e: topk(e, keeps=(3,), indices=e.segs("idx", I32, (3, 0))), V, TOPK_COUNT)
case("topk-indices-count", lambda e: topk(e, indices=[]), V, TOPK_COUNT)
case("topk-values-count", lambda e: topk(e, values=e.segs("val", F32, (3,))), V, TOPK_COUNT)
case("topk-residuals-count", lambda e: topk(e, residuals=[]), V, TOPK_COUNT)
case("topk-errors-count", lambda e: topk(e, errors=[None]), V, TOPK_COUNT)
case("topk-dtype", lambda e: topk(e, dtype=I32), T_, TOPK_DTYPE)
case("topk-mixed", lambda e: topk(e, deltas=[e.flat("delta0", 7, F32), e.flat("delta1", 17, F16)]), V,
     _flat("delta 1", F32))
case("topk-strided", lambda e: topk(e, deltas=[e.flat("delta0", 7, F32, strided=True), e.flat("delta1", 17, F32)]), V,
     _flat("delta 0", F32))
case("topk-keep-over", lambda e: topk(e, keeps=(8, 0)), V, "delta 0: keeps 8 of 7 elements")
case("topk-keep-negative", lambda e: topk(e, keeps=(3, -1), indices=e.segs("idx", I32, (3, 0)),
                                          values=e.segs("val", F32, (3, 0))), V, "delta 1: keeps -1 of 17 elements")
case("topk-error-size", lambda e: topk(e, errors=e.segs("err", F32, (6, 17))), V,
     _flat("error 0", F32, " of 7 elements"))
case("topk-error-dtype", lambda e: topk(e, errors=[None, e.flat("err1", 17, F64)]), V,
     _flat("error 1", F32, " of 17 elements"))
case("topk-index-dtype", lambda e: topk(e, indices=e.segs("idx", torch.int64, (3, 0))), V,
     _flat("index 0", I32, " of 3 elements"))
case("topk-index-size", lambda e: topk(e, indices=e.segs("idx", I32, (3, 1))), V,
     _flat("index 1", I32, " of 0 elements"))
case("topk-value-size", lambda e: topk(e, values=e.segs("val", F32, (2, 0))), V,
     _flat("value 0", F32, " of 3 elements"))
case("topk-value-dtype", lambda e: topk(e, dtype=F16, values=e.segs("val", F32, (3, 0))), V,
     _flat("value 0", F16, " of 3 elements"))
case("topk-residual-size", lambda e: topk(e, residuals=e.segs("res", F32, (7, 16))), V,
     _flat("residual 1", F32, " of 17 elements"))
case("topk-residual-strided", lambda e: topk(e, residuals=e.segs("res", F32, (7, 17), strided=0)), V,
     _flat("residual 0", F32, " of 7 elements"))
case("topk-count-dtype-first", lambda e: topk(e, dtype=I32, residuals=[]), V, TOPK_COUNT)
case("topk-dtype-keep-first", lambda e: topk(e, dtype=I32, keeps=(8, 0)), T_, TOPK_DTYPE)
case("topk-delta-keep-first", lambda e: topk(e, deltas=[e.flat("delta0", 7, F32, strided=True),
                                                        e.flat("delta1", 17, F32)], keeps=(8, 0)), V,
     _flat("delta 0", F32))
case("topk-keep-error-first", lambda e: topk(e, keeps=(8, 0), errors=e.segs("err", F32, (6, 17))), V,
     "delta 0: keeps 8 of 7 elements")
case("topk-error-index-first", lambda e: topk(e, errors=e.segs("err", F32, (6, 17)), indices=e.segs("idx", I32, (2, 0))),
     V, _flat("error 0", F32, " of 7 elements"))
case("topk-residual0-delta1-first", lambda e: topk(
    e, deltas=[e.flat("delta0", 7, F32), e.flat("delta1", 17, F32, strided=True)],
    residuals=e.segs("res", F32, (6, 17))), V, _flat("residual 0", F32, " of 7 elements"))

assert len({c.id for c in REFUSALS}) == len(REFUSALS), "case ids are unique"


# -- where a device tensor is required and a host tensor is given (a real context only) -------------
CPU = torch.device("cpu")
HOST_TENSOR_REFUSALS: list[Case] = [
    Case("sqdist-point-on-host", lambda e: sqdist(e, point=e.segs("point", device=CPU)), V, _fp64("point", 0)),
    Case("moments-direction-on-host", lambda e: moments(e, direction=e.segs("direction", device=CPU)), V,
         _fp64("direction", 0)),
    Case("fold-point-on-host", lambda e: fold(e, point=e.segs("point", device=CPU)), V, _fp64("point", 0)),
    Case("fold-out-on-host", lambda e: fold(e, outs=e.segs("out", device=CPU)), V, _out(0)),
    Case("opt-point-on-host", lambda e: opt(e, point=e.segs("point", device=CPU)), V, _fp64("point", 0)),
    Case("opt-m-out-on-host", lambda e: opt(e, m_out=e.segs("m_out", device=CPU)), V, _fp64("first-moment output", 0)),
    Case("opt-out-on-host", lambda e: opt(e, outs=e.segs("out", device=CPU)), V, _out(0)),
    Case("robust-out-on-host", lambda e: robust(e, outs=e.segs("out", device=CPU)), V,
         "output tensors must be contiguous, on the context device, of the layout size"),
    Case("sparse-base-on-host", lambda e: sparse_fold(e, base=e.segs("base", device=CPU)), V, _fp64("base", 0)),
    Case("sparse-out-on-host", lambda e: sparse_fold(e, outs=e.segs("out", device=CPU)), V, _out(0)),
    Case("sparse-delta-on-host", lambda e: sparse_fold(e, e.rows(1) + [[
        SparseDelta(torch.zeros(2, dtype=I32), torch.zeros(2), (5,)), e.sparse("b", 3, 0)]]), V, SPARSE_SIZED),
    Case("encode-tensor-on-host", lambda e: encode(e, tensors=e.segs("x", F32, (7, 17), device=CPU)), V,
         _flat("tensor 0", F32)),
    Case("encode-record-on-host", lambda e: encode(e, records=e.segs("rec", U8, (48, 64), device=CPU)), V,
         _record(0, 48)),
    Case("decode-record-on-host", lambda e: decode(e, records=e.segs("rec", U8, (48, 64), device=CPU)), V,
         _record(0, 48)),
    Case("decode-out-on-host", lambda e: decode(e, outs=e.segs("out", F32, (7, 17), device=CPU)), V,
         _flat("output 0", F32)),
    Case("decode-outs64-on-host", lambda e: decode(e, outs64=e.segs("wide", F64, (7, 17), device=CPU)), V,
         _flat("fp64 output 0", F64, " of 7 elements")),
    Case("noise-tensor-on-host", lambda e: noise(e, tensors=e.segs("x", F32, (7, 17), device=CPU)), V,
         _flat("tensor 0", F32)),
    Case("noise-out-on-host", lambda e: noise(e, outs=e.segs("out", F32, (7, 17), device=CPU)), V,
         _flat("output 0", F32, " of 7 elements")),
    Case("topk-delta-on-host", lambda e: topk(e, deltas=e.segs("delta", F32, (7, 17), device=CPU)), V,
         _flat("delta 0", F32)),
    Case("topk-index-on-host", lambda e: topk(e, indices=e.segs("idx", I32, (3, 0), device=CPU)), V,
         _flat("index 0", I32, " of 3 elements")),
    Case("topk-residual-on-host", lambda e: topk(e, residuals=e.segs("res", F32, (7, 17), device=CPU)), V,
         _flat("residual 0", F32, " of 7 elements")),
]


def check_refusal(env: Env, c: Case) -> None:
    """``c.call`` raises exactly ``c.exc`` (not a subclass) with exactly ``c.message``."""
    try:
        c.call(env)
    except Exception as err:  # noqa: BLE001 - the type is compared below
        assert type(err) is c.exc, f"{c.id}: {type(err).__name__}: {err}"
        assert str(err) == c.message.format(device=env.device, index=env.index), c.id
    else:
        raise AssertionError(f"{c.id}: accepted")
