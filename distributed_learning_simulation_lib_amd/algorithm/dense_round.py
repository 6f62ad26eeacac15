"""What the side algorithms share above the kernels: the rules that are not the
reference's, each of which keeps the round's messages and answers in ``aggregate_worker_data``.

* ``RoundAlgorithm``: the ``device`` and ``out_dtype`` arguments, ``aggregate_loss`` and the result
  message. A rule implements ``_aggregate_parameter``. ``SparseFedAVGAlgorithm`` stops here.
* ``DenseRoundAlgorithm``: the rules over dense full updates. Delta and quantised payloads are
  refused (``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's
  server restores or dequantises before handing an update over); ``_rows`` checks that every client
  holds every tensor with the same shape, ``_alphas`` gives the clients' weights, ``_previous`` the
  model given to ``set_old_parameter``. The texts name the rule through class attributes.
* ``_CpuRound`` / ``_GpuRound``: the round's clients staged once, with the distances to a point, the
  fold and the step about a point on them. On the GPU the pointer table is built once per round and
  ``table_of`` builds one of a chosen subset over the same staged tensors.
* ``sqdist_to_point_cpu`` / ``pairwise_sqdist_cpu`` / ``weighted_mean_cpu``: the CPU device's
  arithmetic, in the kernels' pinned orders.
"""

from __future__ import annotations

import math
from abc import abstractmethod
from collections.abc import Iterable
from typing import Any

import torch

from ..fedavg import ClientTable, ModelLayout, NaNAggregationError, out_code
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind
from ..quantized import QuantizedTensor
from .aggregation_algorithm import (
    AggregationAlgorithm,
    context_for,
    default_device,
    split_empty,
    to_device_operand,
    unify_dtype,
)

# the kernel's geometry where the native library cannot be asked
POINT_DEFAULTS = {"point_chunk": 4096, "point_threads": 256,
                  "point_ae_f32": 4, "point_ae_f16": 8, "point_ae_bf16": 8, "point_ae_f64": 2}
_DTYPE_TAGS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.float64: "f64"}


def point_constants(dtype: torch.dtype) -> tuple[int, int, int]:
    """(chunk, threads, ae) of ``fedavg_sqdist_to_point`` for a client dtype: from the native
    library, or the documented defaults where it is not built."""
    names = ("point_chunk", "point_threads", f"point_ae_{_DTYPE_TAGS[dtype]}")
    try:
        from .._native import kernel_constant

        return tuple(kernel_constant(n) for n in names)  # type: ignore[return-value]
    except (ImportError, OSError):
        return tuple(POINT_DEFAULTS[n] for n in names)  # type: ignore[return-value]


def sqdist_to_point_cpu(rows: list[list[torch.Tensor]], point: list[torch.Tensor] | None = None,
                        chunk: int | None = None, threads: int | None = None, ae: int | None = None) -> torch.Tensor:
    """``fedavg_sqdist_to_point`` in torch, in the kernel's pinned order:
    ``rows[i]`` are client i's tensors in layout order (one dtype), ``point`` one float64 tensor per
    tensor or ``None`` for the origin. Every segment is cut into chunks of ``chunk`` elements, padded
    with +0.0; lane ``l`` of ``threads`` adds the positions ``(k * threads + l) * ae + i`` in
    ascending order into one accumulator; the 64 lanes of a wave are combined by the halving tree
    (off = 32 .. 1), the waves in wave order, the chunks sequentially from +0.0 in layout order.
    Vectorised over clients and chunks. Raises ``NaNAggregationError`` like the kernel's flags."""
    n = len(rows)
    if chunk is None or threads is None or ae is None:
        dt = rows[0][0].dtype if rows and rows[0] else torch.float64
        c, th, a = point_constants(dt if dt in _DTYPE_TAGS else torch.float64)
        chunk, threads, ae = chunk or c, threads or th, ae or a
    per_lane = chunk // (threads * ae)
    assert per_lane >= 1 and per_lane * threads * ae == chunk and threads % 64 == 0
    x = [[t.to(torch.float64).reshape(-1) for t in r] for r in rows]
    bad = [i for i in range(n) if any(bool(torch.isnan(t).any()) for t in x[i])]
    if bad:
        raise NaNAggregationError("input", f"NaN in client update(s) at rows {bad}", bad)
    if point is not None and any(bool(torch.isnan(z).any()) for z in point):
        raise NaNAggregationError("input", "NaN in the point")
    out = torch.zeros(n, dtype=torch.float64)
    for s in range(len(x[0]) if n else 0):
        X = torch.stack([x[i][s] for i in range(n)])
        numel = X.shape[1]
        if numel == 0:
            continue
        d = X if point is None else X - point[s].to(torch.float64).reshape(-1)
        q = d * d
        nch = (numel + chunk - 1) // chunk
        q = torch.nn.functional.pad(q, (0, nch * chunk - numel)).reshape(n, nch, per_lane, threads, ae)
        acc = torch.zeros((n, nch, threads), dtype=torch.float64, device=q.device)
        for k in range(per_lane):
            for i in range(ae):
                acc = acc + q[:, :, k, :, i]
        a = acc.reshape(n, nch, threads // 64, 64)
        off = 32
        while off >= 1:
            a = a[..., :off] + a[..., off:2 * off]
            off //= 2
        part = a[..., 0, 0]
        for w in range(1, threads // 64):
            part = part + a[..., w, 0]
        part = part.cpu()
        for c in range(nch):
            out = out + part[:, c]
    if torch.isnan(out).any():
        raise NaNAggregationError("accumulator", "NaN in a distance to the point (inf - inf in one element)")
    return out


def pairwise_sqdist_cpu(rows: list[list[torch.Tensor]]) -> torch.Tensor:
    """Krum's distance contract in torch: ``rows[i]`` are client i's tensors in
    layout order. A plain float64 loop over the pairs ``i < j``, mirrored. Raises
    ``NaNAggregationError`` like the kernel's flags."""
    n = len(rows)
    x = [[t.to(torch.float64).reshape(-1) for t in r] for r in rows]
    bad = [i for i in range(n) if any(bool(torch.isnan(t).any()) for t in x[i])]
    if bad:
        raise NaNAggregationError("input", f"NaN in client update(s) at rows {bad}", bad)
    D = torch.zeros((n, n), dtype=torch.float64)
    for i in range(n):
        for j in range(i + 1, n):
            s = torch.zeros((), dtype=torch.float64)
            for a, b in zip(x[i], x[j]):
                d = a - b
                s = s + (d * d).sum()
            D[i, j] = D[j, i] = s.cpu()
    if torch.isnan(D).any():
        raise NaNAggregationError("accumulator", "NaN in a pairwise distance (inf - inf in one element)")
    return D


def weighted_mean_cpu(rows: list[list[torch.Tensor]], weights: list[float],
                      out_dtype: torch.dtype) -> list[torch.Tensor]:
    """The reference's float64 fold of ``rows`` (client by client, their tensors in layout order)
    with ``weights``, one tensor per tensor of the layout in ``out_dtype``."""
    total = 0.0
    for w in weights:
        total += w
    outs = []
    for i in range(len(rows[0])):
        acc = None  # fed_avg_algorithm.py:54-58: tmp = x.to(f64) * w; acc += tmp
        for r, w in zip(rows, weights):
            tmp = r[i].to(torch.float64) * w
            acc = tmp if acc is None else acc + tmp
        if torch.isnan(acc).any():
            raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
        out = acc / total
        if torch.isnan(out).any():
            raise NaNAggregationError("result", "NaN after dividing by the total weight (e.g. 0 / 0)")
        outs.append(out.to(out_dtype))
    return outs


class _CpuRound:
    """The round's clients on a CPU device: distances in the pinned order, the reference's fold and
    the step about a point in the kernel's five operations."""

    def __init__(self, layout: ModelLayout, rows: list[list[torch.Tensor]], device: torch.device) -> None:
        flat = [t.to(device) for r in rows for t in r]
        if flat:
            flat, _ = unify_dtype(flat)  # one input format per call, as on the GPU path
        T = layout.num_segments
        self.layout = layout
        self.rows = [flat[k * T:(k + 1) * T] for k in range(len(rows))]

    def keep(self, kept: list[int]) -> None:
        self.rows = [self.rows[k] for k in kept]

    def distances(self, point: list[torch.Tensor] | None) -> list[float]:
        return sqdist_to_point_cpu(self.rows, point).tolist()

    def fold(self, weights: list[float], out_dtype: torch.dtype) -> list[torch.Tensor]:
        return weighted_mean_cpu(self.rows, weights, out_dtype)

    def centre(self, tensors: list[torch.Tensor]) -> list[torch.Tensor]:
        return tensors

    def step(self, coef: list[float], divisor: float, point: list[torch.Tensor],
             out_dtype: torch.dtype) -> list[torch.Tensor]:
        outs = []
        for i in range(self.layout.num_segments):
            z = point[i].to(torch.float64)
            acc = None
            for r, c in zip(self.rows, coef):
                p = (r[i].to(torch.float64) - z) * c
                acc = p if acc is None else acc + p
            if torch.isnan(acc).any():
                raise NaNAggregationError("accumulator", "NaN in the clipped sum (e.g. inf - inf or 0 * inf)")
            out = z + acc / divisor
            if torch.isnan(out).any():
                raise NaNAggregationError("result", "NaN after adding the step to the centre (e.g. inf - inf)")
            outs.append(out.to(out_dtype))
        return outs

    def finish(self) -> None:
        pass


class _GpuRound:
    """The round's clients on the GPU, staged once: one pointer table, reused by every fold, step
    and distance call. ``weights`` are the table's weights per client (0.0 where every call brings
    its own); with no element to read (``native is None``) there is neither table nor context."""

    def __init__(self, layout: ModelLayout, rows: list[list[torch.Tensor]], device: torch.device,
                 weights: list[float] | None = None) -> None:
        self.layout = layout
        self.device = device
        self.n = len(rows)
        self.weights = weights if weights is not None else [0.0] * self.n
        self.native, self.segments = split_empty(layout)
        if self.native is None:
            return
        flat = [to_device_operand(rows[k][i], device) for k in range(self.n) for i in self.segments]
        flat, self.dt = unify_dtype(flat)
        self.flat = [t.contiguous() for t in flat]
        self.ctx = context_for(self.native, device)
        self.table = self.table_of(range(self.n))

    def table_of(self, kept: Iterable[int]) -> ClientTable:
        """A new table of the round's rows ``kept``, over the tensors staged once."""
        T = len(self.segments)
        table = ClientTable(T)
        for k in kept:
            table.add_client(self.flat[k * T:(k + 1) * T], [self.weights[k]] * T)
        return table

    def keep(self, kept: list[int]) -> None:
        if self.native is not None and len(kept) != self.n:
            self.table = self.table_of(kept)
        self.n = len(kept)

    def _flat(self, tensors: list[torch.Tensor]) -> list[torch.Tensor]:
        return [tensors[i].reshape(-1) for i in self.segments]

    def _outputs(self, out_dtype: torch.dtype) -> tuple[list[torch.Tensor], list[torch.Tensor]]:
        """One new tensor per tensor of the layout, and the non-empty ones flat for the kernel."""
        outs = [torch.empty(s, dtype=out_dtype, device=self.device) for s in self.layout.shapes]
        return outs, [outs[i].view(-1) for i in self.segments]

    def distances(self, point: list[torch.Tensor] | None) -> list[float]:
        if self.native is None:
            return [0.0] * self.n
        z = None if point is None else self._flat(point)
        D = self.ctx.sqdist_to_point(self.table, self.dt, z).cpu()  # the copy synchronises: the flags are final
        self.ctx.raise_on_nan([(self.table, self.dt)])
        return D.tolist()

    def fold(self, weights: list[float], out_dtype: torch.dtype) -> list[torch.Tensor]:
        outs, flat = self._outputs(out_dtype)
        if self.native is not None:
            self.table.set_weights(weights)
            self.ctx.aggregate(self.table, self.dt, flat, out_dtype)
        return outs

    def centre(self, tensors: list[torch.Tensor]) -> list[torch.Tensor]:
        return [t.contiguous() for t in tensors]

    def step(self, coef: list[float], divisor: float, point: list[torch.Tensor],
             out_dtype: torch.dtype) -> list[torch.Tensor]:
        outs, flat = self._outputs(out_dtype)
        if self.native is not None:
            self.ctx.fold_about_point(self.table, self.dt, coef, divisor, self._flat(point), flat, out_dtype)
        return outs

    def finish(self) -> None:
        if self.native is not None:
            self.ctx.raise_on_nan([(self.table, self.dt)])


def finite_screen(work: _CpuRound | _GpuRound, ids: list[int]) -> tuple[list[int], list[int]]:
    """The rows whose squared norm is not ``+inf`` and the worker ids of the others, which the rule
    drops for the round; a NaN input raises."""
    norms = work.distances(None)
    return ([k for k, v in enumerate(norms) if v != math.inf],
            [ids[k] for k, v in enumerate(norms) if v == math.inf])


class RoundAlgorithm(AggregationAlgorithm):
    """``out_dtype`` float64 (what the reference's algorithms return) or float32 (that result
    rounded to nearest even); ``device`` a GPU (default: the current one) or the CPU. Call
    ``__init__`` after the rule's own arguments are checked: theirs are the first refusals."""

    def __init__(self, device: torch.device | str | None, out_dtype: torch.dtype) -> None:
        super().__init__()
        out_code(out_dtype)  # TypeError for anything but float32 / float64
        self.out_dtype = out_dtype
        self.aggregate_loss: bool = False
        self.__device = torch.device(device) if device is not None else None

    @property
    def device(self) -> torch.device:
        if self.__device is None:
            self.__device = default_device()
        if self.__device.type == "cuda" and self.__device.index is None:
            self.__device = torch.device("cuda", torch.cuda.current_device())
        return self.__device

    @abstractmethod
    def _aggregate_parameter(self) -> ModelParameter: ...

    def aggregate_worker_data(self) -> Any:
        return self._result_message(self._aggregate_parameter())


class DenseRoundAlgorithm(RoundAlgorithm):
    """A rule over the clients' dense full updates. The class attributes are the rule's words in the
    refusals: ``rule_subject`` starts a sentence ("Krum needs full updates"; ``rule_verb_ending`` is
    empty for a plural subject), ``rule_name`` stands inside one ("Krum compares whole updates");
    ``max_clients`` is the limit ``_rows`` enforces (``None``: the rule checks its own)."""

    accepts_delta_messages = False
    accepts_quantized_messages = False
    rule_subject = ""
    rule_verb_ending = "s"
    rule_name = ""
    max_clients: int | None = None
    shape_error_names_client = False

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            who, s = self.rule_subject, self.rule_verb_ending
            kind = message_kind(worker_data)
            if kind == KIND_DELTA:
                raise NotImplementedError(
                    f"{who} need{s} full updates: restore a DeltaParameterMessage first "
                    "(accepts_delta_messages is False, so this package's server does)")
            if kind != KIND_PARAMETER:
                raise TypeError(f"{who} take{s} ParameterMessage updates, not {type(worker_data).__name__}")
            if any(isinstance(t, QuantizedTensor) for t in worker_data.parameter.values()):
                raise NotImplementedError(
                    f"{who} read{s} dense tensors: dequantise QSGD / NNADQ payloads first "
                    "(accepts_quantized_messages is False, so this package's server does)")
        return super().process_worker_data(worker_id, worker_data)

    # ---- end of round ---------------------------------------------------------------------
    def _rows(self) -> tuple[ModelLayout, list[int], list[list[torch.Tensor]]]:
        """The layout (names in first-seen order), the worker ids in arrival order and, per worker,
        its tensors in layout order; ValueError for a client that lacks a key or differs in shape."""
        assert self._all_worker_data
        shapes: dict[str, tuple[int, ...]] = {}
        for wid, msg in self._all_worker_data.items():
            assert msg.parameter
            for name, t in msg.parameter.items():
                shape = shapes.setdefault(name, tuple(t.shape))
                if tuple(t.shape) != shape:
                    client = f"client {wid}, " if self.shape_error_names_client else ""
                    raise ValueError(f"{client}tensor {name}: shape {tuple(t.shape)} differs from {shape}")
        ids, rows = [], []
        for wid, msg in self._all_worker_data.items():
            for name in shapes:
                if name not in msg.parameter:
                    raise ValueError(f"client {wid} lacks tensor {name}: {self.rule_name} compares whole updates")
            ids.append(wid)
            rows.append([msg.parameter[name] for name in shapes])
        if self.max_clients is not None and len(ids) > self.max_clients:
            raise NotImplementedError(f"{len(ids)} clients: {self.rule_name} takes at most {self.max_clients}")
        return ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), ids, rows

    def _alphas(self, ids: list[int]) -> list[float]:
        """The clients' weights: 1.0 each or, where the rule's ``weighted`` is set, their own
        ``aggregation_weight``."""
        if not self.weighted:
            return [1.0] * len(ids)
        ws = [self._all_worker_data[w].aggregation_weight for w in ids]
        assert all(w is not None and w >= 0 for w in ws)
        return [float(w) for w in ws]

    def _previous(self, layout: ModelLayout, device: torch.device) -> list[torch.Tensor]:
        """The model given to ``set_old_parameter`` in layout order, float64 on ``device``."""
        old = self._old_parameter
        if old is None:
            raise ValueError('start="previous" needs the previous global model: set_old_parameter was never called '
                             f"(tensor {layout.names[0]})")
        out = []
        for name, shape in zip(layout.names, layout.shapes):
            if name not in old:
                raise ValueError(f"the previous global model lacks tensor {name}")
            if tuple(old[name].shape) != tuple(shape):
                raise ValueError(f"tensor {name}: the previous global model's shape {tuple(old[name].shape)} "
                                 f"differs from {tuple(shape)}")
            out.append(old[name].detach().to(device=device, dtype=torch.float64))
        for name in old:
            if name not in layout.names:
                raise ValueError(f"the previous global model holds tensor {name}, which no client sent")
        return out

    def _named(self, layout: ModelLayout, tensors: list[torch.Tensor]) -> ModelParameter:
        """A round's result tensors by name, in ``out_dtype`` and the layout's shapes."""
        return {name: tensors[i].to(self.out_dtype).view(layout.shapes[i]) for i, name in enumerate(layout.names)}
