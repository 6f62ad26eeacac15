"""The geometric median of the clients' whole updates (RFA: Pillutla, Kakade, Harchaoui, "Robust
Aggregation for Federated Learning"), by smoothed Weiszfeld iterations with the distances on the GPU.

NOT an algorithm of the reference (it aggregates with the weighted mean only): like Krum and the
coordinate-wise rules it is built on the data path the FedAvg reduce already owns. One Weiszfeld
step is "FedAvg with the weights ``alpha_i / max(nu, |x_i - z|)``", which ``FedAvgContext.aggregate``
already is; the other half, the distance of every client's whole update to one fp64 point, is
``fedavg_sqdist_to_point``. The contract (``tests/geomed_reference.py`` restates it
independently):

1. The ``n`` clients of the round that were not skipped (``None``) count, in arrival order; every
   one of them must hold every tensor of the layout with the same shape (a ``ValueError`` names the
   client and the key). ``alpha_i`` is 1.0 each or, with ``weighted=True``, the client's
   ``aggregation_weight``. ``alpha_i = 0`` is legal: that client pulls nothing.
2. Finite screen: ``N_i = sum_e x_i[e]^2`` (the distance to the origin). A NaN input raises
   ``NaNAggregationError`` (stage ``input``) naming the clients. A client with ``N_i = +inf`` — it
   sent an infinity, or its norm is beyond float64 — is *dropped* for the round: a robust rule must
   not die of one client's ``inf``. If none is left: ``ValueError``. There is no ``n >= ...``
   condition; ``n = 1`` returns that update.
3. ``z_0`` is the FedAvg of the kept clients with the weights ``alpha``, in float64.
4. For ``t = 1 .. max_iterations``: ``D_i = sum_e (x_i[e] - z_{t-1}[e])^2`` (values converted exactly
   to float64; subtract, square and add each rounded in float64, in the pinned order of §5i);
   ``(beta, G_{t-1}) = fedavg.geometric_median_step(D, alpha, smoothing)``, that is
   ``beta_i = alpha_i / max(smoothing, sqrt(D_i))`` and ``G = sum_i alpha_i sqrt(D_i)``. If
   ``tolerance > 0``, ``t >= 2`` and ``|G_{t-2} - G_{t-1}| <= tolerance * G_{t-1}``, stop with
   ``z_{t-1}``. Otherwise ``z_t`` is the FedAvg of the kept clients with the weights ``beta``; if
   every ``beta_i`` is 0 (all ``alpha`` zero): ``ValueError``.
5. The result is the last ``z``: bit for bit what ``FedAVGAlgorithm`` returns for the kept messages
   with the last ``beta`` as their weights. With ``out_dtype=float32`` the last fold writes float32,
   that float64 result rounded to nearest even. ``last_iterations`` records the round.
6. On a CPU ``device`` the same rule runs in torch: ``sqdist_to_point_cpu`` follows the kernel's
   pinned summation order and the fold is the reference's float64 loop, so the class returns the
   same bits on the CPU and on the GPU.

On the GPU the pointer table is built once per round; every iteration only replaces its weights
(``ClientTable.set_weights``), folds (``FedAvgContext.aggregate``) and measures
(``FedAvgContext.sqdist_to_point``, whose n-double readback is the synchronisation the flag check
needs). Limits: at most 1024 clients, dense full updates only — delta and quantised payloads are
refused (``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's
server restores or dequantises before handing an update over).
"""

from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch

from ..fedavg import ClientTable, ModelLayout, NaNAggregationError, geometric_median_step, out_code
from .._native import POINT_MAX_CLIENTS
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind, wire_class
from ..quantized import QuantizedTensor
from .aggregation_algorithm import (
    AggregationAlgorithm,
    context_for,
    default_device,
    split_empty,
    to_device_operand,
    unify_dtype,
)
from .fed_avg_algorithm import FedAVGAlgorithm

# the kernel's geometry where the native library cannot be asked
POINT_DEFAULTS = {"point_chunk": 4096, "point_threads": 256,
                  "point_ae_f32": 4, "point_ae_f16": 8, "point_ae_bf16": 8, "point_ae_f64": 2}
_DTYPE_TAGS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.float64: "f64"}


class GeometricMedianIterations(NamedTuple):
    """What the last round did: the counted workers in arrival order, the ids dropped by the finite
    screen, and per measured point z_0, z_1, ... the kept clients' squared distances, the weights
    ``beta`` and the objective ``G``; ``iterations`` is the number of Weiszfeld folds that ran."""

    worker_ids: list[int]
    dropped: list[int]
    distances: list[list[float]]
    betas: list[list[float]]
    objectives: list[float]
    iterations: int


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


class _CpuRound:
    """The round's clients on a CPU device: distances in the pinned order, the reference's fold."""

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
        total = 0.0
        for w in weights:
            total += w
        outs = []
        for i in range(self.layout.num_segments):
            acc = None  # fed_avg_algorithm.py:54-58: tmp = x.to(f64) * w; acc += tmp
            for r, w in zip(self.rows, weights):
                tmp = r[i].to(torch.float64) * w
                acc = tmp if acc is None else acc + tmp
            if torch.isnan(acc).any():
                raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
            out = acc / total
            if torch.isnan(out).any():
                raise NaNAggregationError("result", "NaN after dividing by the total weight (e.g. 0 / 0)")
            outs.append(out.to(out_dtype))
        return outs

    def finish(self) -> None:
        pass


class _GpuRound:
    """The round's clients on the GPU: one pointer table, reused by every fold and distance call."""

    def __init__(self, layout: ModelLayout, rows: list[list[torch.Tensor]], device: torch.device) -> None:
        self.layout = layout
        self.device = device
        self.n = len(rows)
        self.native, self.segments = split_empty(layout)
        if self.native is None:
            return
        T = len(self.segments)
        flat = [to_device_operand(rows[k][i], device) for k in range(self.n) for i in self.segments]
        flat, self.dt = unify_dtype(flat)
        self.flat = [t.contiguous() for t in flat]
        self.ctx = context_for(self.native, device)
        self._build(list(range(self.n)))

    def _build(self, kept: list[int]) -> None:
        T = len(self.segments)
        self.table = ClientTable(T)
        for k in kept:
            self.table.add_client(self.flat[k * T:(k + 1) * T], [0.0] * T)

    def keep(self, kept: list[int]) -> None:
        if self.native is not None and len(kept) != self.n:
            self._build(kept)
        self.n = len(kept)

    def distances(self, point: list[torch.Tensor] | None) -> list[float]:
        if self.native is None:
            return [0.0] * self.n
        z = None if point is None else [point[i].reshape(-1) for i in self.segments]
        D = self.ctx.sqdist_to_point(self.table, self.dt, z).cpu()  # the copy synchronises: the flags are final
        self.ctx.raise_on_nan([(self.table, self.dt)])
        return D.tolist()

    def fold(self, weights: list[float], out_dtype: torch.dtype) -> list[torch.Tensor]:
        outs = [torch.empty(s, dtype=out_dtype, device=self.device) for s in self.layout.shapes]
        if self.native is not None:
            self.table.set_weights(weights)
            self.ctx.aggregate(self.table, self.dt, [outs[i].view(-1) for i in self.segments], out_dtype)
        return outs

    def finish(self) -> None:
        if self.native is not None:
            self.ctx.raise_on_nan([(self.table, self.dt)])


class GeometricMedianFedAVGAlgorithm(AggregationAlgorithm):
    """``max_iterations`` Weiszfeld folds at most (>= 1); ``smoothing`` is nu, the floor of a
    client's distance in its weight (> 0); ``tolerance`` stops early when the objective's relative
    change falls to it (0: never); ``weighted``: the clients' own ``aggregation_weight`` as
    ``alpha`` instead of 1.0 each; ``out_dtype`` float64 (what the reference's algorithms return) or
    float32 (that result rounded to nearest even); ``device`` a GPU (default: the current one) or
    the CPU."""

    accepts_delta_messages = False
    accepts_quantized_messages = False

    def __init__(self, max_iterations: int = 3, smoothing: float = 1e-6, tolerance: float = 0.0,
                 weighted: bool = False, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__()
        if int(max_iterations) != max_iterations or int(max_iterations) < 1:
            raise ValueError(f"max_iterations must be an integer >= 1, not {max_iterations}")
        if not (float(smoothing) > 0 and math.isfinite(float(smoothing))):
            raise ValueError(f"smoothing must be a finite number > 0, not {smoothing}")
        if not (float(tolerance) >= 0 and math.isfinite(float(tolerance))):
            raise ValueError(f"tolerance must be a finite number >= 0, not {tolerance}")
        out_code(out_dtype)  # TypeError for anything but float32 / float64
        self.max_iterations = int(max_iterations)
        self.smoothing = float(smoothing)
        self.tolerance = float(tolerance)
        self.weighted = bool(weighted)
        self.out_dtype = out_dtype
        self.aggregate_loss: bool = False
        self.last_iterations: GeometricMedianIterations | None = None
        self.__device = torch.device(device) if device is not None else None

    @property
    def device(self) -> torch.device:
        if self.__device is None:
            self.__device = default_device()
        if self.__device.type == "cuda" and self.__device.index is None:
            self.__device = torch.device("cuda", torch.cuda.current_device())
        return self.__device

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            kind = message_kind(worker_data)
            if kind == KIND_DELTA:
                raise NotImplementedError(
                    "The geometric median needs full updates: restore a DeltaParameterMessage first "
                    "(accepts_delta_messages is False, so this package's server does)")
            if kind != KIND_PARAMETER:
                raise TypeError(
                    f"The geometric median takes ParameterMessage updates, not {type(worker_data).__name__}")
            if any(isinstance(t, QuantizedTensor) for t in worker_data.parameter.values()):
                raise NotImplementedError(
                    "The geometric median reads dense tensors: dequantise QSGD / NNADQ payloads first "
                    "(accepts_quantized_messages is False, so this package's server does)")
        return super().process_worker_data(worker_id, worker_data)

    # ---- end of round ---------------------------------------------------------------------
    def _rows(self) -> tuple[ModelLayout, list[int], list[list[torch.Tensor]]]:
        """The layout (names in first-seen order), the worker ids in arrival order and, per worker,
        its tensors in layout order; ValueError for a client that lacks a key or differs in shape."""
        assert self._all_worker_data
        shapes: dict[str, tuple[int, ...]] = {}
        for msg in self._all_worker_data.values():
            assert msg.parameter
            for name, t in msg.parameter.items():
                shape = shapes.setdefault(name, tuple(t.shape))
                if tuple(t.shape) != shape:
                    raise ValueError(f"tensor {name}: shape {tuple(t.shape)} differs from {shape}")
        ids, rows = [], []
        for wid, msg in self._all_worker_data.items():
            for name in shapes:
                if name not in msg.parameter:
                    raise ValueError(
                        f"client {wid} lacks tensor {name}: the geometric median compares whole updates")
            ids.append(wid)
            rows.append([msg.parameter[name] for name in shapes])
        if len(ids) > POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: the geometric median takes at most {POINT_MAX_CLIENTS}")
        return ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), ids, rows

    def _alphas(self, ids: list[int]) -> list[float]:
        if not self.weighted:
            return [1.0] * len(ids)
        ws = [self._all_worker_data[w].aggregation_weight for w in ids]
        assert all(w is not None and w >= 0 for w in ws)
        return [float(w) for w in ws]

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        alpha = self._alphas(ids)
        device = self.device
        work = (_GpuRound if device.type == "cuda" else _CpuRound)(layout, rows, device)

        # the finite screen: a client whose squared norm is +inf is dropped for the round
        norms = work.distances(None)
        kept = [k for k, v in enumerate(norms) if v != math.inf]
        dropped = [ids[k] for k, v in enumerate(norms) if v == math.inf]
        if not kept:
            raise ValueError(f"every client of the round sent an infinite update: {dropped}")
        work.keep(kept)
        alpha = [alpha[k] for k in kept]
        if not any(a > 0 for a in alpha):
            raise ValueError("every kept client has weight 0: the geometric median is undefined")

        T = self.max_iterations
        z = work.fold(alpha, torch.float64)
        distances, betas, objectives, folds = [], [], [], 0
        for t in range(1, T + 1):
            D = work.distances(z)
            beta, G = geometric_median_step(D, alpha, self.smoothing)
            distances.append(D)
            betas.append(beta)
            objectives.append(G)
            if self.tolerance > 0 and t >= 2 and abs(objectives[-2] - G) <= self.tolerance * G:
                break
            if not any(b > 0 for b in beta):
                raise ValueError("every Weiszfeld weight is 0: the geometric median is undefined")
            z = work.fold(beta, self.out_dtype if t == T else torch.float64)
            folds += 1
        work.finish()
        self.last_iterations = GeometricMedianIterations(list(ids), dropped, distances, betas, objectives, folds)
        return {name: z[i].to(self.out_dtype).view(layout.shapes[i]) for i, name in enumerate(layout.names)}

    def aggregate_worker_data(self) -> Any:
        parameter = self._aggregate_parameter()
        other_data: dict[str, Any] = {}
        # the same message fields as KrumFedAVGAlgorithm / FedAVGAlgorithm.aggregate_worker_data
        if self.aggregate_loss:
            other_data |= FedAVGAlgorithm._FedAVGAlgorithm__aggregate_loss(self._all_worker_data)
        other_data |= FedAVGAlgorithm._FedAVGAlgorithm__check_and_reduce_other_data(self._all_worker_data)
        first = next(iter(self._all_worker_data.values()))
        return wire_class(first, "ParameterMessage")(
            parameter=parameter,
            end_training=first.end_training,
            in_round=first.in_round,
            other_data=other_data,
        )
