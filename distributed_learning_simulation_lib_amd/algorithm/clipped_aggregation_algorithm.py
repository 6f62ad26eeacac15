"""Centred clipping of the clients' whole updates about the server's previous model (Karimireddy,
He, Jaggi, "Learning from History for Byzantine Robust Optimization", ICML 2021; norm bounding is its
one-iteration case), with the distances and the step on the GPU.

NOT an algorithm of the reference (it aggregates with the weighted mean only): like Krum and the
geometric median it is built on the data path the FedAvg reduce already owns. The distance of every
client's whole update to one fp64 point is ``fedavg_sqdist_to_point``; the step
``v' = v + (sum_i c_i (x_i - v)) / W`` is ``fedavg_fold_about_point``. The contract (DESIGN.md §5j;
``tests/clip_reference.py`` restates it independently):

1. The ``n`` clients of the round that were not skipped (``None``) count, in arrival order; every
   one of them must hold every tensor of the layout with the same shape (a ``ValueError`` names the
   client and the key). ``alpha_i`` is 1.0 each or, with ``weighted=True``, the client's
   ``aggregation_weight``. ``W = sum_i alpha_i`` over the counted clients, added in arrival order;
   ``W = 0`` is a ``ValueError``.
2. Finite screen, as the geometric median's: ``N_i = sum_e x_i[e]^2``. A NaN input raises
   ``NaNAggregationError`` (stage ``input``) naming the clients. A client with ``N_i = +inf`` is
   *dropped* for the round; if none is left: ``ValueError``. A dropped client stays in ``W``: it
   pulls nothing, which is the limit of a client ever farther away (``c_i -> 0``).
3. The centre ``v_0``: with ``start="previous"`` the model given to ``set_old_parameter``, converted
   to float64 and moved to the device once per round (never set, or its keys or shapes differ from
   the layout: a ``ValueError`` names the key); with ``start="mean"`` the FedAvg of the kept clients
   with the weights ``alpha``.
4. For ``l = 1 .. iterations``: ``D_i = sum_e (x_i[e] - v_{l-1}[e])^2`` in the pinned order of §5i;
   ``(coef, clipped) = fedavg.clipping_coefficients(D, alpha, radius)``, that is
   ``coef_i = alpha_i * (1 if sqrt(D_i) <= radius else radius / sqrt(D_i))``; per element
   ``d_i = x_i - v``, ``p_i = coef_i * d_i``, ``acc = p_0 + p_1 + ...`` in arrival order,
   ``r = acc / W``, ``v_l = v_{l-1} + r``: five separately rounded float64 operations. The last
   iteration writes ``out_dtype`` (float32: that float64 result rounded to nearest even). An
   infinity in the supplied centre makes every distance ``+inf``, every coefficient 0 and
   ``0 * inf`` a NaN: it surfaces as ``NaNAggregationError`` (stage ``accumulator``).
5. ``last_clipping`` records the round.
6. On a CPU ``device`` the same rule runs in torch (``sqdist_to_point_cpu`` and a loop over the
   clients with the same five operations), so the class returns the same bits on the CPU and on
   the GPU.

With every client inside the radius the result is ``v + mean(x - v)``: close to FedAvg, not bit-equal
to it. Limits: at most 1024 clients, dense full updates only — delta and quantised payloads are
refused (``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's
server restores or dequantises before handing an update over).
"""

from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch

from ..fedavg import ModelLayout, NaNAggregationError, clipping_coefficients, out_code
from .._native import POINT_MAX_CLIENTS
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind, wire_class
from ..quantized import QuantizedTensor
from .aggregation_algorithm import AggregationAlgorithm, default_device
from .fed_avg_algorithm import FedAVGAlgorithm
from .geometric_median_algorithm import _CpuRound, _GpuRound

STARTS = ("previous", "mean")


class ClippingRecord(NamedTuple):
    """What the last round did: the counted workers in arrival order, the ids dropped by the finite
    screen, and per iteration the kept clients' squared distances to the centre, their coefficients
    and the number of them that were clipped."""

    worker_ids: list[int]
    dropped: list[int]
    distances: list[list[float]]
    coefficients: list[list[float]]
    clipped: list[int]


class _CpuClipRound(_CpuRound):
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


class _GpuClipRound(_GpuRound):
    def centre(self, tensors: list[torch.Tensor]) -> list[torch.Tensor]:
        return [t.contiguous() for t in tensors]

    def step(self, coef: list[float], divisor: float, point: list[torch.Tensor],
             out_dtype: torch.dtype) -> list[torch.Tensor]:
        outs = [torch.empty(s, dtype=out_dtype, device=self.device) for s in self.layout.shapes]
        if self.native is not None:
            self.ctx.fold_about_point(self.table, self.dt, coef, divisor, [point[i].reshape(-1) for i in self.segments],
                                      [outs[i].view(-1) for i in self.segments], out_dtype)
        return outs


class ClippedFedAVGAlgorithm(AggregationAlgorithm):
    """``radius`` is the clipping radius tau (finite, > 0, no default); ``iterations`` the number of
    clipping steps (>= 1); ``start`` the first centre: ``"previous"`` (the model given to
    ``set_old_parameter``) or ``"mean"`` (the FedAvg of the round); ``weighted``: the clients' own
    ``aggregation_weight`` as ``alpha`` instead of 1.0 each; ``out_dtype`` float64 or float32 (that
    result rounded to nearest even); ``device`` a GPU (default: the current one) or the CPU."""

    accepts_delta_messages = False
    accepts_quantized_messages = False

    def __init__(self, radius: float, iterations: int = 1, start: str = "previous", weighted: bool = False,
                 device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__()
        if not (float(radius) > 0 and math.isfinite(float(radius))):
            raise ValueError(f"radius must be a finite number > 0, not {radius}")
        if int(iterations) != iterations or int(iterations) < 1:
            raise ValueError(f"iterations must be an integer >= 1, not {iterations}")
        if start not in STARTS:
            raise ValueError(f"start must be one of {STARTS}, not {start!r}")
        out_code(out_dtype)  # TypeError for anything but float32 / float64
        self.radius = float(radius)
        self.iterations = int(iterations)
        self.start = start
        self.weighted = bool(weighted)
        self.out_dtype = out_dtype
        self.aggregate_loss: bool = False
        self.last_clipping: ClippingRecord | None = None
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
                    "Centred clipping needs full updates: restore a DeltaParameterMessage first "
                    "(accepts_delta_messages is False, so this package's server does)")
            if kind != KIND_PARAMETER:
                raise TypeError(f"Centred clipping takes ParameterMessage updates, not {type(worker_data).__name__}")
            if any(isinstance(t, QuantizedTensor) for t in worker_data.parameter.values()):
                raise NotImplementedError(
                    "Centred clipping reads dense tensors: dequantise QSGD / NNADQ payloads first "
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
                    raise ValueError(f"client {wid} lacks tensor {name}: centred clipping compares whole updates")
            ids.append(wid)
            rows.append([msg.parameter[name] for name in shapes])
        if len(ids) > POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: centred clipping takes at most {POINT_MAX_CLIENTS}")
        return ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), ids, rows

    def _alphas(self, ids: list[int]) -> list[float]:
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

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        alpha = self._alphas(ids)
        W = 0.0
        for a in alpha:
            W = W + a
        if not W > 0:
            raise ValueError("the clients' weights add up to 0: centred clipping is undefined")
        device = self.device
        previous = self._previous(layout, device) if self.start == "previous" else None
        work = (_GpuClipRound if device.type == "cuda" else _CpuClipRound)(layout, rows, device)

        # the finite screen: a client whose squared norm is +inf is dropped for the round
        norms = work.distances(None)
        kept = [k for k, v in enumerate(norms) if v != math.inf]
        dropped = [ids[k] for k, v in enumerate(norms) if v == math.inf]
        if not kept:
            raise ValueError(f"every client of the round sent an infinite update: {dropped}")
        work.keep(kept)
        alpha = [alpha[k] for k in kept]

        if previous is not None:
            v = work.centre(previous)
        else:
            if not any(a > 0 for a in alpha):
                raise ValueError("every kept client has weight 0: the mean to start from is undefined")
            v = work.fold(alpha, torch.float64)
        distances, coefficients, clipped = [], [], []
        for it in range(1, self.iterations + 1):
            D = work.distances(v)
            coef, count = clipping_coefficients(D, alpha, self.radius)
            distances.append(D)
            coefficients.append(coef)
            clipped.append(count)
            v = work.step(coef, W, v, self.out_dtype if it == self.iterations else torch.float64)
        work.finish()
        self.last_clipping = ClippingRecord(list(ids), dropped, distances, coefficients, clipped)
        return {name: v[i].to(self.out_dtype).view(layout.shapes[i]) for i, name in enumerate(layout.names)}

    def aggregate_worker_data(self) -> Any:
        parameter = self._aggregate_parameter()
        other_data: dict[str, Any] = {}
        # the same message fields as GeometricMedianFedAVGAlgorithm / FedAVGAlgorithm.aggregate_worker_data
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
