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
   ``(coef, clipped) = rules.clipping_coefficients(D, alpha, radius)``, that is
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
from typing import NamedTuple

import torch

from .._native import POINT_MAX_CLIENTS
from ..message import ModelParameter
from ..rules import clipping_coefficients
from .dense_round import DenseRoundAlgorithm, _CpuRound, _GpuRound, finite_screen

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


class ClippedFedAVGAlgorithm(DenseRoundAlgorithm):
    """``radius`` is the clipping radius tau (finite, > 0, no default); ``iterations`` the number of
    clipping steps (>= 1); ``start`` the first centre: ``"previous"`` (the model given to
    ``set_old_parameter``) or ``"mean"`` (the FedAvg of the round); ``weighted``: the clients' own
    ``aggregation_weight`` as ``alpha`` instead of 1.0 each; ``out_dtype`` float64 or float32 (that
    result rounded to nearest even); ``device`` a GPU (default: the current one) or the CPU."""

    rule_subject = "Centred clipping"
    rule_name = "centred clipping"
    max_clients = POINT_MAX_CLIENTS

    def __init__(self, radius: float, iterations: int = 1, start: str = "previous", weighted: bool = False,
                 device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        if not (float(radius) > 0 and math.isfinite(float(radius))):
            raise ValueError(f"radius must be a finite number > 0, not {radius}")
        if int(iterations) != iterations or int(iterations) < 1:
            raise ValueError(f"iterations must be an integer >= 1, not {iterations}")
        if start not in STARTS:
            raise ValueError(f"start must be one of {STARTS}, not {start!r}")
        super().__init__(device, out_dtype)
        self.radius = float(radius)
        self.iterations = int(iterations)
        self.start = start
        self.weighted = bool(weighted)
        self.last_clipping: ClippingRecord | None = None

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
        work = (_GpuRound if device.type == "cuda" else _CpuRound)(layout, rows, device)

        kept, dropped = finite_screen(work, ids)  # a client whose squared norm is +inf is dropped for the round
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
        return self._named(layout, v)
