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
   ``(beta, G_{t-1}) = rules.geometric_median_step(D, alpha, smoothing)``, that is
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
from typing import NamedTuple

import torch

from .._native import POINT_MAX_CLIENTS
from ..message import ModelParameter
from ..rules import geometric_median_step
from .dense_round import (  # noqa: F401  (the distance's home is dense_round; the names stay importable here)
    POINT_DEFAULTS,
    DenseRoundAlgorithm,
    _CpuRound,
    _GpuRound,
    finite_screen,
    point_constants,
    sqdist_to_point_cpu,
)


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


class GeometricMedianFedAVGAlgorithm(DenseRoundAlgorithm):
    """``max_iterations`` Weiszfeld folds at most (>= 1); ``smoothing`` is nu, the floor of a
    client's distance in its weight (> 0); ``tolerance`` stops early when the objective's relative
    change falls to it (0: never); ``weighted``: the clients' own ``aggregation_weight`` as
    ``alpha`` instead of 1.0 each; ``out_dtype`` float64 (what the reference's algorithms return) or
    float32 (that result rounded to nearest even); ``device`` a GPU (default: the current one) or
    the CPU."""

    rule_subject = "The geometric median"
    rule_name = "the geometric median"
    max_clients = POINT_MAX_CLIENTS

    def __init__(self, max_iterations: int = 3, smoothing: float = 1e-6, tolerance: float = 0.0,
                 weighted: bool = False, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        if int(max_iterations) != max_iterations or int(max_iterations) < 1:
            raise ValueError(f"max_iterations must be an integer >= 1, not {max_iterations}")
        if not (float(smoothing) > 0 and math.isfinite(float(smoothing))):
            raise ValueError(f"smoothing must be a finite number > 0, not {smoothing}")
        if not (float(tolerance) >= 0 and math.isfinite(float(tolerance))):
            raise ValueError(f"tolerance must be a finite number >= 0, not {tolerance}")
        super().__init__(device, out_dtype)
        self.max_iterations = int(max_iterations)
        self.smoothing = float(smoothing)
        self.tolerance = float(tolerance)
        self.weighted = bool(weighted)
        self.last_iterations: GeometricMedianIterations | None = None

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        alpha = self._alphas(ids)
        device = self.device
        work = (_GpuRound if device.type == "cuda" else _CpuRound)(layout, rows, device)

        kept, dropped = finite_screen(work, ids)  # a client whose squared norm is +inf is dropped for the round
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
        return self._named(layout, z)
