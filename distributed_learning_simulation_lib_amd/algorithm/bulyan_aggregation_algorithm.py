"""Bulyan (El Mhamdi, Guerraoui, Rouault, ICML 2018): Krum applied iteratively picks ``n - 2f``
updates, and per coordinate the mean of the ``n - 4f`` picked values closest to their median is the
result. The pairwise distances and the coordinate step run on the GPU.

NOT an algorithm of the reference (it aggregates with the weighted mean only). The contract
(``tests/bulyan_reference.py`` restates it independently):

* The ``n`` clients of the round that were not skipped (``None``) count, in arrival order. Every one
  of them must hold every tensor with the same shape: otherwise a ``ValueError`` names the client
  and the key. ``aggregation_weight`` is ignored: Bulyan is unweighted.
* ``f = num_byzantine`` (``None``: ``(n - 3) // 4``, the most the round allows), ``theta = n - 2f``
  updates are selected and ``beta = theta - 2f`` values averaged per coordinate. ``n < 4f + 3`` is a
  ``ValueError``; ``n > 256`` or ``theta > 64`` a ``NotImplementedError``.
* ``D`` is Krum's matrix of squared distances (§5h), ``rules.bulyan_select(D, f)`` the selection:
  ``theta`` times the row of the remaining ones with the smallest Krum score among them leaves
  (``max(1, r - f - 2)`` neighbours at ``r`` remaining rows — the paper's count runs out in the
  last picks, and this project then scores a row by its nearest neighbour; ties to the earlier
  arrival).
* The coordinate step runs over the selected clients (in arrival order, which does not enter the
  result): values converted exactly to float64 and sorted in the IEEE total order into
  ``s_0 <= ... <= s_{theta-1}``; ``med = s_{(theta-1)//2}``, the lower median; the window starts at
  ``a = #{t in [0, theta - beta): (s_{t+beta} - med) < (med - s_t)}`` (one rounded subtraction on
  each side, ties keep the lower value); the result is ``(s_a + ... + s_{a+beta-1}) / beta``, added
  in ascending order from ``s_a``, every add rounded, IEEE division. Because the distances to the
  median are rounded, this window is the contract, not "the beta smallest rounded distances".
* A NaN input raises ``NaNAggregationError`` (stage ``input``, at the distances). ``+inf`` / ``-inf``
  inputs are legal; the same infinity in the same element of two clients gives ``inf - inf`` in
  ``D``: stage ``accumulator``. Both infinities inside one window: stage ``result``.

On a CPU device the same rule runs in torch, so the class works without a GPU. Where every entry
of ``D`` is exact, the CPU path and the GPU path return the same bits; where ``D`` only meets
§5h's bound (its summation order differs between the two), a near-tie between two scores may
resolve differently and another client be picked. Limits: dense full updates only — delta and
quantised payloads are refused as Krum refuses them.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from ..fedavg import NaNAggregationError
from .._native import KRUM_MAX_CLIENTS, ROBUST_MAX_CLIENTS
from ..message import ModelParameter
from ..rules import bulyan_select
from .aggregation_algorithm import fill_empty
from .dense_round import DenseRoundAlgorithm, _GpuRound, pairwise_sqdist_cpu
from .robust_aggregation_algorithm import _total_order_sort


class BulyanSelection(NamedTuple):
    """What the last round decided: the counted workers in arrival order, the picked ones in pick
    order with the score each won its pick with, and the round's f, theta and beta."""

    worker_ids: list[int]
    picked: list[int]
    scores: list[float]
    f: int
    theta: int
    beta: int


def mean_around_median_cpu(tensors: list[torch.Tensor], keep: int) -> torch.Tensor:
    """The coordinate step of the contract above for one named tensor in torch (the CPU path of the
    class): float64 of the tensors' shape. Raises ``NaNAggregationError`` like the kernel's flags."""
    n = len(tensors)
    if not 1 <= keep <= n:
        raise ValueError(f"keep {keep} is not in [1, {n}]")
    x = torch.stack([t.to(torch.float64) for t in tensors])
    if torch.isnan(x).any():
        bad = [i for i in range(n) if torch.isnan(x[i]).any()]
        raise NaNAggregationError("input", f"NaN in client update(s) at rows {bad}", bad)
    s = _total_order_sort(x)
    med = s[(n - 1) // 2]
    first = torch.zeros(med.shape, dtype=torch.int64, device=x.device)
    for t in range(n - keep):
        first += ((s[t + keep] - med) < (med - s[t])).to(torch.int64)
    total = torch.gather(s, 0, first.unsqueeze(0)).squeeze(0)
    for j in range(1, keep):
        total = total + torch.gather(s, 0, (first + j).unsqueeze(0)).squeeze(0)
    out = total / float(keep)
    if torch.isnan(out).any():
        raise NaNAggregationError("result", "NaN in the mean around the median (+inf and -inf both in a window)")
    return out


class BulyanFedAVGAlgorithm(DenseRoundAlgorithm):
    """``num_byzantine`` is f, the assumed number of Byzantine clients (``None``: the most the
    round's client count allows, ``(n - 3) // 4``); ``out_dtype`` float64 (what the reference's
    algorithms return) or float32 (that result rounded to nearest even); ``device`` a GPU (default:
    the current one) or the CPU."""

    rule_subject = rule_name = "Bulyan"
    shape_error_names_client = True  # and no max_clients: _rule refuses too few clients before too many

    def __init__(self, num_byzantine: int | None = None, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        if num_byzantine is not None and int(num_byzantine) < 0:
            raise ValueError(f"num_byzantine must be >= 0, not {num_byzantine}")
        super().__init__(device, out_dtype)
        self.num_byzantine = None if num_byzantine is None else int(num_byzantine)
        self.last_selection: BulyanSelection | None = None

    def _rule(self, n: int) -> tuple[int, int, int]:
        """(f, theta, beta) for a round of n clients; the refusals that need no data."""
        f = self.num_byzantine if self.num_byzantine is not None else (n - 3) // 4
        if f < 0 or n < 4 * f + 3:
            raise ValueError(f"Bulyan needs n >= 4f + 3 clients: n = {n}, f = {f}")
        if n > KRUM_MAX_CLIENTS:
            raise NotImplementedError(f"{n} clients: Bulyan takes at most {KRUM_MAX_CLIENTS}")
        theta = n - 2 * f
        if theta > ROBUST_MAX_CLIENTS:
            raise NotImplementedError(
                f"n - 2f = {theta} selected updates: the coordinate step sorts at most {ROBUST_MAX_CLIENTS} "
                "values per element")
        return f, theta, theta - 2 * f

    def _select(self, D: torch.Tensor, ids: list[int], f: int) -> list[int]:
        """The selected rows in arrival order."""
        picked, scores = bulyan_select(D, f)
        theta = len(picked)
        self.last_selection = BulyanSelection(list(ids), [ids[r] for r in picked], scores, f, theta, theta - 2 * f)
        return sorted(picked)

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        f, _, beta = self._rule(len(ids))
        device = self.device
        if device.type != "cuda":
            rows = [[t.to(device) for t in r] for r in rows]
            chosen = self._select(pairwise_sqdist_cpu(rows), ids, f)
            return {name: mean_around_median_cpu([rows[r][i] for r in chosen], beta).to(self.out_dtype)
                    for i, name in enumerate(layout.names)}
        work = _GpuRound(layout, rows, device, [1.0] * len(ids))
        result: ModelParameter = {}
        if work.native is None:
            self._select(torch.zeros((len(ids), len(ids)), dtype=torch.float64), ids, f)
        else:
            ctx, dt = work.ctx, work.dt
            D = ctx.pairwise_sqdist(work.table, dt).cpu()  # the copy synchronises: the flags are final
            ctx.raise_on_nan([(work.table, dt)])
            picked = work.table_of(self._select(D, ids, f))
            outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in work.native.numels]
            ctx.mean_around_median(picked, dt, beta, outs, self.out_dtype)
            ctx.raise_on_nan([(picked, dt)])
            for j, i in enumerate(work.segments):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        return fill_empty(layout, result, self.out_dtype, device)
