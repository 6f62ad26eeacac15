"""Krum and Multi-Krum (Blanchard et al., NeurIPS 2017): the server keeps the updates that lie
closest to their neighbours and averages those, with the pairwise distances on the GPU.

NOT an algorithm of the reference (it aggregates with the weighted mean only): like the
coordinate-wise rules of ``robust_aggregation_algorithm.py`` it is built on the data path the FedAvg
reduce already owns. The contract (``tests/krum_reference.py`` restates it
independently):

* The ``n`` clients of the round that were not skipped (``None``) count, in arrival order. Krum
  compares whole updates, so every one of them must hold every tensor of the layout with the same
  shape: a client that lacks a key is a ``ValueError`` naming the client and the key.
* ``D[i][j] = sum_e (x_i[e] - x_j[e])^2`` over all elements of all tensors: values converted
  exactly to float64, one float64 subtraction, square and add in float64 — never the
  ``|x_i|^2 + |x_j|^2 - 2 <x_i, x_j>`` form, which cancels for updates that share a model. All terms
  are non-negative, so every entry is within ``(P + 2) * 2^-53`` relative of the exact value
  (``P`` elements in all) in any summation order. ``D`` is exactly symmetric with a ``+0.0`` diagonal.
* With ``f = num_byzantine`` (``n >= 2f + 3``), ``score_i`` is the sum of the ``n - f - 2`` smallest
  ``D[i][j]``, ``j != i`` (ascending, ties in ascending ``j``, added from the smallest). The
  ``m = num_selected`` clients with the smallest ``(score, arrival row)`` are chosen — ties go to
  the earlier arrival. ``m = 1`` is Krum; ``1 <= m <= n - f`` is Multi-Krum in its one-shot form
  (the ``m`` lowest scores at once, not iteratively). ``krum_select`` is that rule, for both paths.
* The result is the FedAvg of the chosen clients in arrival order, every weight 1.0 (the papers'
  unweighted mean) or, with ``weighted=True``, the clients' own ``aggregation_weight``: bit for bit
  what ``FedAVGAlgorithm`` returns for the chosen messages. Krum's result is the chosen update
  converted to float64.
* A NaN input raises ``NaNAggregationError`` (stage ``input``). ``+inf`` / ``-inf`` inputs are legal:
  that client's distances are ``+inf`` and it scores worst. Two clients with a same-signed infinity
  in the same element give ``inf - inf``: stage ``accumulator``.

The round's updates stay resident until ``aggregate_worker_data``, which stages them
(``dense_round._GpuRound``), makes one ``fedavg_pairwise_sqdist`` launch, reads the
n x n matrix back (the copy is the synchronisation the flag check needs), selects on the host and
runs the bit-exact ``FedAvgContext.aggregate`` over the chosen rows of the same staged tensors. On
a CPU device the same rule is computed in torch (the distances as a plain float64 loop over pairs),
so the class works without a GPU. Limits: at most 256 clients, dense full updates only — delta and
quantised payloads are refused (``accepts_delta_messages`` / ``accepts_quantized_messages`` stay
false, so this package's server restores or dequantises before handing an update over).
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from .._native import KRUM_MAX_CLIENTS
from ..message import ModelParameter
from ..rules import krum_select
from .aggregation_algorithm import fill_empty
from .dense_round import DenseRoundAlgorithm, _GpuRound, pairwise_sqdist_cpu, weighted_mean_cpu


class KrumSelection(NamedTuple):
    """What the last round decided: the counted workers in arrival order, their scores, and the
    ids of the chosen ones (arrival order)."""

    worker_ids: list[int]
    scores: list[float]
    chosen: list[int]


class KrumFedAVGAlgorithm(DenseRoundAlgorithm):
    """``num_byzantine`` is f, the assumed number of Byzantine clients (``None``: the most the
    round's client count allows, ``(n - 3) // 2``); ``num_selected`` is m (1: Krum; ``None``:
    ``n - f``, resolved per round); ``weighted``: average the chosen clients with their own
    ``aggregation_weight`` instead of 1.0 each; ``out_dtype`` float64 (what the reference's
    algorithms return) or float32 (that result rounded to nearest even); ``device`` a GPU (default:
    the current one) or the CPU."""

    rule_subject = rule_name = "Krum"
    max_clients = KRUM_MAX_CLIENTS

    def __init__(self, num_byzantine: int | None = None, num_selected: int | None = 1, weighted: bool = False,
                 device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        if num_byzantine is not None and int(num_byzantine) < 0:
            raise ValueError(f"num_byzantine must be >= 0, not {num_byzantine}")
        if num_selected is not None and int(num_selected) < 1:
            raise ValueError(f"num_selected must be >= 1, not {num_selected}")
        super().__init__(device, out_dtype)
        self.num_byzantine = None if num_byzantine is None else int(num_byzantine)
        self.num_selected = None if num_selected is None else int(num_selected)
        self.weighted = bool(weighted)
        self.last_selection: KrumSelection | None = None

    def _rule(self, n: int) -> tuple[int, int]:
        """(f, m) for a round of n clients; ValueError where the rule is undefined."""
        f = self.num_byzantine if self.num_byzantine is not None else (n - 3) // 2
        if f < 0 or n < 2 * f + 3:
            raise ValueError(f"Krum needs n >= 2f + 3 clients: n = {n}, f = {f}")
        m = self.num_selected if self.num_selected is not None else n - f
        if not 1 <= m <= n - f:
            raise ValueError(f"Multi-Krum selects 1 <= m <= n - f = {n - f} clients, not {m}")
        return f, m

    def _select(self, D: torch.Tensor, ids: list[int], f: int, m: int) -> list[int]:
        scores, chosen = krum_select(D, f, m)
        self.last_selection = KrumSelection(list(ids), scores, [ids[r] for r in chosen])
        return chosen

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        f, m = self._rule(len(ids))
        weights = self._alphas(ids)
        device = self.device
        if device.type != "cuda":
            rows = [[t.to(device) for t in r] for r in rows]
            chosen = self._select(pairwise_sqdist_cpu(rows), ids, f, m)
            outs = weighted_mean_cpu([rows[r] for r in chosen], [weights[r] for r in chosen], self.out_dtype)
            return dict(zip(layout.names, outs))
        work = _GpuRound(layout, rows, device, weights)
        result: ModelParameter = {}
        if work.native is None:
            self._select(torch.zeros((len(ids), len(ids)), dtype=torch.float64), ids, f, m)
        else:
            ctx, dt = work.ctx, work.dt
            D = ctx.pairwise_sqdist(work.table, dt).cpu()  # the copy synchronises: the flags are final
            ctx.raise_on_nan([(work.table, dt)])
            picked = work.table_of(self._select(D, ids, f, m))
            outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in work.native.numels]
            ctx.aggregate(picked, dt, outs, self.out_dtype)
            ctx.raise_on_nan([(picked, dt)])
            for j, i in enumerate(work.segments):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        return fill_empty(layout, result, self.out_dtype, device)
