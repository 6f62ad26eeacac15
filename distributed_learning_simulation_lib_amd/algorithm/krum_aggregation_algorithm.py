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
(``to_device_operand`` / ``unify_dtype``), makes one ``fedavg_pairwise_sqdist`` launch, reads the
n x n matrix back (the copy is the synchronisation the flag check needs), selects on the host and
runs the bit-exact ``FedAvgContext.aggregate`` over the chosen rows of the same staged tensors. On
a CPU device the same rule is computed in torch (the distances as a plain float64 loop over pairs),
so the class works without a GPU. Limits: at most 256 clients, dense full updates only — delta and
quantised payloads are refused (``accepts_delta_messages`` / ``accepts_quantized_messages`` stay
false, so this package's server restores or dequantises before handing an update over).
"""

from __future__ import annotations

from typing import Any, NamedTuple

import torch

from ..fedavg import ClientTable, ModelLayout, NaNAggregationError, krum_select, out_code
from .._native import KRUM_MAX_CLIENTS
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


class KrumSelection(NamedTuple):
    """What the last round decided: the counted workers in arrival order, their scores, and the
    ids of the chosen ones (arrival order)."""

    worker_ids: list[int]
    scores: list[float]
    chosen: list[int]


def pairwise_sqdist_cpu(rows: list[list[torch.Tensor]]) -> torch.Tensor:
    """The distance contract above in torch: ``rows[i]`` are client i's tensors in layout order.
    A plain float64 loop over the pairs ``i < j``, mirrored. Raises ``NaNAggregationError`` like
    the kernel's flags."""
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


class KrumFedAVGAlgorithm(AggregationAlgorithm):
    """``num_byzantine`` is f, the assumed number of Byzantine clients (``None``: the most the
    round's client count allows, ``(n - 3) // 2``); ``num_selected`` is m (1: Krum; ``None``:
    ``n - f``, resolved per round); ``weighted``: average the chosen clients with their own
    ``aggregation_weight`` instead of 1.0 each; ``out_dtype`` float64 (what the reference's
    algorithms return) or float32 (that result rounded to nearest even); ``device`` a GPU (default:
    the current one) or the CPU."""

    accepts_delta_messages = False
    accepts_quantized_messages = False

    def __init__(self, num_byzantine: int | None = None, num_selected: int | None = 1, weighted: bool = False,
                 device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__()
        if num_byzantine is not None and int(num_byzantine) < 0:
            raise ValueError(f"num_byzantine must be >= 0, not {num_byzantine}")
        if num_selected is not None and int(num_selected) < 1:
            raise ValueError(f"num_selected must be >= 1, not {num_selected}")
        out_code(out_dtype)  # TypeError for anything but float32 / float64
        self.num_byzantine = None if num_byzantine is None else int(num_byzantine)
        self.num_selected = None if num_selected is None else int(num_selected)
        self.weighted = bool(weighted)
        self.out_dtype = out_dtype
        self.aggregate_loss: bool = False
        self.last_selection: KrumSelection | None = None
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
                    "Krum needs full updates: restore a DeltaParameterMessage first "
                    "(accepts_delta_messages is False, so this package's server does)")
            if kind != KIND_PARAMETER:
                raise TypeError(f"Krum takes ParameterMessage updates, not {type(worker_data).__name__}")
            if any(isinstance(t, QuantizedTensor) for t in worker_data.parameter.values()):
                raise NotImplementedError(
                    "Krum reads dense tensors: dequantise QSGD / NNADQ payloads first "
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
                    raise ValueError(f"client {wid} lacks tensor {name}: Krum compares whole updates")
            ids.append(wid)
            rows.append([msg.parameter[name] for name in shapes])
        if len(ids) > KRUM_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: Krum takes at most {KRUM_MAX_CLIENTS}")
        return ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), ids, rows

    def _rule(self, n: int) -> tuple[int, int]:
        """(f, m) for a round of n clients; ValueError where the rule is undefined."""
        f = self.num_byzantine if self.num_byzantine is not None else (n - 3) // 2
        if f < 0 or n < 2 * f + 3:
            raise ValueError(f"Krum needs n >= 2f + 3 clients: n = {n}, f = {f}")
        m = self.num_selected if self.num_selected is not None else n - f
        if not 1 <= m <= n - f:
            raise ValueError(f"Multi-Krum selects 1 <= m <= n - f = {n - f} clients, not {m}")
        return f, m

    def _weights(self, ids: list[int]) -> list[float]:
        if not self.weighted:
            return [1.0] * len(ids)
        ws = [self._all_worker_data[w].aggregation_weight for w in ids]
        assert all(w is not None and w >= 0 for w in ws)
        return [float(w) for w in ws]

    def _select(self, D: torch.Tensor, ids: list[int], f: int, m: int) -> list[int]:
        scores, chosen = krum_select(D, f, m)
        self.last_selection = KrumSelection(list(ids), scores, [ids[r] for r in chosen])
        return chosen

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        f, m = self._rule(len(ids))
        weights = self._weights(ids)
        device = self.device
        if device.type != "cuda":
            rows = [[t.to(device) for t in r] for r in rows]
            chosen = self._select(pairwise_sqdist_cpu(rows), ids, f, m)
            total = 0.0
            for r in chosen:
                total += weights[r]
            result: ModelParameter = {}
            for i, name in enumerate(layout.names):
                acc = None  # fed_avg_algorithm.py:54-58: tmp = x.to(f64) * w; acc += tmp
                for r in chosen:
                    tmp = rows[r][i].to(torch.float64) * weights[r]
                    acc = tmp if acc is None else acc + tmp
                if torch.isnan(acc).any():
                    raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
                out = acc / total
                if torch.isnan(out).any():
                    raise NaNAggregationError("result", "NaN after dividing by the total weight (e.g. 0 / 0)")
                result[name] = out.to(self.out_dtype)
            return result
        native, keep = split_empty(layout)
        result = {}
        if native is None:
            self._select(torch.zeros((len(ids), len(ids)), dtype=torch.float64), ids, f, m)
        else:
            T = len(keep)
            flat = [to_device_operand(rows[k][i], device) for k in range(len(ids)) for i in keep]
            flat, dt = unify_dtype(flat)
            flat = [t.contiguous() for t in flat]
            table = ClientTable(T)
            for k in range(len(ids)):
                table.add_client(flat[k * T:(k + 1) * T], [weights[k]] * T)
            ctx = context_for(native, device)
            D = ctx.pairwise_sqdist(table, dt).cpu()  # the copy synchronises: the flags are final
            ctx.raise_on_nan([(table, dt)])
            chosen = self._select(D, ids, f, m)
            picked = ClientTable(T)
            for r in chosen:
                picked.add_client(flat[r * T:(r + 1) * T], [weights[r]] * T)
            outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
            ctx.aggregate(picked, dt, outs, self.out_dtype)
            ctx.raise_on_nan([(picked, dt)])
            for j, i in enumerate(keep):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        for i, name in enumerate(layout.names):
            if name not in result:
                result[name] = torch.empty(layout.shapes[i], dtype=self.out_dtype, device=device)
        return {name: result[name] for name in layout.names}

    def aggregate_worker_data(self) -> Any:
        parameter = self._aggregate_parameter()
        other_data: dict[str, Any] = {}
        # the same message fields as RobustFedAVGAlgorithm / FedAVGAlgorithm.aggregate_worker_data
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
