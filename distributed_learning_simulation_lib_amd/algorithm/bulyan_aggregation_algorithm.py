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
* ``D`` is Krum's matrix of squared distances (§5h), ``fedavg.bulyan_select(D, f)`` the selection:
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

from typing import Any, NamedTuple

import torch

from ..fedavg import ClientTable, ModelLayout, NaNAggregationError, bulyan_select, out_code
from .._native import KRUM_MAX_CLIENTS, ROBUST_MAX_CLIENTS
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
from .krum_aggregation_algorithm import pairwise_sqdist_cpu
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


class BulyanFedAVGAlgorithm(AggregationAlgorithm):
    """``num_byzantine`` is f, the assumed number of Byzantine clients (``None``: the most the
    round's client count allows, ``(n - 3) // 4``); ``out_dtype`` float64 (what the reference's
    algorithms return) or float32 (that result rounded to nearest even); ``device`` a GPU (default:
    the current one) or the CPU."""

    accepts_delta_messages = False
    accepts_quantized_messages = False

    def __init__(self, num_byzantine: int | None = None, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__()
        if num_byzantine is not None and int(num_byzantine) < 0:
            raise ValueError(f"num_byzantine must be >= 0, not {num_byzantine}")
        out_code(out_dtype)  # TypeError for anything but float32 / float64
        self.num_byzantine = None if num_byzantine is None else int(num_byzantine)
        self.out_dtype = out_dtype
        self.aggregate_loss: bool = False
        self.last_selection: BulyanSelection | None = None
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
                    "Bulyan needs full updates: restore a DeltaParameterMessage first "
                    "(accepts_delta_messages is False, so this package's server does)")
            if kind != KIND_PARAMETER:
                raise TypeError(f"Bulyan takes ParameterMessage updates, not {type(worker_data).__name__}")
            if any(isinstance(t, QuantizedTensor) for t in worker_data.parameter.values()):
                raise NotImplementedError(
                    "Bulyan reads dense tensors: dequantise QSGD / NNADQ payloads first "
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
                    raise ValueError(f"client {wid}, tensor {name}: shape {tuple(t.shape)} differs from {shape}")
        ids, rows = [], []
        for wid, msg in self._all_worker_data.items():
            for name in shapes:
                if name not in msg.parameter:
                    raise ValueError(f"client {wid} lacks tensor {name}: Bulyan compares whole updates")
            ids.append(wid)
            rows.append([msg.parameter[name] for name in shapes])
        return ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), ids, rows

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
        native, keep = split_empty(layout)
        result: ModelParameter = {}
        if native is None:
            self._select(torch.zeros((len(ids), len(ids)), dtype=torch.float64), ids, f)
        else:
            T = len(keep)
            flat = [to_device_operand(rows[k][i], device) for k in range(len(ids)) for i in keep]
            flat, dt = unify_dtype(flat)
            flat = [t.contiguous() for t in flat]
            table = ClientTable(T)
            for k in range(len(ids)):
                table.add_client(flat[k * T:(k + 1) * T], [1.0] * T)
            ctx = context_for(native, device)
            D = ctx.pairwise_sqdist(table, dt).cpu()  # the copy synchronises: the flags are final
            ctx.raise_on_nan([(table, dt)])
            chosen = self._select(D, ids, f)
            picked = ClientTable(T)
            for r in chosen:
                picked.add_client(flat[r * T:(r + 1) * T], [1.0] * T)
            outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
            ctx.mean_around_median(picked, dt, beta, outs, self.out_dtype)
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
