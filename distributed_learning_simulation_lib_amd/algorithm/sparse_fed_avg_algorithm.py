"""FedAvg over sparsified parameter diffs (top-k clients with error feedback), folded on the GPU
without densifying them.

The reference ships the client half: ``worker/error_feedback_worker.py`` (``ErrorFeedbackWorker``)
sends a sparsified parameter diff and keeps the rest as a residual. A sparse delta is a
``DeltaParameterMessage`` whose missing entries are ``+0.0``, so the server half is pinned by the
reference's own code: ``DeltaParameterMessage.restore`` (``message.py:40-61``) followed by
``FedAVGAlgorithm`` (``fed_avg_algorithm.py:43-99``) on the densified delta. The contract (DESIGN.md
§5n; ``tests/sparse_reference.py`` restates it independently):

1. The clients of the round that were not skipped (``None``) count, in arrival order. Each sends a
   ``DeltaParameterMessage`` whose ``delta_parameter`` holds every key of the previous global model
   (``restore``'s own assertion; a ``ValueError`` names the client and the key). A value is a
   ``sparse.SparseDelta`` — used as it is — or a dense tensor, which counts as all-present
   (``SparseDelta.dense``). All values of a round share one dtype (float32 / float16 / bfloat16 /
   float64), otherwise a ``ValueError`` names the key.
2. The previous model is the one given to ``set_old_parameter`` (this package's server does that
   for a class with ``accepts_delta_messages``); never set, a missing key or another shape: a
   ``ValueError`` names the key. ``b`` is that model converted to float64.
3. ``w_i`` is the client's ``aggregation_weight`` (int or float, >= 0); ``W`` is their sum in arrival
   order, as ``FedAVGAlgorithm`` sums scalar weights; ``W = 0`` is a ``ValueError``.
4. Per element: ``d_i`` = client ``i``'s value converted exactly to float64, or ``+0.0``;
   ``x_i = b + d_i``; ``p_i = x_i * w_i``; ``acc = p_0 + p_1 + ...`` in arrival order; ``out = acc /
   W``: separately rounded float64 operations, the add performed even for ``d_i = +0.0``.
   ``out_dtype`` float32 is that result rounded to nearest even.
5. A NaN in any ``x_i`` raises ``NaNAggregationError`` (stage ``input``), a NaN in ``acc`` stage
   ``accumulator``, a NaN in the result stage ``result``. Indices that are not strictly increasing
   inside their tensor are a ``ValueError``.
6. On a CPU ``device`` the same five operations run in torch, so the class returns the same bits on
   the CPU and on the GPU. ``last_round`` records the worker ids and the per-client ``nnz``.

Non-streaming: the messages are kept (they are small — that is the point) and folded in one launch
at ``aggregate_worker_data``. Limits: int32 indices, one value dtype per round, at most 1024
clients, one GPU; full ``ParameterMessage`` updates are ``FedAVGAlgorithm``'s.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from ..fedavg import SPARSE_INDEX_MESSAGE, ModelLayout, NaNAggregationError
from .._native import POINT_MAX_CLIENTS
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind
from ..sparse import VALUE_DTYPES, SparseDelta
from .aggregation_algorithm import context_for, fill_empty, split_empty
from .dense_round import RoundAlgorithm


class SparseRound(NamedTuple):
    """What the last round folded: the counted workers in arrival order and, per worker, the number
    of entries of every tensor in layout order."""

    worker_ids: list[int]
    nnz: list[list[int]]


def fold_cpu(rows: list[list[SparseDelta]], weights: list[float], divisor: float, base: list[torch.Tensor],
             out_dtype: torch.dtype) -> list[torch.Tensor]:
    """The rule in torch on the host, tensor by tensor, from the five operations. As on the GPU the
    indices of the whole round are checked first, and the NaN flags are collected over all tensors
    before the first that is set, in the order input, accumulator, result, is raised."""
    for row in rows:
        for d in row:
            d.validate()
    outs = []
    input_nan = acc_nan = result_nan = False
    for t, b in enumerate(base):
        b = b.reshape(-1)
        acc = None
        for row, w in zip(rows, weights):
            d = row[t]
            dense = torch.zeros(b.numel(), dtype=torch.float64)
            dense[d.indices.to(torch.int64)] = d.values.to(torch.float64)
            x = b + dense
            input_nan |= bool(torch.isnan(x).any())
            p = x * w
            acc = p if acc is None else acc + p
        acc_nan |= bool(torch.isnan(acc).any())
        out = acc / divisor
        result_nan |= bool(torch.isnan(out).any())
        outs.append(out.to(out_dtype))
    if input_nan:
        raise NaNAggregationError("input", "NaN in a restored update (a NaN value, a NaN base or inf - inf)")
    if acc_nan:
        raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
    if result_nan:
        raise NaNAggregationError("result", "NaN after dividing by the total weight")
    return outs


class SparseFedAVGAlgorithm(RoundAlgorithm):
    """``out_dtype`` float64 or float32 (that result rounded to nearest even); ``device`` a GPU
    (default: the current one) or the CPU."""

    accepts_delta_messages = True
    accepts_sparse_messages = True
    accepts_quantized_messages = False

    def __init__(self, device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__(device, out_dtype)
        self.last_round: SparseRound | None = None

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            kind = message_kind(worker_data)
            if kind == KIND_PARAMETER:
                raise NotImplementedError(
                    "the sparse fold takes DeltaParameterMessage updates: full ParameterMessage updates are "
                    "FedAVGAlgorithm's")
            if kind != KIND_DELTA:
                raise TypeError(f"the sparse fold takes DeltaParameterMessage updates, not {type(worker_data).__name__}")
        return super().process_worker_data(worker_id, worker_data)

    # ---- end of round ---------------------------------------------------------------------
    def _base_model(self) -> tuple[ModelLayout, list[torch.Tensor]]:
        old = self._old_parameter
        if not old:
            first = next(iter(next(iter(self._all_worker_data.values())).delta_parameter), "?")
            raise ValueError("a delta needs the previous global model: set_old_parameter was never called "
                             f"(tensor {first})")
        return ModelLayout.from_parameters(old), list(old.values())

    def _deltas(self, layout: ModelLayout, device: torch.device) -> tuple[list[int], list[list[SparseDelta]]]:
        """The worker ids in arrival order and, per worker, its sparse deltas in layout order on
        ``device``; ValueError for a key that is missing, unknown, of another shape or dtype."""
        ids, rows = [], []
        dtype: torch.dtype | None = None
        for wid, msg in self._all_worker_data.items():
            delta = msg.delta_parameter
            for name in delta:
                if name not in layout.names:
                    raise ValueError(f"client {wid} sent tensor {name}, which the previous global model lacks")
            row = []
            for name, shape in zip(layout.names, layout.shapes):
                if name not in delta:
                    raise ValueError(f"client {wid} lacks tensor {name}: a delta holds every key of the previous model")
                d = delta[name]
                if not isinstance(d, SparseDelta):
                    if not isinstance(d, torch.Tensor):
                        raise TypeError(f"tensor {name}: a SparseDelta or a dense tensor is required, not "
                                        f"{type(d).__name__}")
                    if d.dtype not in VALUE_DTYPES:
                        raise ValueError(f"tensor {name}: dtype {d.dtype} is not float32 / float16 / bfloat16 / float64")
                    d = SparseDelta.dense(d.to(device).contiguous())
                if d.shape != tuple(shape):
                    raise ValueError(f"tensor {name}: the delta's shape {d.shape} differs from the previous global "
                                     f"model's {tuple(shape)}")
                if dtype is None:
                    dtype = d.dtype
                if d.dtype != dtype:
                    raise ValueError(f"tensor {name} of client {wid}: dtype {d.dtype} differs from the round's {dtype} "
                                     "(all tensors of a round share one value dtype)")
                row.append(d.to(device))
            ids.append(wid)
            rows.append(row)
        if len(ids) > POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: the sparse fold takes at most {POINT_MAX_CLIENTS}")
        return ids, rows

    def _aggregate_parameter(self) -> ModelParameter:
        assert self._all_worker_data
        layout, previous = self._base_model()
        device = self.device
        ids, rows = self._deltas(layout, device)
        ws = [self._all_worker_data[w].aggregation_weight for w in ids]
        assert all(w is not None and w >= 0 for w in ws)
        W = ws[0]
        for w in ws[1:]:
            W = W + w
        if not float(W) > 0:
            raise ValueError("the clients' weights add up to 0: the average is undefined")
        weights, divisor = [float(w) for w in ws], float(W)
        native, keep = split_empty(layout)
        result: dict[str, torch.Tensor] = {}
        if native is not None:
            base = [previous[i].detach().to(device=device, dtype=torch.float64).contiguous().reshape(-1) for i in keep]
            kept_rows = [[row[i] for i in keep] for row in rows]
            if device.type == "cuda":
                ctx = context_for(native, device)
                outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
                ctx.sparse_aggregate_delta(kept_rows, weights, divisor, base, outs, self.out_dtype,
                                           check_indices=False)
                if ctx.sparse_index_errors():
                    # the same fold may have latched a NaN flag (a NaN value beside the bad index):
                    # the context is cached, so the flag must not outlive the round it belongs to
                    if ctx.flags():
                        ctx.reset()
                    raise ValueError(SPARSE_INDEX_MESSAGE)
                ctx.raise_on_nan()
            else:
                outs = fold_cpu(kept_rows, weights, divisor, base, self.out_dtype)
            for j, i in enumerate(keep):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        self.last_round = SparseRound(list(ids), [[d.nnz for d in row] for row in rows])
        return fill_empty(layout, result, self.out_dtype, device)
