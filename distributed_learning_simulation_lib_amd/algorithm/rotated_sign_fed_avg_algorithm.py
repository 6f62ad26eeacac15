"""FedAvg over randomly rotated 1-bit deltas (DRIVE clients), folded on the GPU in the rotated domain.

A rotated sign delta (``rotated.RotatedSignDelta``) stands for ``D H_B (-+scale)``. The rotation is
linear and the clients of a round share it, so the server averages the ``-+scale`` vectors and inverts
the rotation once. The contract is its own, like the low-rank fold's:

1. The clients of the round that were not skipped (``None``) count, in arrival order. Each sends a
   ``DeltaParameterMessage`` whose ``delta_parameter`` holds every key of the previous global model.
   A value is a ``RotatedSignDelta`` or a dense tensor (float32 / float16 / bfloat16 / float64).
2. The previous model is the one given to ``set_old_parameter``; ``b`` is it converted to float64.
3. ``w_i`` is the client's ``aggregation_weight``; ``W`` is their sum in arrival order.
4. Per padded element of a block: ``d_i`` = ``-s_i`` where client ``i``'s bit is set, ``+s_i`` elsewhere
   (``s_i`` its magnitude of the block, converted exactly to float64); ``p_i = d_i * w_i``; ``acc = p_0 +
   p_1 + ...`` in arrival order; ``m = acc / W``; ``z = H_B m`` (levels ``h = 1, 2, ..., B / 2`` in that
   order); ``out = b + D z``: separately rounded float64 operations. ``out_dtype`` float32 is that
   result rounded to nearest even.
5. A NaN ``d_i`` raises ``NaNAggregationError`` (stage ``input``), a NaN in ``acc`` stage
   ``accumulator``, a NaN in the result stage ``result``.
6. A round in which every value is a ``RotatedSignDelta`` of one scale dtype, with equal ``(seed, draw,
   tensor_id)`` per tensor, is folded by ``fedavg_rsign_aggregate_delta``; on a CPU ``device`` a numpy
   restatement of the same six operations runs (``rotated.fold_numpy``): the same bits on both.
   Differing ``(seed, draw)`` or tensor ids among rotated clients raise ``ValueError``: there is no
   common rotated domain. Any other round (a dense value among them) is densified and goes through
   the dense delta path (``fedavg_aggregate_delta``), which gives the bits of FedAvg on the densified
   deltas, not the rotated fold's: the average is then taken after the inverse rotation.

Non-streaming: the messages are kept (they are 1/32 of a dense update) and folded in one launch at
``aggregate_worker_data``. Limits: at most 1024 clients, one GPU.
"""

from __future__ import annotations

import torch

from .._native import POINT_MAX_CLIENTS
from ..fedavg import ClientTable, ModelLayout, NaNAggregationError
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind
from ..rotated import RotatedSignDelta, fold_numpy
from ..sparse import VALUE_DTYPES
from .aggregation_algorithm import context_for, fill_empty, split_empty, unify_dtype
from .dense_round import RoundAlgorithm
from .sign_fed_avg_algorithm import fold_cpu


def _dense(d: RotatedSignDelta | torch.Tensor) -> torch.Tensor:
    return d.to_dense() if isinstance(d, RotatedSignDelta) else d


class RotatedSignFedAVGAlgorithm(RoundAlgorithm):
    """``out_dtype`` float64 or float32 (that result rounded to nearest even); ``device`` a GPU
    (default: the current one) or the CPU."""

    accepts_delta_messages = True
    accepts_rotated_messages = True
    accepts_quantized_messages = False

    def __init__(self, device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__(device, out_dtype)

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            kind = message_kind(worker_data)
            if kind == KIND_PARAMETER:
                raise NotImplementedError(
                    "the rotated sign fold takes DeltaParameterMessage updates: full ParameterMessage updates are "
                    "FedAVGAlgorithm's")
            if kind != KIND_DELTA:
                raise TypeError(
                    f"the rotated sign fold takes DeltaParameterMessage updates, not {type(worker_data).__name__}")
        return super().process_worker_data(worker_id, worker_data)

    # ---- end of round ---------------------------------------------------------------------
    def _base_model(self) -> tuple[ModelLayout, list[torch.Tensor]]:
        old = self._old_parameter
        if not old:
            first = next(iter(next(iter(self._all_worker_data.values())).delta_parameter), "?")
            raise ValueError("a delta needs the previous global model: set_old_parameter was never called "
                             f"(tensor {first})")
        return ModelLayout.from_parameters(old), list(old.values())

    def _deltas(self, layout: ModelLayout,
                device: torch.device) -> tuple[list[int], list[list[RotatedSignDelta | torch.Tensor]]]:
        """The worker ids in arrival order and, per worker, its values in layout order on ``device``;
        ValueError for a key that is missing, unknown or of another shape."""
        ids, rows = [], []
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
                if not isinstance(d, (RotatedSignDelta, torch.Tensor)):
                    raise TypeError(f"tensor {name}: a RotatedSignDelta or a dense tensor is required, not "
                                    f"{type(d).__name__}")
                if d.dtype not in VALUE_DTYPES:
                    raise ValueError(f"tensor {name}: dtype {d.dtype} is not float32 / float16 / bfloat16 / float64")
                if tuple(d.shape) != tuple(shape):
                    raise ValueError(f"tensor {name}: the delta's shape {tuple(d.shape)} differs from the previous "
                                     f"global model's {tuple(shape)}")
                row.append(d.to(device))
            ids.append(wid)
            rows.append(row)
        if len(ids) > POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: the rotated sign fold takes at most {POINT_MAX_CLIENTS}")
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
            kept = [[row[i] for i in keep] for row in rows]
            rotated = [d for row in kept for d in row if isinstance(d, RotatedSignDelta)]
            if len({(d.seed, d.draw) for d in rotated}) > 1:
                raise ValueError("the rotated clients of a round share one (seed, draw), not "
                                 f"{sorted({(d.seed, d.draw) for d in rotated})}")
            for t in range(len(keep)):
                if len({row[t].tensor_id for row in kept if isinstance(row[t], RotatedSignDelta)}) > 1:
                    raise ValueError(f"tensor {layout.names[keep[t]]}: the rotated clients of a round share its tensor id")
            whole = len(rotated) == len(kept) * len(keep) and len({d.scales.dtype for d in rotated}) == 1
            if device.type != "cuda":
                if whole:
                    outs, (input_nan, acc_nan, result_nan) = fold_numpy(kept, weights, divisor, base, self.out_dtype)
                    if input_nan:
                        raise NaNAggregationError("input", "NaN in a client's magnitude")
                    if acc_nan:
                        raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
                    if result_nan:
                        raise NaNAggregationError("result", "NaN after the inverse rotation or in the base")
                else:
                    outs = fold_cpu([[_dense(d) for d in row] for row in kept], weights, divisor, base, self.out_dtype)
            else:
                ctx = context_for(native, device)
                outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
                if whole:
                    ctx.rsign_aggregate_delta(kept, weights, divisor, base, outs, self.out_dtype)
                    ctx.raise_on_nan()
                else:
                    flat, dt = unify_dtype([_dense(d).contiguous().reshape(-1) for row in kept for d in row])
                    T = len(keep)
                    table = ClientTable(T)
                    for k, w in enumerate(weights):
                        table.add_client([t.contiguous() for t in flat[k * T:(k + 1) * T]], [w] * T)
                    try:
                        ctx.aggregate_delta(table, dt, base, outs, self.out_dtype)
                        ctx.raise_on_nan([(table, dt)])
                    finally:
                        ctx.reset()
            for j, i in enumerate(keep):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        return fill_empty(layout, result, self.out_dtype, device)
