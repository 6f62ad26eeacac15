"""FedAvg over MX block-scaled deltas (FP8 E4M3 / FP4 E2M1 codes under E8M0 block scales), folded on
the GPU from the codes and scale bytes themselves.

An mx delta (``mx.MXDelta``) is a ``DeltaParameterMessage`` value that stands for ``code_value *
2^(s - 127)`` per element, so the server half is pinned by the reference's own code:
``DeltaParameterMessage.restore`` (``message.py:40-61``) followed by ``FedAVGAlgorithm``
(``fed_avg_algorithm.py:43-99``) on the densified delta. The contract is that of
``SignFedAVGAlgorithm`` with another ``d_i``:

1. The clients of the round that were not skipped (``None``) count, in arrival order. Each sends a
   ``DeltaParameterMessage`` whose ``delta_parameter`` holds every key of the previous global model.
   A value is an ``MXDelta`` or a dense tensor (float32 / float16 / bfloat16 / float64).
2. The previous model is the one given to ``set_old_parameter``; ``b`` is it converted to float64.
3. ``w_i`` is the client's ``aggregation_weight``; ``W`` is their sum in arrival order.
4. Per element: ``d_i`` = client ``i``'s element value, exact in float64; ``x_i = b + d_i``; ``p_i = x_i
   * w_i``; ``acc = p_0 + p_1 + ...`` in arrival order; ``out = acc / W``: separately rounded float64
   operations. ``out_dtype`` float32 is that result rounded to nearest even.
5. A NaN in any ``x_i`` (scale byte 255, an E4M3 NaN code, a NaN base) raises ``NaNAggregationError``
   (stage ``input``), a NaN in ``acc`` stage ``accumulator``, a NaN in the result stage ``result``.
6. A round in which every client sent an ``MXDelta`` of one format for every tensor is folded by
   ``fedavg_mx_aggregate_delta`` from the payloads. Any other round is densified (exactly, into
   float64) and folded by the dense delta path (``fedavg_aggregate_delta``), which gives the same bits
   by the contract. On a CPU ``device`` the same five operations run in torch.

Non-streaming: the messages are kept (they are a quarter or an eighth of an fp32 update) and folded in
one launch at ``aggregate_worker_data``. Limits: at most 1024 clients, one GPU.
"""

from __future__ import annotations

import torch

from .._native import POINT_MAX_CLIENTS
from ..fedavg import ClientTable, ModelLayout
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind
from ..mx import MXDelta
from ..sparse import VALUE_DTYPES
from .aggregation_algorithm import context_for, fill_empty, split_empty, unify_dtype
from .dense_round import RoundAlgorithm
from .sign_fed_avg_algorithm import fold_cpu


def _dense(d: MXDelta | torch.Tensor) -> torch.Tensor:
    return d.to_dense(torch.float64) if isinstance(d, MXDelta) else d


class MXFedAVGAlgorithm(RoundAlgorithm):
    """``out_dtype`` float64 or float32 (that result rounded to nearest even); ``device`` a GPU
    (default: the current one) or the CPU."""

    accepts_delta_messages = True
    accepts_mx_messages = True
    accepts_quantized_messages = False

    def __init__(self, device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__(device, out_dtype)

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            kind = message_kind(worker_data)
            if kind == KIND_PARAMETER:
                raise NotImplementedError(
                    "the mx fold takes DeltaParameterMessage updates: full ParameterMessage updates are "
                    "FedAVGAlgorithm's")
            if kind != KIND_DELTA:
                raise TypeError(f"the mx fold takes DeltaParameterMessage updates, not {type(worker_data).__name__}")
        return super().process_worker_data(worker_id, worker_data)

    # ---- end of round ---------------------------------------------------------------------
    def _base_model(self) -> tuple[ModelLayout, list[torch.Tensor]]:
        old = self._old_parameter
        if not old:
            first = next(iter(next(iter(self._all_worker_data.values())).delta_parameter), "?")
            raise ValueError("a delta needs the previous global model: set_old_parameter was never called "
                             f"(tensor {first})")
        return ModelLayout.from_parameters(old), list(old.values())

    def _deltas(self, layout: ModelLayout, device: torch.device) -> tuple[list[int], list[list[MXDelta | torch.Tensor]]]:
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
                if not isinstance(d, (MXDelta, torch.Tensor)):
                    raise TypeError(f"tensor {name}: an MXDelta or a dense tensor is required, not {type(d).__name__}")
                if isinstance(d, torch.Tensor) and d.dtype not in VALUE_DTYPES:
                    raise ValueError(f"tensor {name}: dtype {d.dtype} is not float32 / float16 / bfloat16 / float64")
                if tuple(d.shape) != tuple(shape):
                    raise ValueError(f"tensor {name}: the delta's shape {tuple(d.shape)} differs from the previous "
                                     f"global model's {tuple(shape)}")
                row.append(d.to(device))
            ids.append(wid)
            rows.append(row)
        if len(ids) > POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: the mx fold takes at most {POINT_MAX_CLIENTS}")
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
            values = [d for row in kept for d in row]
            coded = all(isinstance(d, MXDelta) for d in values) and len({d.fmt for d in values}) == 1
            if device.type != "cuda":
                outs = fold_cpu([[_dense(d) for d in row] for row in kept], weights, divisor, base, self.out_dtype)
            else:
                ctx = context_for(native, device)
                outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
                if coded:
                    ctx.mx_aggregate_delta(kept, weights, divisor, base, outs, self.out_dtype)
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
