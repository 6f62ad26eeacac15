"""FedAvg over low-rank deltas (PowerSGD-style clients), folded on the GPU from the factors themselves.

A low-rank delta (``lowrank.LowRankDelta``) is a ``DeltaParameterMessage`` value that stands for
``left @ right``. The contract:

1. The clients of the round that were not skipped (``None``) count, in arrival order. Each sends a
   ``DeltaParameterMessage`` whose ``delta_parameter`` holds every key of the previous global model.
   A value is a ``LowRankDelta`` or a dense tensor (float32 / float16 / bfloat16 / float64).
2. The previous model is the one given to ``set_old_parameter``; ``b`` is it converted to float64.
3. ``w_c`` is the client's ``aggregation_weight``; ``W`` is their sum in arrival order.
4. The tensors are split. A tensor for which every client sent a ``LowRankDelta`` of one rank, in the
   dtype of the first such tensor, follows the low-rank rule: ``a_c = w_c * L_c`` (the factor converted
   exactly to float64, the product rounded once); ``S = sum over (c, j) ascending of a_c[:, j] * R_c[j, :]``;
   ``out = b + S / W``. On the GPU the sum is the fp64 matrix instruction's
   (``fedavg_lowrank_aggregate_delta``: the product fused into the sum, four ``(c, j)`` to an
   instruction); on a CPU ``device`` every product and every addition is a separately rounded float64
   operation, as in ``tests/lowrank_reference.py``. **This contract is the rule's own.** It is not the
   bit pattern of ``restore()`` followed by ``FedAVGAlgorithm`` on the densified deltas
   (``sum_c (b + d_c) w_c / W``): the two agree bit for bit only where every operation is exact.
5. Every other tensor (the dense tensors a compressor always leaves: biases, norms; a tensor with
   mixed ranks or dtypes, whose ``LowRankDelta`` values are densified first) follows the dense delta
   fold, ``fedavg_aggregate_delta``, whose contract is ``SignFedAVGAlgorithm``'s step 4 with ``d_c`` the
   dense delta.
6. A NaN in a factor, a dense delta or the base raises ``NaNAggregationError`` (stage ``input``), a NaN
   sum stage ``accumulator``, a NaN result stage ``result``.

Non-streaming: the messages are kept and folded at ``aggregate_worker_data``, the low-rank tensors in
one launch. Limits: at most 1024 clients, rank at most 16, one GPU.
"""

from __future__ import annotations

import torch

from .._native import LOWRANK_MAX_RANK, POINT_MAX_CLIENTS
from ..fedavg import ClientTable, ModelLayout, NaNAggregationError
from ..lowrank import LowRankDelta
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind
from ..sparse import VALUE_DTYPES
from .aggregation_algorithm import context_for, fill_empty, unify_dtype
from .dense_round import RoundAlgorithm
from .sign_fed_avg_algorithm import fold_cpu


def lowrank_fold_cpu(rows: list[list[LowRankDelta]], weights: list[float], divisor: float, base: list[torch.Tensor],
                     out_dtype: torch.dtype) -> list[torch.Tensor]:
    """The low-rank rule in torch on the host, tensor by tensor: no ``torch.matmul``, every product and
    every addition its own float64 operation, in ascending ``(c, j)``. The NaN flags are collected
    over all tensors before the first that is set, in the order input, accumulator, result, is raised."""
    outs = []
    input_nan = acc_nan = result_nan = False
    for t, b in enumerate(base):
        first = rows[0][t]
        m, n = first.left.shape[0], first.right.shape[1]
        b = b.reshape(m, n)
        input_nan |= bool(torch.isnan(b).any())
        S = torch.zeros(m, n, dtype=torch.float64)
        for row, w in zip(rows, weights):
            L, R = row[t].left.to(torch.float64), row[t].right.to(torch.float64)
            input_nan |= bool(torch.isnan(L).any() or torch.isnan(R).any())
            a = L * w
            for j in range(L.shape[1]):
                S = S + a[:, j:j + 1] * R[j:j + 1, :]
        acc_nan |= bool(torch.isnan(S).any())
        out = b + S / divisor
        result_nan |= bool(torch.isnan(out).any())
        outs.append(out.to(out_dtype).reshape(-1))
    if input_nan:
        raise NaNAggregationError("input", "NaN in a factor or the base")
    if acc_nan:
        raise NaNAggregationError("accumulator", "NaN in the weighted sum of products (e.g. 0 * inf, inf - inf)")
    if result_nan:
        raise NaNAggregationError("result", "NaN after adding the averaged delta to the base")
    return outs


class LowRankFedAVGAlgorithm(RoundAlgorithm):
    """``out_dtype`` float64 or float32 (that result rounded to nearest even); ``device`` a GPU
    (default: the current one) or the CPU. The low-rank tensors' contract, ``b + S / W`` with ``S``
    summed by the fp64 matrix instruction, is its own: it is not the bit pattern of ``restore()`` +
    FedAvg on densified deltas, and the two agree bit for bit only where every operation is exact
    (the module's docstring, step 4)."""

    accepts_delta_messages = True
    accepts_lowrank_messages = True
    accepts_quantized_messages = False

    def __init__(self, device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        super().__init__(device, out_dtype)

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            kind = message_kind(worker_data)
            if kind == KIND_PARAMETER:
                raise NotImplementedError(
                    "the low-rank fold takes DeltaParameterMessage updates: full ParameterMessage updates are "
                    "FedAVGAlgorithm's")
            if kind != KIND_DELTA:
                raise TypeError(f"the low-rank fold takes DeltaParameterMessage updates, not {type(worker_data).__name__}")
        return super().process_worker_data(worker_id, worker_data)

    # ---- end of round ---------------------------------------------------------------------
    def _base_model(self) -> tuple[ModelLayout, list[torch.Tensor]]:
        old = self._old_parameter
        if not old:
            first = next(iter(next(iter(self._all_worker_data.values())).delta_parameter), "?")
            raise ValueError("a delta needs the previous global model: set_old_parameter was never called "
                             f"(tensor {first})")
        return ModelLayout.from_parameters(old), list(old.values())

    def _deltas(self, layout: ModelLayout, device: torch.device) -> tuple[list[int], list[list[LowRankDelta | torch.Tensor]]]:
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
                if not isinstance(d, (LowRankDelta, torch.Tensor)):
                    raise TypeError(f"tensor {name}: a LowRankDelta or a dense tensor is required, not {type(d).__name__}")
                if d.dtype not in VALUE_DTYPES:
                    raise ValueError(f"tensor {name}: dtype {d.dtype} is not float32 / float16 / bfloat16 / float64")
                if tuple(d.shape) != tuple(shape):
                    raise ValueError(f"tensor {name}: the delta's shape {tuple(d.shape)} differs from the previous "
                                     f"global model's {tuple(shape)}")
                row.append(d.to(device))
            ids.append(wid)
            rows.append(row)
        if len(ids) > POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{len(ids)} clients: the low-rank fold takes at most {POINT_MAX_CLIENTS}")
        return ids, rows

    def _dense_fold(self, layout: ModelLayout, rows: list[list[torch.Tensor]], weights: list[float], divisor: float,
                    base: list[torch.Tensor]) -> list[torch.Tensor]:
        """The dense delta fold of the tensors of ``layout``."""
        device = self.device
        if device.type != "cuda":
            return fold_cpu(rows, weights, divisor, base, self.out_dtype)
        ctx = context_for(layout, device)
        outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in layout.numels]
        flat, dt = unify_dtype([d.contiguous().reshape(-1) for row in rows for d in row])
        T = layout.num_segments
        table = ClientTable(T)
        for k, w in enumerate(weights):
            table.add_client([t.contiguous() for t in flat[k * T:(k + 1) * T]], [w] * T)
        try:
            ctx.aggregate_delta(table, dt, base, outs, self.out_dtype)
            ctx.raise_on_nan([(table, dt)])
        finally:
            ctx.reset()
        return outs

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

        # the split: the tensors every client sent as factors of one rank, in the first such tensor's dtype
        low: list[int] = []
        dense: list[int] = []
        dtype = None
        for i, numel in enumerate(layout.numels):
            if numel == 0:
                continue
            column = [row[i] for row in rows]
            fit = all(isinstance(d, LowRankDelta) for d in column) \
                and len({(d.rank, d.dtype) for d in column}) == 1 and column[0].rank <= LOWRANK_MAX_RANK \
                and (dtype is None or column[0].dtype == dtype)
            if fit:
                dtype = column[0].dtype
            (low if fit else dense).append(i)

        def part(keep: list[int]) -> tuple[ModelLayout, list[torch.Tensor]]:
            sub = ModelLayout(names=tuple(layout.names[i] for i in keep), shapes=tuple(layout.shapes[i] for i in keep))
            return sub, [previous[i].detach().to(device=device, dtype=torch.float64).contiguous().reshape(-1)
                         for i in keep]

        result: dict[str, torch.Tensor] = {}
        if low:
            sub, base = part(low)
            kept = [[row[i] for i in low] for row in rows]
            if device.type != "cuda":
                outs = lowrank_fold_cpu(kept, weights, divisor, base, self.out_dtype)
            else:
                ctx = context_for(sub, device)
                outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in sub.numels]
                ctx.lowrank_aggregate_delta(kept, weights, divisor, base, outs, self.out_dtype)
                ctx.raise_on_nan()
            for j, i in enumerate(low):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        if dense:
            sub, base = part(dense)
            kept = [[row[i].to_dense() if isinstance(row[i], LowRankDelta) else row[i] for i in dense] for row in rows]
            outs = self._dense_fold(sub, kept, weights, divisor, base)
            for j, i in enumerate(dense):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        return fill_empty(layout, result, self.out_dtype, device)
