"""Coordinate-wise trimmed mean and median of the clients' updates, on the GPU.

NOT an algorithm of the reference (it aggregates with the weighted mean only): the standard
server-side answers to corrupted or adversarial clients, built on the data path the FedAvg
reduce already owns. The contract (DESIGN.md "Robust rules"; ``tests/robust_reference.py``
restates it independently), per named tensor and element:

* The ``n`` clients that sent the tensor count: a skipped client (``None``) or a key missing
  from a client does not, so ``n`` may differ between tensors.
* Values are the inputs converted exactly to float64, sorted in the IEEE total order
  (``-inf < ... < -0.0 < +0.0 < ... < +inf``) into ``s_0 <= ... <= s_{n-1}``.
* ``mode="trimmed_mean"``: ``k = floor(trim * n)``, result ``(s_k + ... + s_{n-k-1}) / (n - 2k)``,
  summed in ascending order from ``s_k``, every add rounded in float64, IEEE division.
  ``trim=0`` is the mean in *sorted* order: its bits need not equal FedAvg's arrival-order sum.
* ``mode="median"``: ``s_{(n-1)/2}`` for odd ``n``, ``(s_{n/2-1} + s_{n/2}) / 2.0`` for even ``n``.
* ``aggregation_weight`` is ignored: both rules are unweighted by definition.
* A NaN input raises ``NaNAggregationError`` (stage ``input``); a NaN result — ``+inf`` and
  ``-inf`` both among the kept values — stage ``result``.

Like the ``accumulate=False`` ratio path of ``FedAVGAlgorithm`` the round's updates stay resident
until ``aggregate_worker_data``, which stages them (``to_device_operand`` / ``unify_dtype``) and
makes one launch (``fedavg_robust_aggregate``). On a CPU device the same semantics are computed
in torch, so the class works without a GPU. Delta and quantised payloads are refused:
``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's server
restores or dequantises before handing an update over.
"""

from __future__ import annotations

import torch

from ..fedavg import ClientTable, ModelLayout, NaNAggregationError
from .._native import ROBUST_MAX_CLIENTS
from ..message import ModelParameter
from ..rules import check_robust_rule, robust_trim
from .aggregation_algorithm import context_for, fill_empty, split_empty, to_device_operand, unify_dtype
from .dense_round import DenseRoundAlgorithm

_MAGNITUDE = 0x7FFFFFFFFFFFFFFF


def _total_order_sort(x: torch.Tensor) -> torch.Tensor:
    """Sort float64 ``x`` ([n, ...]) along dim 0 in the IEEE total order: negative bit patterns
    have their magnitude bits flipped, which makes the signed integer order the total order."""
    bits = x.contiguous().view(torch.int64)
    keys = torch.where(bits < 0, bits ^ _MAGNITUDE, bits)
    keys = torch.sort(keys, dim=0).values
    return torch.where(keys < 0, keys ^ _MAGNITUDE, keys).view(torch.float64)


def robust_reduce_cpu(tensors: list[torch.Tensor], mode: str, trim: float) -> torch.Tensor:
    """The contract above for one named tensor in torch (any device; the CPU path of the class).
    Returns float64 of the tensors' shape; raises ``NaNAggregationError`` like the kernel's flags."""
    n = len(tensors)
    x = torch.stack([t.to(torch.float64) for t in tensors])
    if torch.isnan(x).any():
        bad = [i for i in range(n) if torch.isnan(x[i]).any()]
        raise NaNAggregationError("input", f"NaN in client update(s) at rows {bad}", bad)
    s = _total_order_sort(x)
    k = robust_trim(mode, trim, n)
    total = s[k].clone()
    for j in range(k + 1, n - k):
        total = total + s[j]
    out = total / float(n - 2 * k)
    if torch.isnan(out).any():
        raise NaNAggregationError("result", "NaN in the robust aggregate (+inf and -inf both kept)")
    return out


class RobustFedAVGAlgorithm(DenseRoundAlgorithm):
    """``mode`` is ``"trimmed_mean"`` (``trim`` in [0, 0.5)) or ``"median"``; ``out_dtype`` float64
    (what the reference's algorithms return) or float32 (that result rounded to nearest even);
    ``device`` a GPU (default: the current one) or the CPU."""

    # Of the dense base this rule takes the guard, the device and the result message only. It does not
    # compare whole updates: ``_columns`` stands in for ``_rows`` (so there is no ``rule_name``), and
    # ``_alphas`` and ``_previous`` have no meaning here (both rules are unweighted, with no centre).
    rule_subject = "robust aggregation"

    def __init__(self, mode: str = "trimmed_mean", trim: float = 0.1,
                 device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        check_robust_rule(mode, trim)
        super().__init__(device, out_dtype)
        self.mode = mode
        self.trim = float(trim)

    # ---- end of round ---------------------------------------------------------------------
    def _columns(self) -> tuple[ModelLayout, dict[str, list[tuple[int, torch.Tensor]]]]:
        """Names in first-seen order with, per name, (client row, tensor) of the clients that sent it."""
        assert self._all_worker_data
        shapes: dict[str, tuple[int, ...]] = {}
        cols: dict[str, list[tuple[int, torch.Tensor]]] = {}
        for row, msg in enumerate(self._all_worker_data.values()):
            assert msg.parameter
            for name, t in msg.parameter.items():
                shape = shapes.setdefault(name, tuple(t.shape))
                if tuple(t.shape) != shape:
                    raise ValueError(f"tensor {name}: shape {tuple(t.shape)} differs from {shape}")
                cols.setdefault(name, []).append((row, t))
        for name, col in cols.items():
            if len(col) > ROBUST_MAX_CLIENTS:
                raise NotImplementedError(
                    f"tensor {name} was sent by {len(col)} clients: the register-resident sort holds at most "
                    f"{ROBUST_MAX_CLIENTS} values per element")
        return ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), cols

    def _aggregate_parameter(self) -> ModelParameter:
        layout, cols = self._columns()
        device = self.device
        if device.type != "cuda":
            return {name: robust_reduce_cpu([t.to(device) for _, t in cols[name]], self.mode, self.trim)
                    .to(self.out_dtype) for name in layout.names}
        native, keep = split_empty(layout)
        result: ModelParameter = {}
        if native is not None:
            K = len(self._all_worker_data)
            rows: list[list[torch.Tensor | None]] = [[None] * len(keep) for _ in range(K)]
            present: list[torch.Tensor] = []
            where: list[tuple[int, int]] = []
            for j, i in enumerate(keep):
                for row, t in cols[layout.names[i]]:
                    present.append(to_device_operand(t, device))
                    where.append((row, j))
            present, dt = unify_dtype(present)
            for (row, j), t in zip(where, present):
                rows[row][j] = t.contiguous()
            table = ClientTable(len(keep))
            for r in rows:
                table.add_client(r, [0.0] * len(keep))
            ctx = context_for(native, device)
            outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
            ctx.robust_aggregate(table, dt, self.mode, self.trim, outs, self.out_dtype)
            ctx.raise_on_nan([(table, dt)])
            for j, i in enumerate(keep):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        return fill_empty(layout, result, self.out_dtype, device)
