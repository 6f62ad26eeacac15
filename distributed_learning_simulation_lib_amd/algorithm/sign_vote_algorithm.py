"""signSGD with majority vote (Bernstein, Wang, Azizzadenesheli, Anandkumar, "signSGD: Compressed
Optimisation for Non-Convex Problems", ICML 2018; the fault-tolerance analysis is "signSGD with
Majority Vote is Communication Efficient and Fault Tolerant", ICLR 2019) over 1-bit sign deltas,
counted on the GPU from the bits themselves.

Not a reference algorithm (the reference has only the weighted mean): the contract is DESIGN.md §5x
and parity is bit-identity with a plain restatement of it.

1. The clients of the round that were not skipped (``None``) vote, whatever their arrival order. The
   messages and their checks are ``SignFedAVGAlgorithm``'s: each sends a ``DeltaParameterMessage``
   whose ``delta_parameter`` holds every key of the previous global model, a value being a
   ``SignDelta`` or a dense tensor. ``aggregation_weight`` is ignored: a majority vote is unweighted.
2. A ``SignDelta`` votes with its bits (a set bit is a negative vote; its scale is not read). A dense
   tensor votes with its sign bit, ``torch.signbit``: ``-0.0`` is negative and ``0.0`` positive, as
   ``sign_compress`` packs them.
3. Per element, with ``c`` the number of negative votes among the ``n`` clients, ``b`` the previous
   model converted to float64 and ``s = learning_rate``: ``out = b - s`` where ``2c > n``,
   ``out = b + s`` where ``2c < n`` and ``out = b`` bit for bit on a tie (``-0.0`` stays ``-0.0``).
   ``out_dtype`` float32 is that value rounded to nearest even.
4. A NaN in the previous model raises ``NaNAggregationError`` (stage ``input``).
5. On a GPU every round, mixed or not, is one ``fedavg_sign_majority_vote`` launch; on a CPU
   ``device`` the same rule runs in torch and gives the same bits.

Non-streaming: the messages are kept and voted on in ``aggregate_worker_data``. Limits: at most 1024
clients, one GPU, one step for every tensor.
"""

from __future__ import annotations

import math

import torch

from .._native import FLAG_INPUT_NAN
from ..fedavg import NaNAggregationError
from ..message import ModelParameter
from ..sign import SignDelta, _pack
from .aggregation_algorithm import context_for, fill_empty, split_empty
from .sign_fed_avg_algorithm import SignFedAVGAlgorithm

NAN_BASE = "NaN in the previous global model"


def vote_cpu(rows: list[list[torch.Tensor]], step: float, base: list[torch.Tensor],
             out_dtype: torch.dtype) -> list[torch.Tensor]:
    """The rule in torch on the host: ``rows[i][t]`` are client ``i``'s packed bits of tensor ``t``.
    Unpack, an integer sum over the clients, two compares, one add or subtract."""
    n, outs = len(rows), []
    if any(bool(torch.isnan(b).any()) for b in base):
        raise NaNAggregationError("input", NAN_BASE)
    for t, b in enumerate(base):
        b = b.reshape(-1)
        e = torch.arange(b.numel())
        c = torch.zeros(b.numel(), dtype=torch.int32)
        for row in rows:
            c += (row[t].to(torch.int32)[e >> 3] >> (e & 7).to(torch.int32)) & 1
        out = torch.where(2 * c > n, b - step, torch.where(2 * c < n, b + step, b))
        outs.append(out.to(out_dtype))
    return outs


class SignMajorityVoteAlgorithm(SignFedAVGAlgorithm):
    """``learning_rate`` (a finite float >= 0, no default) is the step of every tensor; ``out_dtype``
    float64 or float32; ``device`` a GPU (default: the current one) or the CPU."""

    def __init__(self, learning_rate: float, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        if isinstance(learning_rate, bool) or not isinstance(learning_rate, (int, float)) \
                or not (math.isfinite(learning_rate) and learning_rate >= 0):
            raise ValueError(f"learning_rate must be a finite number >= 0, not {learning_rate!r}")
        super().__init__(device, out_dtype)
        self.learning_rate = float(learning_rate)

    def _aggregate_parameter(self) -> ModelParameter:
        assert self._all_worker_data
        layout, previous = self._base_model()
        device = self.device
        _, rows = self._deltas(layout, device)
        native, keep = split_empty(layout)
        result: dict[str, torch.Tensor] = {}
        if native is not None:
            base = [previous[i].detach().to(device=device, dtype=torch.float64).contiguous().reshape(-1) for i in keep]
            # one packed vote per client and tensor: a dense value through the module's own packer
            kept = [[row[i] if isinstance(row[i], SignDelta) else
                     SignDelta(_pack(torch.signbit(row[i].detach()).reshape(-1)),
                               torch.zeros((), dtype=row[i].dtype, device=device), tuple(row[i].shape))
                     for i in keep] for row in rows]
            if device.type != "cuda":
                outs = vote_cpu([[d.bits for d in row] for row in kept], self.learning_rate, base, self.out_dtype)
            else:
                ctx = context_for(native, device)
                outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
                ctx.sign_majority_vote(kept, [self.learning_rate] * len(keep), base, outs, self.out_dtype)
                if ctx.flags() & FLAG_INPUT_NAN:  # waits for the stream
                    ctx.reset()  # the flag is sticky until reset: the context stays usable
                    raise NaNAggregationError("input", NAN_BASE)
            for j, i in enumerate(keep):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        return fill_empty(layout, result, self.out_dtype, device)
