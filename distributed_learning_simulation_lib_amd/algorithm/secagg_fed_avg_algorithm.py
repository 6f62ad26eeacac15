"""FedAvg over pairwise-masked updates (secure aggregation, Bonawitz et al., CCS 2017): the server
half. Not an algorithm of the reference; the contract is DESIGN.md §5z, restated in
``tests/secagg_reference.py``.

1. The round's workers ``U`` are ``0 .. n - 1``: those that reported (``A``) and those that were
   skipped (``None``: ``D``). Each reporting client sends a ``DeltaParameterMessage`` whose
   ``delta_parameter`` holds a ``secagg.MaskedDelta`` for every key of the previous global model, all
   of one ``frac_bits``, masked for this round (the algorithm counts its rounds like the endpoint).
2. ``w_i`` is the client's ``aggregation_weight``, an integer; ``W`` their sum over ``A``. A round whose
   ``value_bits + bit_length(W)`` exceeds 63 is refused.
3. Per element, in Z/2^64: the sum of the clients' words, minus the survivors' own masks, minus the
   pair masks between a survivor and a dropout (``SecAggSession.server_table``: the seeds stand in
   for the protocol's recovery). That is the sum of the survivors' weighted fixed-point values.
4. ``out = base + ((double)(int64)S * 2^-frac_bits) / W``, ``base`` the previous model in float64;
   ``out_dtype`` float32 is that result rounded to nearest even.
5. A NaN in the base raises ``NaNAggregationError`` (stage ``input``), ``W = 0`` stage ``result``.

Non-streaming: one ``fedavg_secagg_unmask`` launch at ``aggregate_worker_data``; a CPU ``device`` runs
the numpy composition and gives the same bits. Limits: at most 1024 workers, one GPU, dense payloads.
"""

from __future__ import annotations

import torch

from ..fedavg import ModelLayout, NaNAggregationError
from ..message import KIND_DELTA, KIND_PARAMETER, Message, ModelParameter, message_kind
from ..secagg import MaskedDelta, SecAggSession, check_round_weights, unmask_numpy
from .aggregation_algorithm import context_for, fill_empty, split_empty
from .dense_round import RoundAlgorithm


class SecAggFedAVGAlgorithm(RoundAlgorithm):
    """``session_seed`` is the seed of the clients' ``SecAggSession``; ``value_bits`` the clients'
    (it bounds the total weight); ``out_dtype`` float64 or float32; ``device`` a GPU (default: the
    current one) or the CPU. ``round`` is the round the next aggregation unmasks."""

    accepts_delta_messages = True
    accepts_masked_messages = True
    accepts_quantized_messages = False

    def __init__(self, session_seed: int, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64, value_bits: int = 40) -> None:
        super().__init__(device, out_dtype)
        self.session_seed, self.value_bits = int(session_seed), int(value_bits)
        self.round = 0

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None:
            kind = message_kind(worker_data)
            if kind == KIND_PARAMETER:
                raise NotImplementedError(
                    "secure aggregation takes DeltaParameterMessage updates: masking full ParameterMessage updates "
                    "is not supported")
            if kind != KIND_DELTA:
                raise TypeError(f"secure aggregation takes DeltaParameterMessage updates, not {type(worker_data).__name__}")
            values = list(worker_data.delta_parameter.values())
            if not all(isinstance(v, MaskedDelta) for v in values):
                mixed = any(isinstance(v, MaskedDelta) for v in values)
                raise ValueError(f"client {worker_id} sent {'a mix of masked and plain' if mixed else 'plain'} values: "
                                 "a plain value would be averaged in the clear")
        return super().process_worker_data(worker_id, worker_data)

    def _rows(self, layout: ModelLayout, device: torch.device) -> tuple[list[int], list[list[MaskedDelta]], int]:
        ids, rows, frac = [], [], set()
        for wid, msg in self._all_worker_data.items():
            delta = msg.delta_parameter
            for name in delta:
                if name not in layout.names:
                    raise ValueError(f"client {wid} sent tensor {name}, which the previous global model lacks")
            order = [name for name, d in delta.items() if d.words.numel() > 0]
            if order != [name for name, n in zip(layout.names, layout.numels) if n > 0 and name in delta]:
                raise ValueError(f"client {wid} lists its tensors in another order than the previous global model: "
                                 "a tensor's position is its index in the mask stream")
            row = []
            for name, shape in zip(layout.names, layout.shapes):
                if name not in delta:
                    raise ValueError(f"client {wid} lacks tensor {name}: a delta holds every key of the previous model")
                d = delta[name]
                if tuple(d.shape) != tuple(shape):
                    raise ValueError(f"tensor {name}: the delta's shape {tuple(d.shape)} differs from the previous "
                                     f"global model's {tuple(shape)}")
                frac.add(int(d.frac_bits))
                row.append(d.to(device))
            ids.append(wid)
            rows.append(row)
        if len(frac) > 1:
            raise ValueError(f"the round mixes frac_bits {sorted(frac)}: one fixed-point format per round")
        return ids, rows, frac.pop()

    def _aggregate_parameter(self) -> ModelParameter:
        assert self._all_worker_data
        old = self._old_parameter
        if not old:
            raise ValueError("a delta needs the previous global model: set_old_parameter was never called")
        layout, previous = ModelLayout.from_parameters(old), list(old.values())
        device = self.device
        ids, rows, frac_bits = self._rows(layout, device)
        dropped = sorted(self.skipped_workers)
        workers = sorted(ids + dropped)
        if workers != list(range(len(workers))):
            raise ValueError(f"the round's workers {workers} are not 0 .. {len(workers) - 1}: the masks of a worker "
                             "the server never heard of cannot be removed")
        ws = check_round_weights([self._all_worker_data[w].aggregation_weight for w in ids], self.value_bits)
        W = float(sum(ws))
        seeds, signs = SecAggSession(self.session_seed, len(workers)).server_table(ids, dropped, self.round)
        native, keep = split_empty(layout)
        result: dict[str, torch.Tensor] = {}
        if native is not None:
            base = [previous[i].detach().to(device=device, dtype=torch.float64).contiguous().reshape(-1) for i in keep]
            words = [[row[i].words.contiguous() for i in keep] for row in rows]
            if device.type != "cuda":
                outs, result_nan, input_nan = unmask_numpy(words, seeds, signs, self.round, frac_bits, W, base,
                                                           self.out_dtype)
                if input_nan:
                    raise NaNAggregationError("input", "NaN in the previous global model")
                if result_nan:
                    raise NaNAggregationError("result", "NaN after dividing by the total weight (0 / 0)")
            else:
                ctx = context_for(native, device)
                outs = [torch.empty(n, dtype=self.out_dtype, device=device) for n in native.numels]
                ctx.secagg_unmask(words, seeds, signs, self.round, frac_bits, W, base, outs, self.out_dtype)
                ctx.raise_on_nan()
            for j, i in enumerate(keep):
                result[layout.names[i]] = outs[j].view(layout.shapes[i])
        self.round += 1
        return fill_empty(layout, result, self.out_dtype, device)
