"""FoolsGold (Fung, Yoon, Beschastnikh, "The Limitations of Federated Learning in Sybil Settings",
RAID 2020): sybils push the same way round after round, so every client is scored by its largest
cosine similarity to any other client's accumulated update and the look-alikes are down-weighted. It
needs no bound on the number of attackers and no root dataset.

NOT an algorithm of the reference (it aggregates with the weighted mean only). The cosines come from
the Gram matrix of the accumulated updates, which one GPU call computes with the fp64 matrix
instruction (``fedavg_gram_about_point``); the step is the fold about a point. The contract (DESIGN.md
§5y; ``tests/foolsgold_reference.py`` restates it independently):

1. The ``n`` clients of the round that were not skipped (``None``) count, in arrival order; every
   one of them must hold every tensor of the layout with the same shape. At most 256 clients. The
   clients' ``aggregation_weight`` is ignored: FoolsGold's weights are its own.
2. The centre ``v`` is the model given to ``set_old_parameter``, converted to float64.
3. One ``gram_about_point`` call: per element ``d = x_i - v`` and, with ``use_history``,
   ``h_i = history_i + d`` (two separately rounded float64 operations); ``G = R R^T`` over the rows
   ``r_i = h_i`` (``d`` without history).
4. A NaN input raises ``NaNAggregationError`` (stage ``input``). A non-finite entry of ``G`` (an
   infinite client, ``inf - inf``) raises it with stage ``accumulator`` and names the workers whose
   diagonal entry is not finite. Either way the histories are unchanged.
5. ``alpha, max_cosines = rules.foolsgold_coefficients(G, kappa)``.
6. The result is ``fold_about_point(alpha, n, v)``: ``v + (sum_i alpha_i (x_i - v)) / n``. If nobody
   is down-weighted this is the unweighted mean of the updates; if everybody is, the model stays
   at ``v``.
7. History is keyed by worker id: two float64 buffer sets per worker ever seen on the device, zero at
   first sight, which costs ``2 * 8 * P`` bytes per worker (``P`` = the model's element count). The set
   written this round becomes the worker's history only after the round's flags came back clean; a
   skipped worker keeps its own. ``state_dict()`` / ``load_state_dict()`` checkpoint the histories.
   ``use_history=False`` passes no history tables and keeps no state: the cosines are the round's.
8. ``last_foolsgold`` records the round.
9. On a CPU ``device`` the same round runs in torch: the history by the same two operations, ``G`` by
   a float64 matmul per segment, the same rule, centred clipping's fold loop. The histories and the
   fold are the same bits as on the GPU; ``G`` agrees within ``2 (P + 2) 2^-53 sum_e |r_i r_j|``
   and alpha with it, so this class does NOT promise CPU/GPU bit-identity of its result.

Limits: dense full updates only — delta and quantised payloads are refused
(``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's server
restores or dequantises before handing an update over); the paper's optional indicative-feature
weighting is not built.
"""

from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch

from .. import _native
from ..fedavg import ModelLayout, NaNAggregationError
from ..message import ModelParameter
from ..rules import foolsgold_coefficients
from .dense_round import DenseRoundAlgorithm, _CpuRound, _GpuRound


class FoolsGoldRecord(NamedTuple):
    """What the last round did: the counted workers in arrival order and, per worker, the squared
    norm of its (accumulated) update (``G``'s diagonal), its largest cosine to another worker and
    its weight alpha."""

    worker_ids: list[int]
    sqnorms: list[float]
    max_cosines: list[float]
    alphas: list[float]


def gram_about_point_cpu(rows: list[list[torch.Tensor]], point: list[torch.Tensor],
                         history: list[list[torch.Tensor]] | None
                         ) -> tuple[torch.Tensor, list[list[torch.Tensor]] | None]:
    """``fedavg_gram_about_point`` in torch: ``(G, history_out)``. ``rows[i]`` are client i's tensors in
    layout order, ``point`` one float64 tensor per tensor, ``history[i]`` client i's float64 history or
    ``None`` for no history. Raises ``NaNAggregationError`` (stage ``input``) like the kernel's flag."""
    n = len(rows)
    G = torch.zeros((n, n), dtype=torch.float64)
    new = [[] for _ in range(n)] if history is not None else None
    for s, z in enumerate(point):
        R = []
        for i in range(n):
            r = rows[i][s].to(torch.float64) - z
            if history is not None:
                r = history[i][s] + r
                new[i].append(r)
            R.append(r.reshape(-1))
        R = torch.stack(R)
        if bool(torch.isnan(z).any()) or any(bool(torch.isnan(rows[i][s]).any()) for i in range(n)) or (
                history is not None and any(bool(torch.isnan(history[i][s]).any()) for i in range(n))):
            raise NaNAggregationError("input", "NaN in a client update, the centre or a history")
        if R.shape[1]:
            G = G + (R @ R.T).cpu()
    return G, new


class _CpuFoolsGoldRound(_CpuRound):
    def gram(self, point: list[torch.Tensor], hin: list[list[torch.Tensor]] | None,
             hout: list[list[torch.Tensor]] | None) -> tuple[torch.Tensor, list[list[torch.Tensor]] | None]:
        return gram_about_point_cpu(self.rows, point, hin)

    def reset_flags(self) -> None:
        pass


class _GpuFoolsGoldRound(_GpuRound):
    def gram(self, point: list[torch.Tensor], hin: list[list[torch.Tensor]] | None,
             hout: list[list[torch.Tensor]] | None) -> tuple[torch.Tensor, list[list[torch.Tensor]] | None]:
        if self.native is None:
            return torch.zeros((self.n, self.n), dtype=torch.float64), hout
        flat_in = None if hin is None else [self._flat(h) for h in hin]
        flat_out = None if hout is None else [self._flat(h) for h in hout]
        G = self.ctx.gram_about_point(self.table, self.dt, self._flat(point), flat_in, flat_out).cpu()
        if self.ctx.flags() & _native.FLAG_INPUT_NAN:  # the copy synchronised: the flags are final
            self.ctx.raise_on_nan([(self.table, self.dt)])
        return G, hout

    def reset_flags(self) -> None:
        if self.native is not None and self.ctx.flags():
            self.ctx.reset()


class FoolsGoldFedAVGAlgorithm(DenseRoundAlgorithm):
    """``kappa`` is the confidence of the logit (finite, > 0; the paper's 1.0); ``use_history``:
    score the updates accumulated over the rounds (the paper) instead of the round's alone;
    ``out_dtype`` float64 or float32 (that result rounded to nearest even); ``device`` a GPU (default:
    the current one) or the CPU."""

    rule_subject = rule_name = "FoolsGold"
    max_clients = _native.GRAM_MAX_CLIENTS

    def __init__(self, kappa: float = 1.0, use_history: bool = True, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        if not (float(kappa) > 0 and math.isfinite(float(kappa))):
            raise ValueError(f"kappa must be a finite number > 0, not {kappa}")
        super().__init__(device, out_dtype)
        self.kappa = float(kappa)
        self.use_history = bool(use_history)
        self.last_foolsgold: FoolsGoldRecord | None = None
        self._layout: ModelLayout | None = None
        self._history: dict[int, list[torch.Tensor]] = {}  # worker id -> one float64 tensor per tensor
        self._spare: dict[int, list[torch.Tensor]] = {}    # the set the next round writes

    def _fresh(self, layout: ModelLayout, device: torch.device, zero: bool) -> list[torch.Tensor]:
        make = torch.zeros if zero else torch.empty
        return [make(tuple(s), dtype=torch.float64, device=device) for s in layout.shapes]

    def _histories(self, layout: ModelLayout, ids: list[int], device: torch.device
                   ) -> tuple[list[list[torch.Tensor]], list[list[torch.Tensor]]]:
        if self._layout is not None and self._layout != layout:
            raise ValueError("the round's tensors differ from those of the histories: FoolsGold keeps one history "
                             "per worker for one model")
        self._layout = layout
        for w in ids:
            if w not in self._history:
                self._history[w] = self._fresh(layout, device, True)
            elif any(t.device != device for t in self._history[w]):
                self._history[w] = [t.to(device) for t in self._history[w]]
            if w not in self._spare or any(t.device != device for t in self._spare[w]):
                self._spare[w] = self._fresh(layout, device, False)
        return [self._history[w] for w in ids], [self._spare[w] for w in ids]

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        device = self.device
        previous = self._previous(layout, device)
        work = (_GpuFoolsGoldRound if device.type == "cuda" else _CpuFoolsGoldRound)(layout, rows, device)
        v = work.centre(previous)
        known = set(self._history)
        hin, hout = self._histories(layout, ids, device) if self.use_history else (None, None)
        try:
            G, new = work.gram(v, hin, hout)
            diag = [float(G[i, i]) for i in range(len(ids))]
            if not bool(torch.isfinite(G).all()):
                work.reset_flags()
                bad = [ids[i] for i, d in enumerate(diag) if not math.isfinite(d)]
                raise NaNAggregationError(
                    "accumulator", f"a Gram entry is not finite (an infinite update, inf - inf): workers {bad}", bad)
            alphas, cosines = foolsgold_coefficients(G, self.kappa)
            out = work.step(alphas, float(len(ids)), v, self.out_dtype)
            work.finish()
        except Exception:
            for w in set(self._history) - known:  # a worker first seen in a failed round was not seen
                del self._history[w]
                self._spare.pop(w, None)
            raise
        if self.use_history:  # the flags came back clean: what the round wrote is the history now
            for w, old, h in zip(ids, hin, new):
                self._history[w], self._spare[w] = h, old
        self.last_foolsgold = FoolsGoldRecord(list(ids), diag, cosines, alphas)
        return self._named(layout, out)

    # ---- checkpoint -----------------------------------------------------------------------
    def state_dict(self) -> dict[str, Any]:
        """The histories as CPU float64 tensors by worker id and tensor name, and ``kappa``."""
        names = self._layout.names if self._layout is not None else ()
        return {"kappa": self.kappa, "use_history": self.use_history,
                "history": {w: {n: t.detach().to("cpu", copy=True) for n, t in zip(names, h)}
                            for w, h in self._history.items()}}

    def load_state_dict(self, state: dict[str, Any]) -> None:
        """Restore a ``state_dict()``. Validated before anything changes: the keys, that every worker
        names the same tensors with the same shapes, that every value is finite. ``kappa`` and
        ``use_history`` stay this instance's. The tensors move to the device in the next round."""
        if set(state) != {"kappa", "use_history", "history"}:
            raise ValueError(f"a FoolsGold checkpoint holds the keys kappa, use_history and history, not {sorted(state)}")
        layout, history = None, {}
        for w, named in state["history"].items():
            this = ModelLayout(names=tuple(named), shapes=tuple(tuple(t.shape) for t in named.values()))
            if layout is not None and this != layout:
                raise ValueError(f"worker {w}'s history names other tensors or shapes than the first worker's")
            layout = this
            hs = [t.detach().to("cpu", torch.float64, copy=True) for t in named.values()]
            if not all(bool(torch.isfinite(t).all()) for t in hs):
                raise ValueError(f"worker {w}'s history holds a value that is not finite")
            history[int(w)] = hs
        self._layout, self._history, self._spare = layout, history, {}
