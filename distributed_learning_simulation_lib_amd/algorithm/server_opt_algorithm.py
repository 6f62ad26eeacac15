"""Adaptive federated optimisation (Reddi et al., "Adaptive Federated Optimization", ICLR 2021):
FedAvgM, FedAdagrad, FedYogi and FedAdam on the server. The round's weighted mean update about the
previous global model is a pseudo-gradient, and the server takes an optimiser step along it with
moments it keeps from round to round. The fold and the step are one GPU pass over the client bytes.

NOT an algorithm of the reference (it aggregates with the weighted mean only, and replaces the
global model with it): like the robust rules it is built on the data path the FedAvg reduce already
owns. The contract (``tests/opt_reference.py`` restates it independently):

1. The ``n`` clients of the round that were not skipped (``None``) count, in arrival order; every
   one of them must hold every tensor of the layout with the same shape (the ``ValueError`` of
   ``DenseRoundAlgorithm._rows`` names the client and the key). ``c_i`` is the client's
   ``aggregation_weight`` or, with ``weighted=False``, 1.0. ``W = sum_i c_i``, added in arrival order;
   ``W = 0`` is a ``ValueError``. At most 1024 clients.
2. ``z`` is the model given to ``set_old_parameter``, converted to float64 and moved to the device
   once per round (never set, or its keys or shapes differ from the layout: the ``ValueError`` of
   ``DenseRoundAlgorithm._previous`` names the key).
3. Per element, every value converted exactly to float64 and every line one separately rounded
   float64 operation (no FMA, no reciprocal, a correctly rounded square root, no bias correction):
   ``d_i = x_i - z``, ``p_i = c_i * d_i``, ``acc = p_0 + p_1 + ...`` in arrival order,
   ``delta = acc / W`` — so far ``fedavg_fold_about_point`` — then
   ``rules.server_opt_update``'s lines for the optimiser (``m' = beta1 * m + delta`` for ``"avgm"``,
   ``m' = beta1 * m + (1 - beta1) * delta`` and the second moment's rule for the others),
   ``u = lr * m'`` (``"avgm"``) or ``(lr * m') / (sqrt(v') + tau)``, ``out = z + u`` written in
   ``out_dtype`` (float32: that float64 result rounded to nearest even).
4. The state: float64 ``m`` and, except for ``"avgm"``, ``v``, one tensor per tensor of the model,
   allocated on the device in the first round and filled with ``+0.0`` and
   ``initial_second_moment`` (default ``tau ** 2``, the paper's ``v_{-1} >= tau^2``). There are two
   buffers of each: a round writes the spare ones and they are swapped in only after the NaN flags
   came back clean, so a round that raises for any reason leaves ``m``, ``v`` and ``rounds_done``
   exactly as they were. A layout that differs from the state's is a ``ValueError``
   (``reset_state()`` starts anew).
5. A NaN in a client, in ``z``, in ``m`` or in ``v`` raises ``NaNAggregationError`` (stage
   ``input``), a NaN in ``acc`` (``inf - inf``, ``0 * inf``) stage ``accumulator``, a NaN in ``out``,
   ``m'`` or ``v'`` stage ``result``. In the adaptive modes an infinite client value makes
   ``u = inf / inf``: stage ``result``, an error and not a drop (there is no finite screen and so no
   second pass over the client bytes). ``"avgm"`` has no quotient: like the weighted mean it turns an
   infinite client value into an infinite model, and an infinite ``m``.
6. ``state_dict()`` / ``load_state_dict()`` checkpoint the moments as CPU float64 tensors by name;
   ``last_step`` records the round.
7. On a CPU ``device`` the same rule runs in torch, operation by operation, so the class returns
   the same bits on the CPU and on the GPU.

Limits: at most 1024 clients, dense full updates only — delta and quantised payloads are refused
(``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's server
restores or dequantises before handing an update over).
"""

from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch

from .._native import POINT_MAX_CLIENTS
from ..fedavg import ModelLayout, NaNAggregationError
from ..message import ModelParameter
from ..rules import SERVER_OPT_MODES, check_server_opt, server_opt_update
from .dense_round import DenseRoundAlgorithm, _CpuRound, _GpuRound


class ServerOptStep(NamedTuple):
    """What the last round did: the counted workers in arrival order, their weights, the weights'
    sum ``W`` and the optimiser."""

    worker_ids: list[int]
    weights: list[float]
    total_weight: float
    mode: str


class _CpuOptRound(_CpuRound):
    def opt_step(self, coef: list[float], divisor: float, point: list[torch.Tensor], m: list[torch.Tensor],
                 v: list[torch.Tensor] | None, m_out: list[torch.Tensor], v_out: list[torch.Tensor] | None,
                 out_dtype: torch.dtype, mode: str, hyper: tuple[float, ...]) -> list[torch.Tensor]:
        outs = []
        for i in range(self.layout.num_segments):
            z = point[i].to(torch.float64)
            vi = v[i] if v is not None else None
            if any(bool(torch.isnan(t).any()) for t in (z, m[i], vi) if t is not None):
                raise NaNAggregationError("input", "NaN in the previous model or in the optimiser state")
            acc = None
            for k, (r, c) in enumerate(zip(self.rows, coef)):
                x = r[i].to(torch.float64)
                if torch.isnan(x).any():
                    raise NaNAggregationError("input", f"NaN in client update(s) at table rows {[k]}", [k])
                p = (x - z) * c
                acc = p if acc is None else acc + p
            if torch.isnan(acc).any():
                raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
            delta = acc / divisor
            m_new, v_new, u = server_opt_update(mode, delta, m[i], vi, *hyper)
            out = z + u
            if any(bool(torch.isnan(t).any()) for t in (out, m_new, v_new) if t is not None):
                raise NaNAggregationError("result", "NaN after the optimiser step (e.g. inf / inf)")
            m_out[i].copy_(m_new)
            if v_new is not None:
                v_out[i].copy_(v_new)
            outs.append(out.to(out_dtype))
        return outs


class _GpuOptRound(_GpuRound):
    def opt_step(self, coef: list[float], divisor: float, point: list[torch.Tensor], m: list[torch.Tensor],
                 v: list[torch.Tensor] | None, m_out: list[torch.Tensor], v_out: list[torch.Tensor] | None,
                 out_dtype: torch.dtype, mode: str, hyper: tuple[float, ...]) -> list[torch.Tensor]:
        outs, flat_outs = self._outputs(out_dtype)
        if self.native is not None:
            def flat(ts: list[torch.Tensor] | None) -> list[torch.Tensor] | None:
                return None if ts is None else self._flat(ts)

            lr, beta1, _, beta2, _, tau = hyper
            self.ctx.server_opt_step(self.table, self.dt, coef, divisor, flat(point), flat(m), flat(v), flat(m_out),
                                     flat(v_out), flat_outs, out_dtype, mode=mode, lr=lr, beta1=beta1, beta2=beta2,
                                     tau=tau)
        return outs


class ServerOptFedAVGAlgorithm(DenseRoundAlgorithm):
    """``optimizer`` is ``"avgm"``, ``"adagrad"``, ``"yogi"`` or ``"adam"``; ``learning_rate`` the
    server's step size (``None``: 1.0 for ``"avgm"``; the adaptive optimisers have no default);
    ``beta1``, ``beta2`` in [0, 1); ``tau`` the adaptivity (finite, > 0); ``initial_second_moment`` the
    value ``v`` starts from (``None``: ``tau ** 2``); ``weighted``: the clients' own
    ``aggregation_weight`` instead of 1.0 each; ``out_dtype`` float64 or float32 (that result rounded
    to nearest even); ``device`` a GPU (default: the current one) or the CPU."""

    rule_subject = "The server optimisers"
    rule_verb_ending = ""
    rule_name = "centred clipping"  # the row checks, the client limit and their texts are centred clipping's
    max_clients = POINT_MAX_CLIENTS

    def __init__(self, optimizer: str, learning_rate: float | None = None, beta1: float = 0.9, beta2: float = 0.99,
                 tau: float = 1e-3, initial_second_moment: float | None = None, weighted: bool = True,
                 device: torch.device | str | None = None, out_dtype: torch.dtype = torch.float64) -> None:
        if optimizer not in SERVER_OPT_MODES:
            raise ValueError(f"optimizer must be one of {SERVER_OPT_MODES}, not {optimizer!r}")
        if learning_rate is None:
            if optimizer != "avgm":
                raise ValueError(f'learning_rate has no default for optimizer "{optimizer}": bind it '
                                 "(the paper tunes it per task)")
            learning_rate = 1.0
        _, lr, b1, omb1, b2, omb2, tau_ = check_server_opt(optimizer, learning_rate, beta1, beta2, tau)
        if initial_second_moment is None:
            initial_second_moment = tau_ * tau_
        v0 = float(initial_second_moment)
        if not (v0 >= 0 and math.isfinite(v0)):
            raise ValueError(f"initial_second_moment must be a finite number >= 0, not {initial_second_moment}")
        super().__init__(device, out_dtype)
        self.optimizer = optimizer
        self.learning_rate, self.beta1, self.beta2, self.tau = lr, b1, b2, tau_
        self._hyper = (lr, b1, omb1, b2, omb2, tau_)
        self.initial_second_moment = v0
        self.weighted = bool(weighted)
        self.last_step: ServerOptStep | None = None
        self.rounds_done = 0
        self._layout: ModelLayout | None = None  # the state's layout; None: no state yet
        self._m: list[torch.Tensor] | None = None
        self._v: list[torch.Tensor] | None = None
        self._spare: tuple[list[torch.Tensor], list[torch.Tensor] | None] | None = None

    @property
    def adaptive(self) -> bool:
        return self.optimizer != "avgm"

    # ---- the state ------------------------------------------------------------------------
    def reset_state(self) -> None:
        """Forget the moments and the round count: the next round starts from ``+0.0`` and
        ``initial_second_moment`` with whatever layout it brings."""
        self._layout = self._m = self._v = self._spare = None
        self.rounds_done = 0

    def _fresh(self, layout: ModelLayout, device: torch.device, fill: float | None) -> list[torch.Tensor]:
        if fill is None:
            return [torch.empty(s, dtype=torch.float64, device=device) for s in layout.shapes]
        return [torch.full(s, fill, dtype=torch.float64, device=device) for s in layout.shapes]

    def _state_for(self, layout: ModelLayout, device: torch.device):
        """``(m, v, spare_m, spare_v)`` on ``device`` for this round, without changing ``self``."""
        if self._layout is not None and (self._layout.names != layout.names or
                                         tuple(map(tuple, self._layout.shapes)) != tuple(map(tuple, layout.shapes))):
            raise ValueError("the round's tensors differ from the optimiser state's (names, order or shapes): "
                             "call reset_state() to start the optimiser anew")
        if self._m is None:
            m = self._fresh(layout, device, 0.0)
            v = self._fresh(layout, device, self.initial_second_moment) if self.adaptive else None
        else:
            m = [t.to(device) for t in self._m]  # a loaded checkpoint lives on the CPU until its first round
            v = [t.to(device) for t in self._v] if self._v is not None else None
        spare = self._spare
        if spare is None or any(t.device != device for t in spare[0]):
            spare =(self._fresh(layout, device, None), self._fresh(layout, device, None) if self.adaptive else None)
        return m, v, spare[0], spare[1]

    def state_dict(self) -> dict[str, Any]:
        """The optimiser's checkpoint: the moments as CPU float64 tensors by tensor name (``None``
        before the first round; ``"v"`` is ``None`` for ``"avgm"``), ``rounds_done`` and the
        hyper-parameters the state was built with."""
        def named(ts: list[torch.Tensor] | None) -> dict[str, torch.Tensor] | None:
            if ts is None or self._layout is None:
                return None
            return {n: t.detach().to("cpu", copy=True) for n, t in zip(self._layout.names, ts)}

        return {"optimizer": self.optimizer, "learning_rate": self.learning_rate, "beta1": self.beta1,
                "beta2": self.beta2, "tau": self.tau, "initial_second_moment": self.initial_second_moment,
                "weighted": self.weighted, "rounds_done": self.rounds_done, "m": named(self._m), "v": named(self._v)}

    STATE_KEYS = ("optimizer", "learning_rate", "beta1", "beta2", "tau", "initial_second_moment", "weighted",
                  "rounds_done", "m", "v")

    def load_state_dict(self, state: dict[str, Any]) -> None:
        """Restore a ``state_dict()``. Validated on the host before anything changes: the keys, the
        optimiser, ``rounds_done``, that ``m`` and ``v`` name the same tensors with the same shapes,
        that every value is finite and ``v >= 0``. The hyper-parameters stay this instance's (the
        checkpoint's are a record). The tensors move to the device in the next round."""
        if set(state) != set(self.STATE_KEYS):
            raise ValueError(f"a server optimiser checkpoint holds exactly the keys {self.STATE_KEYS}, "
                             f"not {sorted(state)}")
        if state["optimizer"] != self.optimizer:
            raise ValueError(f'the checkpoint is of optimizer "{state["optimizer"]}", not "{self.optimizer}"')
        rounds = state["rounds_done"]
        if isinstance(rounds, bool) or int(rounds) != rounds or rounds < 0:
            raise ValueError(f"rounds_done must be an integer >= 0, not {rounds!r}")
        m, v = state["m"], state["v"]
        if m is None:
            if v is not None or rounds != 0:
                raise ValueError("a checkpoint without first moments holds no second moments and no rounds")
            self.reset_state()
            return
        if (v is not None) != self.adaptive:
            raise ValueError(f'optimizer "{self.optimizer}" ' + ("needs" if self.adaptive else "keeps no") +
                             " second moments")
        if v is not None and list(v) != list(m):
            raise ValueError("the first and the second moments name different tensors")
        new_m, new_v = [], []
        for name, t in m.items():
            groups = [("m", t, new_m)] + ([("v", v[name], new_v)] if v is not None else [])
            for what, x, dst in groups:
                if not isinstance(x, torch.Tensor) or tuple(x.shape) != tuple(t.shape):
                    raise ValueError(f"{what}[{name}]: a tensor of shape {tuple(t.shape)} is required")
                x = x.detach().to("cpu", torch.float64, copy=True)
                if not bool(torch.isfinite(x).all()):
                    raise ValueError(f"{what}[{name}] holds a value that is not finite")
                if what == "v" and bool((x < 0).any()):
                    raise ValueError(f"v[{name}] holds a negative value")
                dst.append(x)
        self._layout = ModelLayout(names=tuple(m), shapes=tuple(tuple(t.shape) for t in m.values()))
        self._m, self._v, self._spare = new_m, (new_v if v is not None else None), None
        self.rounds_done = int(rounds)

    # ---- end of round ---------------------------------------------------------------------
    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        coef = self._alphas(ids)
        W = 0.0
        for c in coef:
            W = W + c
        if not W > 0:
            raise ValueError("the clients' weights add up to 0: the pseudo-gradient is undefined")
        device = self.device
        previous = self._previous(layout, device)
        m, v, spare_m, spare_v = self._state_for(layout, device)
        work = (_GpuOptRound if device.type == "cuda" else _CpuOptRound)(layout, rows, device)
        out = work.opt_step(coef, W, work.centre(previous), m, v, spare_m, spare_v, self.out_dtype, self.optimizer,
                            self._hyper)
        work.finish()  # synchronises and raises on a NaN flag: nothing below runs for a failed round
        self._layout, self._m, self._v, self._spare = layout, spare_m, spare_v, (m, v)
        self.rounds_done += 1
        self.last_step = ServerOptStep(list(ids), coef, W, self.optimizer)
        return self._named(layout, out)
