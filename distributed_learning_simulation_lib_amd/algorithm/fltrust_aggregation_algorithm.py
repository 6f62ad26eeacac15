"""FLTrust (Cao, Fang, Liu, Gong, "FLTrust: Byzantine-robust Federated Learning via Trust
Bootstrapping", NDSS 2021): every client is scored by the cosine between its update and the update
the server itself trained on a small root dataset, negative cosines score 0, every update is rescaled
to the root update's norm, and the result is the score-weighted mean. The dots and the norms come
from one GPU pass over the client bytes and the step is the fold about a point.

NOT an algorithm of the reference (it aggregates with the weighted mean only): like the other robust
rules it is built on the data path the FedAvg reduce already owns. With ``v`` the previous global
model, an update is ``x_i - v``; the dot of every client's update with the root's and its squared
norm are ``fedavg_moments_about_point``; the step ``v + (sum_i c_i (x_i - v)) / W`` is
``fedavg_fold_about_point``. The contract (``tests/trust_reference.py`` restates it
independently):

1. The ``n`` clients of the round that were not skipped (``None``) count, in arrival order; every
   one of them must hold every tensor of the layout with the same shape (a ``ValueError`` names the
   client and the key). The root worker is one of them: its "update" is the server's own, trained on
   the root dataset. At most 1024 clients.
2. Finite screen, as the geometric median's: ``N_i = sum_e x_i[e]^2``. A NaN input raises
   ``NaNAggregationError`` (stage ``input``) naming the clients. A client with ``N_i = +inf`` is
   *dropped* for the round.
3. The root worker absent from the round, skipped or dropped by the screen: ``ValueError``. A root
   update of squared norm 0 (``S_root = 0``, step 6) gives no direction: ``ValueError``.
4. The centre ``v`` is the model given to ``set_old_parameter``, converted to float64 and moved to
   the device once per round (never set, or its keys or shapes differ from the layout: the
   ``ValueError`` of ``DenseRoundAlgorithm._previous`` names the key).
5. The direction is ``g = x_root.to(float64) - v``: one IEEE subtract per element.
6. ``T_i = sum_e (x_i[e] - v[e]) * g[e]`` and ``S_i = sum_e (x_i[e] - v[e])^2`` over the kept clients,
   the root among them, in one ``moments_about_point`` call: per element ``d = x - v``,
   ``q = d * d``, ``p = d * g``, ``S = S + q``, ``T = T + p``, five separately rounded float64
   operations in the pinned order of §5i. The root's own ``S`` is ``root_sqnorm``. A NaN in the
   centre raises ``NaNAggregationError`` (stage ``input``); a NaN moment (stage ``accumulator``)
   needs ``inf - inf`` or ``0 * inf``, which the screen leaves no way to. An infinity in the centre
   makes every squared norm ``+inf``: every client is distrusted and step 7 raises.
7. ``(score, coef) = rules.trust_coefficients(T, S, root_sqnorm)``: ``n0 = sqrt(root_sqnorm)``,
   ``ni = sqrt(S_i)``, ``den = ni * n0``; ``S_i`` not finite or ``den == 0``: distrusted (0.0, 0.0);
   otherwise ``cos = T_i / den``, ``score = cos if cos > 0 else 0.0``,
   ``coef = score * (n0 / ni)``. ``W`` is the sum of the non-root scores, added in arrival order;
   ``W == 0``: ``ValueError`` ("no client is trusted").
8. The root is removed from the table. The result is one ``fold_about_point(coef, W, v)`` over the
   remaining clients: per element ``d_i = x_i - v``, ``p_i = coef_i * d_i``, ``acc = p_0 + p_1 + ...``
   in arrival order, ``r = acc / W``, ``out = v + r``, written in ``out_dtype`` (float32: that
   float64 result rounded to nearest even).
9. ``last_trust`` records the round.
10. On a CPU ``device`` the same rule runs in torch (``moments_about_point_cpu`` and centred
    clipping's loop over the clients), so the class returns the same bits on the CPU and on the GPU.

The rule tolerates a majority of malicious clients, as long as the root update is honest. Limits: at
most 1024 clients, dense full updates only — delta and quantised payloads are refused
(``accepts_delta_messages`` / ``accepts_quantized_messages`` stay false, so this package's server
restores or dequantises before handing an update over).
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from ..fedavg import ModelLayout, NaNAggregationError
from .._native import POINT_MAX_CLIENTS
from ..message import ModelParameter
from ..rules import trust_coefficients
from .dense_round import _DTYPE_TAGS, DenseRoundAlgorithm, _CpuRound, _GpuRound, finite_screen

# the kernel's geometry where the native library cannot be asked (§5i's)
TRUST_DEFAULTS = {"trust_chunk": 4096, "trust_threads": 256,
                  "trust_ae_f32": 4, "trust_ae_f16": 8, "trust_ae_bf16": 8, "trust_ae_f64": 2}


class TrustRecord(NamedTuple):
    """What the last round did: the counted workers in arrival order, the ids dropped by the finite
    screen, the kept workers in arrival order (the root among them) and, per kept worker, its dot
    with the root direction, its squared norm about the centre, its trust score and its
    coefficient. The root's own score and coefficient are recorded and not used: it is not averaged."""

    worker_ids: list[int]
    dropped: list[int]
    kept: list[int]
    root_worker: int
    dots: list[float]
    sqnorms: list[float]
    scores: list[float]
    coefficients: list[float]
    total_score: float


def trust_constants(dtype: torch.dtype) -> tuple[int, int, int]:
    """(chunk, threads, ae) of ``fedavg_moments_about_point`` for a client dtype: from the native
    library, or the documented defaults where it is not built."""
    names = ("trust_chunk", "trust_threads", f"trust_ae_{_DTYPE_TAGS[dtype]}")
    try:
        from .._native import kernel_constant

        return tuple(kernel_constant(n) for n in names)  # type: ignore[return-value]
    except (ImportError, OSError):
        return tuple(TRUST_DEFAULTS[n] for n in names)  # type: ignore[return-value]


def moments_about_point_cpu(rows: list[list[torch.Tensor]], centre: list[torch.Tensor] | None,
                            direction: list[torch.Tensor], chunk: int | None = None, threads: int | None = None,
                            ae: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``fedavg_moments_about_point`` in torch, in the kernel's pinned order:
    ``rows[i]`` are client i's tensors in layout order (one dtype), ``centre`` one float64 tensor per
    tensor or ``None`` for the origin, ``direction`` one float64 tensor per tensor. Per element
    ``d = x - v``, ``q = d * d``, ``p = d * g``; every segment is cut into chunks of ``chunk``
    elements, padded with +0.0; lane ``l`` of ``threads`` adds the positions
    ``(k * threads + l) * ae + i`` in ascending order into one accumulator per sum; the 64 lanes of a
    wave are combined by the halving tree (off = 32 .. 1), the waves in wave order, the chunks
    sequentially from +0.0 in layout order. Returns ``(dots, sqnorms)``; raises
    ``NaNAggregationError`` like the kernel's flags."""
    n = len(rows)
    if chunk is None or threads is None or ae is None:
        dt = rows[0][0].dtype if rows and rows[0] else torch.float64
        c, th, a = trust_constants(dt if dt in _DTYPE_TAGS else torch.float64)
        chunk, threads, ae = chunk or c, threads or th, ae or a
    per_lane = chunk // (threads * ae)
    assert per_lane >= 1 and per_lane * threads * ae == chunk and threads % 64 == 0
    x = [[t.to(torch.float64).reshape(-1) for t in r] for r in rows]
    bad = [i for i in range(n) if any(bool(torch.isnan(t).any()) for t in x[i])]
    if bad:
        raise NaNAggregationError("input", f"NaN in client update(s) at rows {bad}", bad)
    if centre is not None and any(bool(torch.isnan(z).any()) for z in centre):
        raise NaNAggregationError("input", "NaN in the centre")
    if any(bool(torch.isnan(z).any()) for z in direction):
        raise NaNAggregationError("input", "NaN in the direction")
    out = torch.zeros((2, n), dtype=torch.float64)
    for s in range(len(x[0]) if n else 0):
        X = torch.stack([x[i][s] for i in range(n)])
        numel = X.shape[1]
        if numel == 0:
            continue
        d = X if centre is None else X - centre[s].to(torch.float64).reshape(-1)
        nch = (numel + chunk - 1) // chunk
        terms = torch.stack([d * direction[s].to(torch.float64).reshape(-1), d * d])  # [2][n][numel]
        terms = torch.nn.functional.pad(terms, (0, nch * chunk - numel)).reshape(2, n, nch, per_lane, threads, ae)
        acc = torch.zeros((2, n, nch, threads), dtype=torch.float64, device=terms.device)
        for k in range(per_lane):
            for i in range(ae):
                acc = acc + terms[:, :, :, k, :, i]
        a = acc.reshape(2, n, nch, threads // 64, 64)
        off = 32
        while off >= 1:
            a = a[..., :off] + a[..., off:2 * off]
            off //= 2
        part = a[..., 0, 0]
        for w in range(1, threads // 64):
            part = part + a[..., w, 0]
        part = part.cpu()
        for c in range(nch):
            out = out + part[:, :, c]
    if torch.isnan(out).any():
        raise NaNAggregationError("accumulator",
                                  "NaN in a moment about the point (inf - inf, 0 * inf or +inf + -inf)")
    return out[0], out[1]


class _CpuTrustRound(_CpuRound):
    def __init__(self, layout: ModelLayout, rows: list[list[torch.Tensor]], device: torch.device) -> None:
        super().__init__(layout, rows, device)
        self.all_rows = self.rows

    def keep(self, kept: list[int]) -> None:  # indices of the round's rows, as on the GPU
        self.rows = [self.all_rows[k] for k in kept]

    def direction(self, root: int, centre: list[torch.Tensor]) -> list[torch.Tensor]:
        return [x.to(torch.float64) - z for x, z in zip(self.all_rows[root], centre)]

    def moments(self, centre: list[torch.Tensor], direction: list[torch.Tensor]) -> tuple[list[float], list[float]]:
        T, S = moments_about_point_cpu(self.rows, centre, direction)
        return T.tolist(), S.tolist()


class _GpuTrustRound(_GpuRound):
    def direction(self, root: int, centre: list[torch.Tensor]) -> list[torch.Tensor]:
        out = [torch.empty(s, dtype=torch.float64, device=self.device) for s in self.layout.shapes]
        if self.native is not None:
            T = len(self.segments)
            for j, i in enumerate(self.segments):
                out[i] = (self.flat[root * T + j].to(torch.float64) - centre[i]).contiguous()
        return out

    def moments(self, centre: list[torch.Tensor], direction: list[torch.Tensor]) -> tuple[list[float], list[float]]:
        if self.native is None:
            return [0.0] * self.n, [0.0] * self.n
        T, S = self.ctx.moments_about_point(self.table, self.dt, self._flat(centre), self._flat(direction))
        T, S = T.cpu(), S.cpu()  # the copy synchronises: the flags are final
        self.ctx.raise_on_nan([(self.table, self.dt)])
        return T.tolist(), S.tolist()


class FLTrustFedAVGAlgorithm(DenseRoundAlgorithm):
    """``root_worker`` is the id of the worker whose update is the server's own, trained on the root
    dataset (no default); ``out_dtype`` float64 or float32 (that result rounded to nearest even);
    ``device`` a GPU (default: the current one) or the CPU."""

    rule_subject = rule_name = "FLTrust"
    max_clients = POINT_MAX_CLIENTS

    def __init__(self, root_worker: int, device: torch.device | str | None = None,
                 out_dtype: torch.dtype = torch.float64) -> None:
        if isinstance(root_worker, bool) or int(root_worker) != root_worker:
            raise ValueError(f"root_worker must be a worker id (an integer), not {root_worker!r}")
        super().__init__(device, out_dtype)
        self.root_worker = int(root_worker)
        self.last_trust: TrustRecord | None = None

    def _aggregate_parameter(self) -> ModelParameter:
        layout, ids, rows = self._rows()
        if self.root_worker not in ids:
            raise ValueError(f"the root worker {self.root_worker} sent no update this round: FLTrust has no direction")
        device = self.device
        previous = self._previous(layout, device)
        work = (_GpuTrustRound if device.type == "cuda" else _CpuTrustRound)(layout, rows, device)

        kept, dropped = finite_screen(work, ids)  # a client whose squared norm is +inf is dropped for the round
        if self.root_worker in dropped:
            raise ValueError(f"the root worker {self.root_worker} sent an infinite update: FLTrust has no direction")
        work.keep(kept)
        kept_ids = [ids[k] for k in kept]
        root_row = ids.index(self.root_worker)
        root_pos = kept_ids.index(self.root_worker)

        v = work.centre(previous)
        g = work.direction(root_row, v)
        dots, sqnorms = work.moments(v, g)
        root_sqnorm = sqnorms[root_pos]
        if root_sqnorm == 0:
            raise ValueError(f"the root worker {self.root_worker}'s update is the previous model itself "
                             "(squared norm 0): FLTrust has no direction")
        scores, coef = trust_coefficients(dots, sqnorms, root_sqnorm)
        W = 0.0
        for k, s in enumerate(scores):
            if k != root_pos:
                W = W + s
        if not W > 0:
            raise ValueError("no client is trusted: every trust score of the round is 0")
        work.keep([k for k in kept if k != root_row])
        out = work.step([c for k, c in enumerate(coef) if k != root_pos], W, v, self.out_dtype)
        work.finish()
        self.last_trust = TrustRecord(list(ids), dropped, kept_ids, self.root_worker, dots, sqnorms, scores, coef, W)
        return self._named(layout, out)
