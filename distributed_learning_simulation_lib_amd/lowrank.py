"""Low-rank compression of parameter diffs with error feedback (the structured low-rank updates of
Konečný et al., "Federated Learning: Strategies for Improving Communication Efficiency", 2016; the
PowerSGD compressor of Vogels, Karimireddy, Jaggi, NeurIPS 2019).

A client sends a weight matrix's diff as two thin factors: ``D ≈ L · R`` with ``L`` of ``[m, r]`` and
``R`` of ``[r, n]``, ``r ≪ min(m, n)``; a tensor of more than two dimensions is the matrix of its first
dimension against the rest. ``LowRankDelta`` is what travels: a value of
``DeltaParameterMessage.delta_parameter[name]`` of ``r (m + n)`` values instead of ``m n``.
``LowRankFedAVGAlgorithm`` folds the factors as they are (``fedavg_lowrank_aggregate_delta``, DESIGN.md
§5aa: the round's sum is one product per tensor on the fp64 matrix unit), every other algorithm gets
``to_dense()`` from the server. The client step, one power-iteration step, is
``fedavg_lowrank_compress`` on a GPU (one call and five launches for a whole diff, the
products on the fp64 matrix unit, no host round trip) and a torch composition of the same contract on
the host, which is also the kernel's oracle. ``LowRankErrorFeedback`` keeps the residuals and the
warm-start factors and ``LowRankEndpoint`` puts the step in front of a client endpoint.
"""

from __future__ import annotations

import dataclasses
import math
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Any

import torch

from . import _native
from ._native import LOWRANK_MAX_RANK
from .message import is_delta_message
from .sparse import INT32_MAX, VALUE_DTYPES


@dataclass
class LowRankDelta:
    """The factors of one tensor of ``shape``: ``left`` is a contiguous ``[m, r]`` tensor and ``right`` a
    contiguous ``[r, n]`` tensor of one dtype (float32 / float16 / bfloat16 / float64) on one device,
    with ``m = shape[0]`` and ``n = prod(shape[1:])``. It stands for ``left @ right`` reshaped to
    ``shape``."""

    left: torch.Tensor
    right: torch.Tensor
    shape: tuple[int, ...]

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        if len(self.shape) < 2:
            raise ValueError(f"a low-rank delta stands for a tensor of at least 2 dimensions, not {self.shape}")
        if self.numel > INT32_MAX:
            raise ValueError(f"{self.numel} elements: a low-rank delta holds at most 2^31 - 1")
        m, n = self.shape[0], math.prod(self.shape[1:])
        if self.left.dim() != 2 or self.right.dim() != 2 or self.left.shape[0] != m or self.right.shape[1] != n \
                or self.left.shape[1] != self.right.shape[0] or self.left.shape[1] < 1:
            raise ValueError(f"the factors of a {self.shape} tensor are [{m}, r] and [r, {n}] with r >= 1, not "
                             f"{tuple(self.left.shape)} and {tuple(self.right.shape)}")
        if self.left.dtype != self.right.dtype or self.left.dtype not in VALUE_DTYPES:
            raise ValueError("the factors share one dtype: float32 / float16 / bfloat16 / float64")
        if self.left.device != self.right.device:
            raise ValueError("the factors must be on one device")
        if not self.left.is_contiguous() or not self.right.is_contiguous():
            raise ValueError("the factors must be contiguous")

    @property
    def numel(self) -> int:
        return math.prod(self.shape)

    @property
    def rank(self) -> int:
        return int(self.left.shape[1])

    @property
    def dtype(self) -> torch.dtype:
        return self.left.dtype

    @property
    def device(self) -> torch.device:
        return self.left.device

    def to(self, device: torch.device | str) -> LowRankDelta:
        device = torch.device(device)
        if self.left.device == device:
            return self
        return LowRankDelta(self.left.to(device), self.right.to(device), self.shape)

    def to_dense(self) -> torch.Tensor:
        """The dense delta: the factors converted exactly to float64, the products added in ascending
        rank index as separately rounded float64 operations, the sum rounded to the factors' dtype."""
        L, R = self.left.to(torch.float64), self.right.to(torch.float64)
        acc = L[:, 0:1] * R[0:1, :]
        for j in range(1, self.rank):
            acc = acc + L[:, j:j + 1] * R[j:j + 1, :]
        return acc.to(self.dtype).view(self.shape)


def is_lowrank(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, LowRankDelta) for v in parameter.values())


def densify_parameter(parameter: Mapping[str, object]) -> dict[str, object]:
    """Every ``LowRankDelta`` of ``parameter`` as its dense tensor, for consumers that take none."""
    return {k: v.to_dense() if isinstance(v, LowRankDelta) else v for k, v in parameter.items()}


def _check_rank(rank: int) -> int:
    rank = int(rank)
    if not 1 <= rank <= LOWRANK_MAX_RANK:
        raise ValueError(f"the rank is in 1 .. {LOWRANK_MAX_RANK}, not {rank}")
    return rank


def _orthonormalise(P: torch.Tensor) -> torch.Tensor:
    """Modified Gram–Schmidt over the columns of ``P``, twice per column; a column that vanishes stays 0."""
    cols: list[torch.Tensor] = []
    for j in range(P.shape[1]):
        v = P[:, j]
        for _ in range(2):
            for q in cols:
                v = v - (q @ v) * q
        norm = torch.linalg.vector_norm(v)
        cols.append(v / norm if float(norm) > 0 else torch.zeros_like(v))
    return torch.stack(cols, dim=1)


def _shape(delta: torch.Tensor, rank: int) -> tuple[int, int] | None:
    """``(m, n)`` of a tensor the factors make smaller, ``None`` for one that travels dense."""
    if delta.dim() < 2:
        return None
    m, n = int(delta.shape[0]), math.prod(delta.shape[1:])
    return None if rank * (m + n) >= m * n else (m, n)


def _check_start(right_prev: torch.Tensor | None, m: int, n: int, rank: int) -> None:
    if right_prev is not None and tuple(right_prev.shape) != (rank, n):
        raise ValueError(f"the warm start of a [{m}, {n}] matrix at rank {rank} is [{rank}, {n}], not "
                         f"{tuple(right_prev.shape)}")


def _first_start(rank: int, n: int) -> torch.Tensor:
    """The start of a tensor's first round: fixed by ``n`` alone, made on the host."""
    return torch.randn(rank, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))


def _for_kernel(delta: torch.Tensor, rank: int, error: torch.Tensor | None) -> bool:
    """The kernel takes a floating tensor on a GPU that the factors make smaller, of at most 2^31 - 1
    elements, with a residual (if any) of its own shape, dtype and device; the torch composition
    takes everything else."""
    return (delta.device.type == "cuda" and delta.dtype in VALUE_DTYPES and _shape(delta, rank) is not None
            and delta.numel() <= INT32_MAX
            and (error is None or (error.shape == delta.shape and error.dtype == delta.dtype
                                   and error.device == delta.device)))


@torch.no_grad()
def _lowrank_compress_kernel(deltas: list[torch.Tensor], rank: int, starts: list[torch.Tensor | None],
                             errors: list[torch.Tensor | None]) -> list[tuple[LowRankDelta, torch.Tensor]]:
    """One ``fedavg_lowrank_compress`` call over compressible tensors of one dtype on one GPU."""
    from .sign import _context  # the layout-free context of a device, shared with the sign step

    device, dt = deltas[0].device, deltas[0].dtype
    mats, qs = [], []
    for d, q in zip(deltas, starts):
        m, n = _shape(d, rank)
        _check_start(q, m, n, rank)
        mats.append(d.detach().contiguous())
        if q is None:
            q = _first_start(rank, n).to(device)
        elif q.device != device or q.dtype not in (dt, torch.float64):
            q = q.detach().to(device=device, dtype=torch.float64)
        qs.append(q.detach().contiguous())
    errs = [None if e is None else e.detach().contiguous() for e in errors]
    lefts = [torch.empty(d.shape[0], rank, dtype=dt, device=device) for d in mats]
    rights = [torch.empty(rank, q.shape[1], dtype=dt, device=device) for q in qs]
    res = [torch.empty_like(d) for d in mats]
    ctx = _context(device)
    ctx.lowrank_compress(mats, errs, qs, lefts, rights, res)
    if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
        ctx.reset()  # the flag is sticky until reset: the context stays usable
        raise ValueError("lowrank_compress: a non-finite element")
    return [(LowRankDelta(l, r, tuple(d.shape)), e.view(d.shape)) for d, l, r, e in zip(deltas, lefts, rights, res)]


@torch.no_grad()
def lowrank_compress(delta: torch.Tensor, rank: int, right_prev: torch.Tensor | None = None,
                     error: torch.Tensor | None = None) -> tuple[LowRankDelta | torch.Tensor, torch.Tensor]:
    """One PowerSGD step (``_lowrank_compress_torch`` states it). A compressible floating tensor on a
    GPU goes through ``fedavg_lowrank_compress``: the same contract at the kernel's
    own summation order, the same bits on every run, and a non-finite element is a ``ValueError``.
    Host tensors go through the torch composition."""
    rank = _check_rank(rank)
    if delta.dtype not in VALUE_DTYPES:
        raise TypeError(f"low-rank compression takes fp32, fp16, bf16 and fp64 tensors, not {delta.dtype}")
    if _for_kernel(delta, rank, error):
        return _lowrank_compress_kernel([delta], rank, [right_prev], [error])[0]
    return _lowrank_compress_torch(delta, rank, right_prev, error)


@torch.no_grad()
def _lowrank_compress_torch(delta: torch.Tensor, rank: int, right_prev: torch.Tensor | None = None,
                            error: torch.Tensor | None = None) -> tuple[LowRankDelta | torch.Tensor, torch.Tensor]:
    """One PowerSGD step: ``M = delta + error`` as an ``[m, n]`` matrix, ``P = M Qᵀ`` with ``Q`` the
    ``right`` of the round before (``right_prev``; a fixed pseudo-random matrix without one),
    ``P`` orthonormalised by Gram–Schmidt, ``Q = Pᵀ M``; ``left = P`` and ``right = Q`` rounded into the
    diff's dtype, and the new error is ``M - left right`` of the rounded factors. The arithmetic is
    float64. A tensor with fewer than 2 dimensions, or one that the factors would not make smaller
    (``r (m + n) >= m n``), comes back dense and unchanged with a zero error."""
    rank = _check_rank(rank)
    if delta.dtype not in VALUE_DTYPES:
        raise TypeError(f"low-rank compression takes fp32, fp16, bf16 and fp64 tensors, not {delta.dtype}")
    m = int(delta.shape[0]) if delta.dim() >= 2 else 0
    n = math.prod(delta.shape[1:]) if delta.dim() >= 2 else 0
    if delta.dim() < 2 or rank * (m + n) >= m * n:
        return delta, torch.zeros_like(delta)
    M = delta.detach().reshape(m, n).to(torch.float64)
    if error is not None:
        M = M + error.detach().reshape(m, n).to(torch.float64)
    if right_prev is not None:
        if tuple(right_prev.shape) != (rank, n):
            raise ValueError(f"the warm start of a [{m}, {n}] matrix at rank {rank} is [{rank}, {n}], not "
                             f"{tuple(right_prev.shape)}")
        Q = right_prev.detach().to(device=M.device, dtype=torch.float64)
    else:
        Q = torch.randn(rank, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n)).to(M.device)
    P = _orthonormalise(M @ Q.T)
    Q = P.T @ M
    sent = LowRankDelta(P.to(delta.dtype).contiguous(), Q.to(delta.dtype).contiguous(), tuple(delta.shape))
    residual = M - sent.left.to(torch.float64) @ sent.right.to(torch.float64)
    return sent, residual.to(delta.dtype).view(delta.shape)


def lowrank_compress_parameter(delta: Mapping[str, torch.Tensor], rank: int,
                               right_prev: Mapping[str, torch.Tensor] | None = None,
                               error: Mapping[str, torch.Tensor] | None = None,
                               ) -> tuple[dict[str, LowRankDelta | torch.Tensor], dict[str, torch.Tensor]]:
    """``lowrank_compress`` per tensor of a parameter diff (a name that ``right_prev`` or ``error`` lacks
    has no warm start or residual yet). Returns what is sent and the new residuals, both by name. The
    compressible tensors of one floating dtype on one GPU go through one ``fedavg_lowrank_compress``
    call; host tensors, mixed dtypes and dicts spread over several devices go tensor by tensor. A
    non-floating tensor is a ``TypeError``."""
    rank = _check_rank(rank)
    items = list(delta.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in VALUE_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: low-rank compression takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
    starts = [None if right_prev is None else right_prev.get(name) for name, _ in items]
    errors = [None if error is None else error.get(name) for name, _ in items]
    results: list[Any] = [None] * len(items)
    fit = [k for k, ((_, v), e) in enumerate(zip(items, errors)) if _for_kernel(v, rank, e)]
    if fit and len({items[k][1].device for k in fit}) == 1 and len({items[k][1].dtype for k in fit}) == 1:
        done = _lowrank_compress_kernel([items[k][1] for k in fit], rank, [starts[k] for k in fit],
                                        [errors[k] for k in fit])
        for k, r in zip(fit, done):
            results[k] = r
    for k, ((_, v), q, e) in enumerate(zip(items, starts, errors)):
        if results[k] is None:
            results[k] = lowrank_compress(v, rank, q, e)
    return ({name: r[0] for (name, _), r in zip(items, results)},
            {name: r[1] for (name, _), r in zip(items, results)})


class LowRankErrorFeedback:
    """The ``_sparsify`` step of the reference's ``ErrorFeedbackWorker`` with the low-rank factors as the
    scheme: one residual per tensor name, added to the next round's diff, and the ``right`` factor sent
    last, which starts the next round's power iteration."""

    def __init__(self, rank: int) -> None:
        self.rank = _check_rank(rank)
        self._error: dict[str, torch.Tensor] = {}
        self._right: dict[str, torch.Tensor] = {}

    def error(self, name: str) -> torch.Tensor | None:
        """The residual kept for ``name``, or ``None`` before its first round."""
        return self._error.get(name)

    def warm_start(self, name: str) -> torch.Tensor | None:
        """The ``right`` factor last sent for ``name``, or ``None`` where none was."""
        return self._right.get(name)

    def reset(self) -> None:
        self._error.clear()
        self._right.clear()

    def compress(self, message: Any) -> Any:
        """A new message of the class of ``message`` (a ``DeltaParameterMessage``) whose floating
        matrices travel as ``LowRankDelta``; every other field is copied, every other value of
        ``delta_parameter`` passes unchanged. Keeps the new residuals and warm starts. ``ValueError``
        for a name whose shape or dtype changed."""
        dense = {n: v for n, v in message.delta_parameter.items()
                 if isinstance(v, torch.Tensor) and v.dtype in VALUE_DTYPES}
        for name, value in dense.items():
            e = self._error.get(name)
            if e is not None and (e.shape != value.shape or e.dtype != value.dtype):
                raise ValueError(f"{name}: {tuple(value.shape)} {value.dtype} now, {tuple(e.shape)} {e.dtype} in the "
                                 "round before: reset() the residuals of a changed model")
            if e is not None and e.device != value.device:
                self._error[name] = e.to(value.device)
        sent, residual = lowrank_compress_parameter(dense, self.rank, self._right, self._error)
        self._error.update(residual)
        self._right.update({n: v.right for n, v in sent.items() if isinstance(v, LowRankDelta)})
        return dataclasses.replace(
            message, delta_parameter={n: sent.get(n, v) for n, v in message.delta_parameter.items()})


class LowRankEndpoint:
    """Wraps a client endpoint (any object with ``send(data)``): a ``DeltaParameterMessage`` goes out
    compressed by the endpoint's ``LowRankErrorFeedback`` of ``rank``, everything else unchanged. Every
    other attribute is the wrapped endpoint's. Without an ``endpoint`` the keyword arguments build the
    simulator's ``ClientEndpoint``, which is how ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, endpoint: Any = None, rank: int = 4, **kwargs: Any) -> None:
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.feedback = LowRankErrorFeedback(rank)

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def send(self, data: Any) -> None:
        self._endpoint.send(self.feedback.compress(data) if is_delta_message(data) else data)
