"""1-bit sign compression of parameter diffs with error feedback (EF-signSGD: Karimireddy, Rebjock,
Stich, Jaggi, "Error Feedback Fixes SignSGD and other Gradient Compression Schemes", ICML 2019).

The reference's ``worker/error_feedback_worker.py`` (``ErrorFeedbackWorker``) leaves ``_sparsify``
abstract; ``sparse.topk_sparsify`` is one scheme, this is the other one people reach for: a client
sends the sign of every element of ``p = delta + error`` and one magnitude per tensor, ``‖p‖₁ / d``,
and keeps ``p - sent`` as the next round's residual. ``SignDelta`` is what travels: a value of
``DeltaParameterMessage.delta_parameter[name]``, 32 times smaller than fp32 and with no indices.
``SignFedAVGAlgorithm`` folds it as it is (``fedavg_sign_aggregate_delta``), every other algorithm
gets ``to_dense()`` from the server. On a GPU the client step is ``fedavg_sign_compress`` (DESIGN.md
§5w): all tensors of a diff in three launches; host tensors, and dicts that mix dtypes or devices, go
through a torch composition of the same contract, which gives the same bits and is the kernel's
oracle. ``SignErrorFeedback`` keeps the residuals and ``SignEndpoint`` puts the step in front of a
client endpoint.
"""

from __future__ import annotations

import dataclasses
import math
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from . import _native
from .message import is_delta_message
from .sparse import INT32_MAX, VALUE_DTYPES

_TAGS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.float64: "f64"}
_INT_VIEWS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16,
              torch.float64: torch.int64}


def bit_bytes(numel: int) -> int:
    """The byte size of a ``numel``-element tensor's sign bits: whole 64-bit words."""
    return 8 * ((numel + 63) // 64)


@dataclass
class SignDelta:
    """The signs and the magnitude of one tensor of ``shape``: ``bits`` is a uint8 tensor of
    ``8 * ceil(numel / 64)`` bytes, 8-byte aligned, element ``e`` being bit ``e % 8`` of byte
    ``e // 8`` (``numpy.packbits(..., bitorder="little")``; on the GPU bit ``e % 64`` of 64-bit word
    ``e // 64``); the bits past ``numel`` are written as 0 by the encoder and ignored by every
    reader. ``scale`` is a 0-dim tensor of the diff's dtype (float32 / float16 / bfloat16 / float64)
    on the device of ``bits``. The element is ``-scale`` where its bit is set, ``+scale`` elsewhere."""

    bits: torch.Tensor
    scale: torch.Tensor
    shape: tuple[int, ...]

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        if self.numel > INT32_MAX:
            raise ValueError(f"{self.numel} elements: a sign delta holds at most 2^31 - 1")
        if self.bits.dtype != torch.uint8 or self.bits.dim() != 1 or self.bits.numel() != bit_bytes(self.numel):
            raise ValueError(f"the bits of {self.numel} elements are a 1-D uint8 tensor of {bit_bytes(self.numel)} bytes")
        if self.scale.dim() != 0 or self.scale.dtype not in VALUE_DTYPES:
            raise ValueError("the scale is a 0-dim float32 / float16 / bfloat16 / float64 tensor")
        if self.bits.device != self.scale.device:
            raise ValueError("bits and scale must be on one device")

    @property
    def numel(self) -> int:
        return math.prod(self.shape)

    @property
    def dtype(self) -> torch.dtype:
        return self.scale.dtype

    @property
    def device(self) -> torch.device:
        return self.bits.device

    def to(self, device: torch.device | str) -> SignDelta:
        device = torch.device(device)
        if self.bits.device == device:
            return self
        return SignDelta(self.bits.to(device), self.scale.to(device), self.shape)

    def to_dense(self) -> torch.Tensor:
        """The dense delta: ``-scale`` where the bit is set, ``+scale`` elsewhere, in the scale's dtype."""
        e = torch.arange(self.numel, device=self.bits.device)
        byte = self.bits.to(torch.int32)[e >> 3]
        neg = ((byte >> (e & 7).to(torch.int32)) & 1).bool()
        return torch.where(neg, -self.scale, self.scale).view(self.shape)


def is_sign(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, SignDelta) for v in parameter.values())


def densify_parameter(parameter: Mapping[str, object]) -> dict[str, object]:
    """Every ``SignDelta`` of ``parameter`` as its dense tensor, for consumers that take none."""
    return {k: v.to_dense() if isinstance(v, SignDelta) else v for k, v in parameter.items()}


def _pack(neg: torch.Tensor) -> torch.Tensor:
    """A flat bool tensor as little-endian bits in whole 64-bit words; the padding bits are 0."""
    padded = torch.zeros(bit_bytes(neg.numel()) * 8, dtype=torch.int32, device=neg.device)
    padded[: neg.numel()] = neg
    place = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=neg.device)
    return (padded.view(-1, 8) * place).sum(dim=1).to(torch.uint8)


@torch.no_grad()
def _sign_compress_torch(delta: torch.Tensor, error: torch.Tensor | None = None) -> tuple[SignDelta, torch.Tensor]:
    """``sign_compress`` as a torch composition of the contract (include/fedavg_hip.h,
    ``fedavg_sign_compress``): the path of host tensors, and the oracle of the kernel."""
    from .dp import _lanes_then_tree, _narrow, _piece_partials  # dp imports fedavg, which imports this package's payloads

    dtype = delta.dtype
    total = (delta if error is None else delta + error).detach().reshape(-1)
    n = total.numel()
    if n == 0:
        return (SignDelta(torch.empty(0, dtype=torch.uint8, device=delta.device),
                          torch.zeros((), dtype=dtype, device=delta.device), tuple(delta.shape)),
                total.clone().view(delta.shape))
    a = total.abs().to(device="cpu", dtype=torch.float64).contiguous().numpy()
    if not np.isfinite(a).all():
        raise ValueError("sign_compress: a non-finite element")
    group = _native.kernel_constant(f"dp_ae_{_TAGS[dtype]}")
    S = _lanes_then_tree(_piece_partials(a.reshape(1, -1), group), _native.kernel_constant("dp_threads"))[0]
    s64 = np.float64(S) / np.float64(n)
    scale = _narrow(np.array([s64], dtype=np.float64), dtype)[0].to(delta.device)
    neg = total.view(_INT_VIEWS[dtype]) < 0  # the sign bit: -0.0 has it
    sent = torch.where(neg, -scale, scale)
    residual = total - sent
    return SignDelta(_pack(neg), scale, tuple(delta.shape)), residual.view(delta.shape)


_contexts: dict[torch.device, Any] = {}


def _context(device: torch.device) -> Any:
    ctx = _contexts.get(device)
    if ctx is None:
        from .fedavg import FedAvgContext, ModelLayout  # fedavg imports this module

        # the step does not depend on a context's layout: a one-element layout carries the device,
        # the stream order, the flag words and the call's workspace
        ctx = _contexts[device] = FedAvgContext(ModelLayout.flat(1, "sign"), device)
    return ctx


def _for_kernel(delta: torch.Tensor, error: torch.Tensor | None) -> bool:
    """The kernel takes a non-empty floating tensor on a GPU of at most 2^31 - 1 elements, with a
    residual (if any) of its own shape, dtype and device; the torch composition takes everything else."""
    return (delta.device.type == "cuda" and delta.dtype in VALUE_DTYPES and 0 < delta.numel() <= INT32_MAX
            and (error is None or (error.shape == delta.shape and error.dtype == delta.dtype
                                   and error.device == delta.device)))


@torch.no_grad()
def _sign_compress_kernel(deltas: list[torch.Tensor],
                          errors: list[torch.Tensor | None]) -> list[tuple[SignDelta, torch.Tensor]]:
    """One ``fedavg_sign_compress`` call over tensors of one dtype on one GPU."""
    device, dtype = deltas[0].device, deltas[0].dtype
    flat = [d.detach().contiguous().reshape(-1) for d in deltas]
    err = [None if e is None else e.detach().contiguous().reshape(-1) for e in errors]
    bits = [torch.empty(bit_bytes(f.numel()), dtype=torch.uint8, device=device) for f in flat]
    scales = [torch.empty((), dtype=dtype, device=device) for _ in flat]
    res = [torch.empty_like(f) for f in flat]
    ctx = _context(device)
    ctx.sign_compress(flat, err, bits, scales, res)
    if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
        ctx.reset()  # the flag is sticky until reset: the context stays usable
        raise ValueError("sign_compress: a non-finite element")
    return [(SignDelta(b, s, tuple(d.shape)), r.view(d.shape)) for d, b, s, r in zip(deltas, bits, scales, res)]


def sign_compress(delta: torch.Tensor, error: torch.Tensor | None = None) -> tuple[SignDelta, torch.Tensor]:
    """One ``ErrorFeedbackWorker`` step with the scaled sign as the compressor: ``total = delta +
    error`` (rounded once into the dtype), ``scale = mean |total|`` (an fp64 sum in the pinned order
    of ``fedavg_dp_noise``, divided by the element count, rounded once into the dtype), one sign bit
    per element (``-0.0`` sends ``-scale``), and ``residual = total - sent`` (rounded once). Returns
    the ``SignDelta`` and the new residual. A floating tensor on a GPU goes through
    ``fedavg_sign_compress``, which gives the same bits; an empty tensor has scale
    ``+0.0`` and no bits. A non-finite element is a ``ValueError``."""
    if delta.dtype not in VALUE_DTYPES:
        raise TypeError(f"sign compression takes fp32, fp16, bf16 and fp64 tensors, not {delta.dtype}")
    if _for_kernel(delta, error):
        return _sign_compress_kernel([delta], [error])[0]
    return _sign_compress_torch(delta, error)


def sign_compress_parameter(delta: Mapping[str, torch.Tensor], error: Mapping[str, torch.Tensor] | None = None,
                            ) -> tuple[dict[str, SignDelta], dict[str, torch.Tensor]]:
    """``sign_compress`` per tensor of a parameter diff (a name that ``error`` lacks has no residual
    yet). Returns the sign deltas and the new residuals, both by name. Tensors of one floating dtype
    on one GPU go through one ``fedavg_sign_compress`` call; host tensors, empty tensors, mixed
    dtypes and dicts spread over several devices go tensor by tensor. A non-floating tensor is a
    ``TypeError``."""
    items = list(delta.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in VALUE_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: sign compression takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
    errors = [None if error is None else error.get(name) for name, _ in items]
    results: list[Any] = [None] * len(items)
    fit = [k for k, ((_, v), e) in enumerate(zip(items, errors)) if _for_kernel(v, e)]
    if fit and len({items[k][1].device for k in fit}) == 1 and len({items[k][1].dtype for k in fit}) == 1:
        for k, r in zip(fit, _sign_compress_kernel([items[k][1] for k in fit], [errors[k] for k in fit])):
            results[k] = r
    for k, ((_, v), e) in enumerate(zip(items, errors)):
        if results[k] is None:
            results[k] = sign_compress(v, e)
    return ({name: r[0] for (name, _), r in zip(items, results)},
            {name: r[1] for (name, _), r in zip(items, results)})


class SignErrorFeedback:
    """The ``_sparsify`` step of the reference's ``ErrorFeedbackWorker`` with the scaled sign as the
    scheme, and its ``_get_error`` / ``_set_error`` state: one residual per tensor name, added to the
    next round's diff before its signs go out."""

    def __init__(self) -> None:
        self._error: dict[str, torch.Tensor] = {}

    def error(self, name: str) -> torch.Tensor | None:
        """The residual kept for ``name``, or ``None`` before its first round."""
        return self._error.get(name)

    def reset(self) -> None:
        self._error.clear()

    def compress(self, message: Any) -> Any:
        """A new message of the class of ``message`` (a ``DeltaParameterMessage``) whose floating
        tensors travel as ``SignDelta``; every other field is copied, every other value of
        ``delta_parameter`` passes unchanged. Keeps the new residuals. ``ValueError`` for a name
        whose shape or dtype changed."""
        dense = {n: v for n, v in message.delta_parameter.items()
                 if isinstance(v, torch.Tensor) and v.dtype in VALUE_DTYPES}
        for name, value in dense.items():
            e = self._error.get(name)
            if e is not None and (e.shape != value.shape or e.dtype != value.dtype):
                raise ValueError(f"{name}: {tuple(value.shape)} {value.dtype} now, {tuple(e.shape)} {e.dtype} in the "
                                 "round before: reset() the residuals of a changed model")
            if e is not None and e.device != value.device:
                self._error[name] = e.to(value.device)
        sent, residual = sign_compress_parameter(dense, self._error)
        self._error.update(residual)
        return dataclasses.replace(
            message, delta_parameter={n: sent.get(n, v) for n, v in message.delta_parameter.items()})


class SignEndpoint:
    """Wraps a client endpoint (any object with ``send(data)``): a ``DeltaParameterMessage`` goes out
    compressed by the endpoint's ``SignErrorFeedback``, everything else unchanged. Every other
    attribute is the wrapped endpoint's. Without an ``endpoint`` the keyword arguments build the
    simulator's ``ClientEndpoint``, which is how ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, endpoint: Any = None, **kwargs: Any) -> None:
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.feedback = SignErrorFeedback()

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def send(self, data: Any) -> None:
        self._endpoint.send(self.feedback.compress(data) if is_delta_message(data) else data)
