"""OCP Microscaling (MX) compression of parameter diffs with error feedback (OCP Microscaling Formats
(MX) Specification v1.0; Rouhani et al., "Microscaling Data Formats for Deep Learning", 2023).

A block of 32 consecutive elements shares one E8M0 power-of-two scale byte and every element travels
as one FP8 E4M3 code (8.25 bits per element) or one FP4 E2M1 code (4.25 bits): deterministic, no
random stream, and a dynamic range per block where ``sign`` and QSGD have one magnitude per tensor.
``MXDelta`` is what travels: a value of ``DeltaParameterMessage.delta_parameter[name]``.
``MXFedAVGAlgorithm`` folds it as it is (``fedavg_mx_aggregate_delta``), every other algorithm gets
``to_dense()`` from the server. On a GPU the client step is ``fedavg_mx_compress``:
all tensors of a diff in one launch; host tensors, and dicts that mix dtypes or devices, go through a
numpy composition of the same contract, which gives the same bits and is the kernel's oracle.
``MXErrorFeedback`` keeps the residuals and ``MXEndpoint`` puts the step in front of a client endpoint.
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

BLOCK = 32
FORMATS = {"mxfp8": _native.MXFP8, "mxfp4": _native.MXFP4}
# per format: mantissa bits, the exponent of the smallest normal, emax of the scale rule, the largest value
_ELEMENT = {"mxfp8": (3, -6, 8, 448.0), "mxfp4": (1, 0, 2, 6.0)}


def _blocks(numel: int) -> int:
    return (numel + BLOCK - 1) // BLOCK


def code_bytes(numel: int, fmt: str) -> int:
    """The byte size of a ``numel``-element tensor's codes: whole blocks, one byte (FP8) or one
    nibble (FP4) per element."""
    return _blocks(numel) * (BLOCK if fmt == "mxfp8" else BLOCK // 2)


def _code_values(fmt: str) -> np.ndarray:
    """The fp64 value of every code of the element format (256 for E4M3, 16 for E2M1)."""
    mant, emin, _, _ = _ELEMENT[fmt]
    bits = 8 if fmt == "mxfp8" else 4
    code = np.arange(1 << bits)
    field = (code >> mant) & ((1 << (bits - 1 - mant)) - 1)
    frac = code & ((1 << mant) - 1)
    mag = np.where(field == 0, np.ldexp(frac.astype(np.float64), emin - mant),
                   np.ldexp((frac + (1 << mant)).astype(np.float64), field - 1 + emin - mant))
    if fmt == "mxfp8":
        mag[code & 0x7F == 0x7F] = np.nan
    return np.where(code >> (bits - 1) == 1, -mag, mag)


@dataclass
class MXDelta:
    """The codes and the scale bytes of one tensor of ``shape`` in ``fmt`` ("mxfp8" or "mxfp4"), with
    ``B = ceil(numel / 32)``: ``scales`` is a uint8 tensor of ``B`` bytes, byte ``s`` standing for
    ``2^(s - 127)`` and 255 for NaN; ``codes`` is a 16-byte aligned uint8 tensor of ``32 B`` bytes
    (FP8 E4M3: element ``e`` is byte ``e``) or ``16 B`` bytes (FP4 E2M1: element ``e`` is in byte
    ``e // 2``, the even element in the low nibble). The code positions past ``numel`` are written as
    0 by the encoder and ignored by every reader. The element is ``code_value * 2^(s - 127)``."""

    codes: torch.Tensor
    scales: torch.Tensor
    shape: tuple[int, ...]
    fmt: str

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        if self.fmt not in FORMATS:
            raise ValueError(f"the format is one of {sorted(FORMATS)}, not {self.fmt!r}")
        if self.numel > INT32_MAX:
            raise ValueError(f"{self.numel} elements: an mx delta holds at most 2^31 - 1")
        need = code_bytes(self.numel, self.fmt)
        if self.codes.dtype != torch.uint8 or self.codes.dim() != 1 or self.codes.numel() != need:
            raise ValueError(f"the {self.fmt} codes of {self.numel} elements are a 1-D uint8 tensor of {need} bytes")
        if self.scales.dtype != torch.uint8 or self.scales.dim() != 1 or self.scales.numel() != _blocks(self.numel):
            raise ValueError(f"the scales of {self.numel} elements are a 1-D uint8 tensor of {_blocks(self.numel)} bytes")
        if self.codes.device != self.scales.device:
            raise ValueError("codes and scales must be on one device")

    @property
    def numel(self) -> int:
        return math.prod(self.shape)

    @property
    def device(self) -> torch.device:
        return self.codes.device

    def to(self, device: torch.device | str) -> MXDelta:
        device = torch.device(device)
        if self.codes.device == device:
            return self
        return MXDelta(self.codes.to(device), self.scales.to(device), self.shape, self.fmt)

    def to_dense(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """The dense delta: ``code_value * 2^(s - 127)`` (exact in fp64), rounded once into ``dtype``."""
        n, device = self.numel, self.codes.device
        e = torch.arange(n, device=device)
        if self.fmt == "mxfp8":
            code = self.codes[:n].to(torch.int64)
        else:
            code = (self.codes.to(torch.int64)[e >> 1] >> ((e & 1) << 2)) & 15
        value = torch.from_numpy(_code_values(self.fmt)).to(device)[code]
        s = self.scales.to(torch.int64)[e >> 5]
        scale = ((s + 896) << 52).view(torch.float64)  # 2^(s - 127), assembled: no pow whose last bit could differ
        dense = torch.where(s == 255, torch.full_like(value, float("nan")), value * scale)
        # at most 4 significant bits: the conversion is one rounding on every path torch takes
        return dense.to(dtype).view(self.shape)


def is_mx(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, MXDelta) for v in parameter.values())


def densify_parameter(parameter: Mapping[str, object]) -> dict[str, object]:
    """Every ``MXDelta`` of ``parameter`` as its dense tensor, for consumers that take none."""
    return {k: v.to_dense() if isinstance(v, MXDelta) else v for k, v in parameter.items()}


@torch.no_grad()
def _mx_compress_torch(delta: torch.Tensor, error: torch.Tensor | None = None,
                       fmt: str = "mxfp8") -> tuple[MXDelta, torch.Tensor]:
    """``mx_compress`` as a torch / numpy composition of the contract (include/fedavg_hip.h,
    ``fedavg_mx_compress``): the path of host tensors, and the oracle of the kernel."""
    from .dp import _narrow  # dp imports fedavg, which imports this package's payloads

    mant, emin, emax, vmax = _ELEMENT[fmt]
    dtype, device = delta.dtype, delta.device
    total = (delta if error is None else delta + error).detach().to("cpu").reshape(-1)
    n, B = total.numel(), _blocks(total.numel())
    t64 = np.zeros(B * BLOCK, dtype=np.float64)
    t64[:n] = total.to(torch.float64).numpy()
    if not np.isfinite(t64).all():
        raise ValueError("mx_compress: a non-finite element")
    mag = np.abs(t64)
    # the shared exponent of a block: floor(log2 amax) - emax in [-127, 127], -127 for an all-zero block
    amax = mag.reshape(B, BLOCK).max(axis=1) if B else np.zeros(0)
    _, ex = np.frexp(amax)  # amax = m * 2^ex with m in [0.5, 1)
    E = np.clip(np.where(amax > 0, ex - 1 - emax, -127), -127, 127).astype(np.int64)
    Ee = np.repeat(E, BLOCK)
    with np.errstate(over="ignore", under="ignore"):
        q = np.minimum(np.ldexp(mag, -Ee), vmax)  # saturates
    # one rounding to nearest even at the quantum of q's binade; subnormals share the quantum of emin
    _, qx = np.frexp(q)
    e = np.maximum(np.where(q > 0, qx - 1, emin), emin)
    r = np.rint(np.ldexp(q, mant - e))  # 2^(mant + 1) carries into the next binade by itself
    code = ((e - emin) << mant) + r.astype(np.int64)
    neg = np.signbit(t64)
    if fmt == "mxfp8":
        packed = (code | (neg.astype(np.int64) << 7)).astype(np.uint8)
    else:
        nibble = code | (neg.astype(np.int64) << 3)
        packed = (nibble[0::2] | (nibble[1::2] << 4)).astype(np.uint8)
    value = np.ldexp(np.where(neg, -r, r), e - mant + Ee)[:n]  # exact
    sent = _narrow(value, dtype)
    residual = (total - sent).view(delta.shape).to(device)
    sd = MXDelta(torch.from_numpy(packed).to(device), torch.from_numpy((E + 127).astype(np.uint8)).to(device),
                 tuple(delta.shape), fmt)
    return sd, residual


def _for_kernel(delta: torch.Tensor, error: torch.Tensor | None) -> bool:
    """The kernel takes a non-empty floating tensor on a GPU of at most 2^31 - 1 elements, with a
    residual (if any) of its own shape, dtype and device; the composition takes everything else."""
    return (delta.device.type == "cuda" and delta.dtype in VALUE_DTYPES and 0 < delta.numel() <= INT32_MAX
            and (error is None or (error.shape == delta.shape and error.dtype == delta.dtype
                                   and error.device == delta.device)))


@torch.no_grad()
def _mx_compress_kernel(deltas: list[torch.Tensor], errors: list[torch.Tensor | None],
                        fmt: str) -> list[tuple[MXDelta, torch.Tensor]]:
    """One ``fedavg_mx_compress`` call over tensors of one dtype on one GPU."""
    from .sign import _context  # the layout-free context of a device, shared with the sign step

    device = deltas[0].device
    flat = [d.detach().contiguous().reshape(-1) for d in deltas]
    err = [None if e is None else e.detach().contiguous().reshape(-1) for e in errors]
    codes = [torch.empty(code_bytes(f.numel(), fmt), dtype=torch.uint8, device=device) for f in flat]
    scales = [torch.empty(_blocks(f.numel()), dtype=torch.uint8, device=device) for f in flat]
    res = [torch.empty_like(f) for f in flat]
    ctx = _context(device)
    ctx.mx_compress(flat, err, codes, scales, res, fmt)
    if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
        ctx.reset()  # the flag is sticky until reset: the context stays usable
        raise ValueError("mx_compress: a non-finite element")
    return [(MXDelta(c, s, tuple(d.shape), fmt), r.view(d.shape)) for d, c, s, r in zip(deltas, codes, scales, res)]


def _check_format(fmt: str) -> None:
    if fmt not in FORMATS:
        raise ValueError(f"the format is one of {sorted(FORMATS)}, not {fmt!r}")


def mx_compress(delta: torch.Tensor, error: torch.Tensor | None = None,
                fmt: str = "mxfp8") -> tuple[MXDelta, torch.Tensor]:
    """One ``ErrorFeedbackWorker`` step with MX as the compressor: ``total = delta + error`` (rounded
    once into the dtype); per block of 32 the shared exponent ``E = floor(log2 amax) - emax`` clamped
    to [-127, 127]; every element ``total / 2^E`` rounded once to nearest even into FP8 E4M3
    (``fmt="mxfp8"``) or FP4 E2M1 (``"mxfp4"``), saturating, the sign bit kept; and ``residual =
    total - sent`` (rounded once). Returns the ``MXDelta`` and the new residual. A floating tensor on
    a GPU goes through ``fedavg_mx_compress``, which gives the same bits. A
    non-finite element is a ``ValueError``."""
    _check_format(fmt)
    if delta.dtype not in VALUE_DTYPES:
        raise TypeError(f"mx compression takes fp32, fp16, bf16 and fp64 tensors, not {delta.dtype}")
    if _for_kernel(delta, error):
        return _mx_compress_kernel([delta], [error], fmt)[0]
    return _mx_compress_torch(delta, error, fmt)


def mx_compress_parameter(delta: Mapping[str, torch.Tensor], error: Mapping[str, torch.Tensor] | None = None,
                          fmt: str = "mxfp8") -> tuple[dict[str, MXDelta], dict[str, torch.Tensor]]:
    """``mx_compress`` per tensor of a parameter diff (a name that ``error`` lacks has no residual
    yet). Returns the mx deltas and the new residuals, both by name. Tensors of one floating dtype on
    one GPU go through one ``fedavg_mx_compress`` call; host tensors, empty tensors, mixed dtypes and
    dicts spread over several devices go tensor by tensor. A non-floating tensor is a ``TypeError``."""
    _check_format(fmt)
    items = list(delta.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in VALUE_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: mx compression takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
    errors = [None if error is None else error.get(name) for name, _ in items]
    results: list[Any] = [None] * len(items)
    fit = [k for k, ((_, v), e) in enumerate(zip(items, errors)) if _for_kernel(v, e)]
    if fit and len({items[k][1].device for k in fit}) == 1 and len({items[k][1].dtype for k in fit}) == 1:
        for k, r in zip(fit, _mx_compress_kernel([items[k][1] for k in fit], [errors[k] for k in fit], fmt)):
            results[k] = r
    for k, ((_, v), e) in enumerate(zip(items, errors)):
        if results[k] is None:
            results[k] = mx_compress(v, e, fmt)
    return ({name: r[0] for (name, _), r in zip(items, results)},
            {name: r[1] for (name, _), r in zip(items, results)})


class MXErrorFeedback:
    """The ``_sparsify`` step of the reference's ``ErrorFeedbackWorker`` with MX as the scheme, and
    its ``_get_error`` / ``_set_error`` state: one residual per tensor name, added to the next
    round's diff before its codes go out."""

    def __init__(self, fmt: str = "mxfp8") -> None:
        _check_format(fmt)
        self.fmt = fmt
        self._error: dict[str, torch.Tensor] = {}

    def error(self, name: str) -> torch.Tensor | None:
        """The residual kept for ``name``, or ``None`` before its first round."""
        return self._error.get(name)

    def reset(self) -> None:
        self._error.clear()

    def compress(self, message: Any) -> Any:
        """A new message of the class of ``message`` (a ``DeltaParameterMessage``) whose floating
        tensors travel as ``MXDelta``; every other field is copied, every other value of
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
        sent, residual = mx_compress_parameter(dense, self._error, self.fmt)
        self._error.update(residual)
        return dataclasses.replace(
            message, delta_parameter={n: sent.get(n, v) for n, v in message.delta_parameter.items()})


class MXEndpoint:
    """Wraps a client endpoint (any object with ``send(data)``): a ``DeltaParameterMessage`` goes out
    compressed by the endpoint's ``MXErrorFeedback`` in ``fmt``, everything else unchanged. Every
    other attribute is the wrapped endpoint's. Without an ``endpoint`` the keyword arguments build the
    simulator's ``ClientEndpoint``, which is how ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, endpoint: Any = None, fmt: str = "mxfp8", **kwargs: Any) -> None:
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.feedback = MXErrorFeedback(fmt)

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def send(self, data: Any) -> None:
        self._endpoint.send(self.feedback.compress(data) if is_delta_message(data) else data)
