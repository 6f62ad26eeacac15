"""Quantised client updates, dequantised inside the FedAvg fold on the GPU.

The reference can run its workers behind ``StochasticQuantClientEndpoint`` and the server behind
``StochasticQuantServerEndpoint`` (simulation_lib/topology/quantized_endpoint.py:96-111): every
parameter tensor travels QSGD-quantised at ``quantization_level=255`` (one norm per tensor, a
uint8 slot and a sign bit per element) and ``QuantServerEndpoint.get`` (:69-77) dequantises it
on the host before the FedAvg algorithm folds the dense copy (fed_avg_algorithm.py:43-64). The
same file's ``NNADQClientEndpoint`` / ``NNADQServerEndpoint`` (:114-142) do the same with the
deterministic NNADQ codec (one lo / step per tensor, a uint8 code per element).

Here the quantised tensor itself is the client operand. A ``QuantizedTensor`` is one record in
the layout of ``include/fedavg_hip.h`` (FEDAVG_QSGD_F32: a 16-byte header (norm, level), the
slots, the packed sign bits; FEDAVG_NNADQ_F32: a 32-byte header (lo, step, levels), the codes).
``FedAVGAlgorithm`` passes record pointers to the kernels with the record's input format and
the kernel folds ``round(f64(x_hat) * w)`` per element with x_hat computed in the codec's
dtype — the same value the host dequantisation would have produced — while reading about 1
byte per element instead of 4 or 8:

* QSGD: x_hat = ((norm * sign) * slot) / level;
* NNADQ: x_hat = code * step + lo.

Both codecs live in the unvendored ``cyy_torch_algorithm`` (git ``@main``, quantization.
stochastic / quantization.deterministic); they are restated here (QSGD from the published
scheme; NNADQ as a deterministic adaptive-level affine code), so parity with that package is
unpinned (``oracle/qsgd_oracle.py`` and ``oracle/nnadq_oracle.py`` say what exactly is claimed).
``stochastic_quantization`` and ``NNADQ`` below are this framework's client-side quantisers (and
host dequantisers for consumers that need dense tensors, e.g. workers receiving a quantised
broadcast); the server-side hot path never calls ``dequantize_tensor``.

The worker's side is at the end of the module: ``BroadcastDequantizer`` and the quantised client
endpoints, which decode records on a GPU with ``fedavg_quant_decode``, as
``dequantize_tensor`` and ``dequantize_parameter`` do for records that lie there.
"""

from __future__ import annotations

import logging
import math
import os
from collections.abc import Callable, Mapping
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from . import _native
from .fedavg import FedAvgContext, ModelLayout, NaNAggregationError
from .message import is_parameter_message

_log = logging.getLogger(__name__)

HEADER_BYTES = 16  # QSGD records
NNADQ_HEADER_BYTES = 32
DEFAULT_LEVEL = 255  # quantized_endpoint.py:104,110
NNADQ_MAX_LEVELS = 255  # one byte per code


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


@dataclass(frozen=True)
class QuantizedDtype:
    """Input format code of quantised records for the C ABI (``fedavg_dtype``)."""

    name: str
    value_dtype: torch.dtype  # the codec's arithmetic dtype (what dequant returns)
    code: int
    scheme: str = "qsgd"  # "qsgd" | "nnadq"

    def record_bytes(self, numel: int) -> int:
        """Byte size of one record of a numel-element tensor (== fedavg_<scheme>_record_bytes)."""
        return _native.record_bytes(self.code, numel)


QSGD_F32 = QuantizedDtype("qsgd_f32", torch.float32, _native.QSGD_F32)
QSGD_F64 = QuantizedDtype("qsgd_f64", torch.float64, _native.QSGD_F64)
NNADQ_F32 = QuantizedDtype("nnadq_f32", torch.float32, _native.NNADQ_F32, "nnadq")
NNADQ_F64 = QuantizedDtype("nnadq_f64", torch.float64, _native.NNADQ_F64, "nnadq")


def codec_for(dtype: torch.dtype, scheme: str = "qsgd") -> QuantizedDtype:
    if scheme == "nnadq":
        return NNADQ_F64 if dtype == torch.float64 else NNADQ_F32
    return QSGD_F64 if dtype == torch.float64 else QSGD_F32


def sign_offset(numel: int) -> int:
    """Byte offset of the sign bits in a record (== fedavg_qsgd_sign_offset)."""
    return HEADER_BYTES + _align16(numel)


def record_bytes(numel: int) -> int:
    """Byte size of one record (== fedavg_qsgd_record_bytes)."""
    return _native.record_bytes(_native.QSGD_F32, numel)


@dataclass
class QuantizedTensor:
    """One quantised parameter tensor: a record (uint8, 1-D) + its shape and codec."""

    record: torch.Tensor
    shape: tuple[int, ...]
    codec: QuantizedDtype

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        if self.record.dtype != torch.uint8 or self.record.dim() != 1:
            raise ValueError("a quantised record is a 1-D uint8 tensor")
        need = self.codec.record_bytes(self.numel)
        if self.record.numel() != need:
            raise ValueError(f"record holds {self.record.numel()} bytes, the layout needs {need}")

    @property
    def numel(self) -> int:
        n = 1
        for s in self.shape:
            n *= s
        return n

    @property
    def device(self) -> torch.device:
        return self.record.device

    @property
    def dtype(self) -> torch.dtype:
        return self.codec.value_dtype

    def _qsgd(self) -> None:
        if self.codec.scheme != "qsgd":
            raise AttributeError(f"{self.codec.name} records have no QSGD fields")

    def _nnadq(self) -> None:
        if self.codec.scheme != "nnadq":
            raise AttributeError(f"{self.codec.name} records have no NNADQ fields")

    @property
    def norm(self) -> float:
        self._qsgd()
        return float(self.record[0:8].cpu().view(torch.float64)[0])

    @property
    def level(self) -> int:
        self._qsgd()
        return int(self.record[8:12].cpu().view(torch.int32)[0])

    @property
    def slots(self) -> torch.Tensor:
        self._qsgd()
        return self.record[HEADER_BYTES : HEADER_BYTES + self.numel]

    @property
    def sign_bits(self) -> torch.Tensor:
        """One 0/1 (uint8) per element, 1 = non-negative."""
        self._qsgd()
        so = sign_offset(self.numel)
        packed = self.record[so : so + (self.numel + 7) // 8]
        shifts = torch.arange(7, -1, -1, device=packed.device, dtype=torch.uint8)
        return ((packed.unsqueeze(1) >> shifts) & 1).reshape(-1)[: self.numel]

    @property
    def lo(self) -> float:
        self._nnadq()
        return float(self.record[0:8].cpu().view(torch.float64)[0])

    @property
    def step(self) -> float:
        self._nnadq()
        return float(self.record[8:16].cpu().view(torch.float64)[0])

    @property
    def levels(self) -> int:
        self._nnadq()
        return int(self.record[16:20].cpu().view(torch.int32)[0])

    @property
    def codes(self) -> torch.Tensor:
        self._nnadq()
        return self.record[NNADQ_HEADER_BYTES : NNADQ_HEADER_BYTES + self.numel]

    def to(self, device: torch.device | str, non_blocking: bool = False) -> QuantizedTensor:
        return QuantizedTensor(self.record.to(device, non_blocking=non_blocking), self.shape, self.codec)


_BIT_WEIGHTS: dict[torch.device, torch.Tensor] = {}


def _pack_bits(bits: torch.Tensor) -> torch.Tensor:
    """numpy.packbits order: element i -> byte i // 8, bit 7 - i % 8 (zero padded)."""
    n = bits.numel()
    pad = (-n) % 8
    b = bits.to(torch.uint8)
    if pad:
        b = torch.cat([b, torch.zeros(pad, dtype=torch.uint8, device=b.device)])
    w = _BIT_WEIGHTS.get(b.device)
    if w is None:
        w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.int32, device=b.device)
        _BIT_WEIGHTS[b.device] = w
    return (b.view(-1, 8).to(torch.int32) * w).sum(dim=1).to(torch.uint8)


def quantize_tensor(
    tensor: torch.Tensor,
    quantization_level: int = DEFAULT_LEVEL,
    use_l2_norm: bool = False,
    generator: torch.Generator | None = None,
) -> QuantizedTensor:
    """QSGD quantisation of one tensor (on its own device): norm n = max|x| (l2 if asked),
    r = |x| / n * level, slot = floor(r) + Bernoulli(r - floor(r)), sign bit = not (x < 0)."""
    if not 1 <= quantization_level <= 255:
        raise ValueError("quantization_level must be in [1, 255] (one byte per slot)")
    codec = codec_for(tensor.dtype)
    v = tensor.detach().reshape(-1).to(codec.value_dtype)
    n = v.numel()
    dev = v.device
    rec = torch.zeros(record_bytes(n), dtype=torch.uint8, device=dev)
    if n:
        absv = v.abs()
        norm = torch.linalg.vector_norm(v) if use_l2_norm else absv.max()
        r = (absv / norm) * quantization_level
        fl = torch.floor(r)
        u = torch.rand(n, generator=generator, device=dev, dtype=codec.value_dtype)
        slots = fl + (u < (r - fl)).to(fl.dtype)
        slots = torch.where(norm > 0, slots, torch.zeros_like(slots))
        slots = slots.clamp_(0, quantization_level).to(torch.uint8)
        rec[HEADER_BYTES : HEADER_BYTES + n] = slots
        packed = _pack_bits(~(v < 0))
        so = sign_offset(n)
        rec[so : so + packed.numel()] = packed
        rec[0:8] = norm.to(torch.float64).reshape(1).view(torch.uint8)
    rec[8:12] = torch.tensor([quantization_level], dtype=torch.int32).view(torch.uint8).to(dev)
    return QuantizedTensor(rec, tuple(tensor.shape), codec)


def dequantize_tensor(q: QuantizedTensor) -> torch.Tensor:
    """Dense x_hat in the codec's dtype (consumers of dense tensors; the server's FedAvg fold
    dequantises inside its kernel instead): QSGD ((norm * sign) * slot) / level, NNADQ
    code * step + lo. A record on a GPU is decoded there by ``fedavg_quant_decode`` (one launch,
    DESIGN.md §5u), a host record by torch ops on the host: the same bits either way. Non-finite
    values are handed on as they come (the consumer's own check sees them)."""
    if q.record.device.type == "cuda":
        return _decode_plain({"x": q})["x"]
    return _dequantize_host(q)


def _dequantize_host(q: QuantizedTensor) -> torch.Tensor:
    """The decoder as eager torch ops, one rounding per op in the codec's dtype."""
    dt = q.codec.value_dtype
    rec = q.record
    if q.codec.scheme == "nnadq":
        lo = rec[0:8].view(torch.float64).to(dt)
        step = rec[8:16].view(torch.float64).to(dt)
        return (q.codes.to(dt) * step + lo).reshape(q.shape)  # two eager ops: two roundings
    norm = rec[0:8].view(torch.float64).to(dt)
    level = rec[8:12].view(torch.int32).to(dt)
    sign = q.sign_bits.to(dt) * 2 - 1
    x = (norm * sign) * q.slots.to(dt)
    return (x / level).reshape(q.shape)  # tensor / tensor: a true division, never a reciprocal


def stochastic_quantization(
    quantization_level: int = DEFAULT_LEVEL,
    use_l2_norm: bool = False,
    generator: torch.Generator | None = None,
) -> tuple[Callable[[Mapping[str, torch.Tensor]], dict[str, QuantizedTensor]],
           Callable[[Mapping[str, QuantizedTensor]], dict[str, torch.Tensor]]]:
    """The (quant, dequant) pair the reference's endpoints take (quantized_endpoint.py:96-111)."""

    def quant(parameter: Mapping[str, torch.Tensor]) -> dict[str, QuantizedTensor]:
        return {k: quantize_tensor(v, quantization_level, use_l2_norm, generator) for k, v in parameter.items()}

    def dequant(parameter: Mapping[str, QuantizedTensor]) -> dict[str, torch.Tensor]:
        return {k: dequantize_tensor(v) if isinstance(v, QuantizedTensor) else v for k, v in parameter.items()}

    return quant, dequant


def is_quantized(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, QuantizedTensor) for v in parameter.values())


def dequantize_parameter(parameter: Mapping[str, object]) -> dict[str, object]:
    """QuantServerEndpoint.get's dequantisation (quantized_endpoint.py:69-77) for consumers
    that cannot take records (the fused FedAvg path never calls this). Records on a GPU are
    decoded there, one ``fedavg_quant_decode`` launch per codec present; host records by the host
    path; dense values pass through."""
    if any(isinstance(v, QuantizedTensor) and v.record.device.type == "cuda" for v in parameter.values()):
        return _decode_plain(parameter)
    return {k: _dequantize_host(v) if isinstance(v, QuantizedTensor) else v for k, v in parameter.items()}


# -- the record decoder on the device (fedavg_quant_decode) -------------------------

_DecodeItem = tuple[QuantizedTensor, torch.Tensor, torch.Tensor | None]  # record, flat output, flat fp64 output


def _decode_on_device(ctx: FedAvgContext, items: list[_DecodeItem]) -> None:
    """Enqueue the decode of ``(record, flat output, flat fp64 output or None)`` triples that lie on
    the context's device: one launch per codec present (two where only part of a codec's records
    carry an fp64 output)."""
    groups: dict[tuple[int, bool], list[_DecodeItem]] = {}
    for item in items:
        if item[0].numel:
            groups.setdefault((item[0].codec.code, item[2] is not None), []).append(item)
    for (code, wide), group in sorted(groups.items()):
        ctx.quant_decode(code, [_aligned_record(q.record) for q, _, _ in group], [o for _, o, _ in group],
                         [w for _, _, w in group] if wide else None)


def _aligned_record(record: torch.Tensor) -> torch.Tensor:
    """The record as the kernel takes it: contiguous and 16-byte aligned (a copy where it is not)."""
    record = record.contiguous()
    return record if record.data_ptr() % 16 == 0 else record.clone()


_plain_contexts: dict[torch.device, FedAvgContext] = {}


def _decode_plain(parameter: Mapping[str, object]) -> dict[str, object]:
    """``dequantize_parameter`` with the device records decoded by the kernel into fresh tensors.
    The context's flag is not read: what the contract's lines give is handed on, finite or not, as
    the host path hands it on (the kernel writes every element by those lines either way)."""
    out: dict[str, object] = {}
    by_device: dict[torch.device, list[_DecodeItem]] = {}
    for name, v in parameter.items():
        if not isinstance(v, QuantizedTensor):
            out[name] = v
        elif v.record.device.type != "cuda":
            out[name] = _dequantize_host(v)
        else:
            dense = torch.empty(v.shape, dtype=v.codec.value_dtype, device=v.record.device)
            by_device.setdefault(v.record.device, []).append((v, dense.reshape(-1), None))
            out[name] = dense
    for device, items in by_device.items():
        ctx = _plain_contexts.get(device)
        if ctx is None:
            ctx = _plain_contexts[device] = FedAvgContext(ModelLayout.flat(1, "quant"), device)
        _decode_on_device(ctx, items)
    return {name: out[name] for name in parameter}


def record_layout(numels: list[int], codec: QuantizedDtype = QSGD_F32) -> ModelLayout:
    """Byte layout of one client's records in one bucket (every record 16-B aligned)."""
    return ModelLayout(names=tuple(f"r{i}" for i in range(len(numels))),
                       shapes=tuple((codec.record_bytes(n),) for n in numels))


# -- NNADQ (NNADQClientEndpoint / NNADQServerEndpoint, quantized_endpoint.py:114-142) ----------

def nnadq_levels(lo: float, hi: float, weight: float) -> int:
    """Levels of one tensor's code: the step is at most ``weight`` x the tensor's largest
    magnitude, capped at 255 levels (one byte per code); 1 for a constant or non-finite tensor."""
    amax = max(abs(lo), abs(hi))
    if not (amax > 0 and weight > 0):
        return 1
    r = (hi - lo) / (weight * amax)
    if not math.isfinite(r) or r <= 0:
        return 1
    return int(min(NNADQ_MAX_LEVELS, max(1, math.ceil(r))))


def nnadq_quantize_tensor(tensor: torch.Tensor, weight: float = 0.01) -> QuantizedTensor:
    """Deterministic NNADQ quantisation of one tensor (on its own device): lo = min, hi = max,
    L = nnadq_levels(lo, hi, weight), step = (hi - lo) / L, code = clamp(round((x - lo) / step),
    0, L) (round half to even), all in the codec's dtype."""
    codec = codec_for(tensor.dtype, "nnadq")
    dt = codec.value_dtype
    v = tensor.detach().reshape(-1).to(dt)
    n = v.numel()
    dev = v.device
    rec = torch.zeros(codec.record_bytes(n), dtype=torch.uint8, device=dev)
    levels = 1
    if n:
        lo, hi = v.min(), v.max()
        levels = nnadq_levels(float(lo), float(hi), weight)
        step = (hi - lo) / torch.tensor(levels, dtype=dt, device=dev)
        s = float(step)
        if s > 0 and math.isfinite(s):
            codes = torch.clamp(torch.round((v - lo) / step), 0, levels)
            codes = torch.nan_to_num(codes, nan=0.0).to(torch.uint8)
        else:
            codes = torch.zeros(n, dtype=torch.uint8, device=dev)
        rec[NNADQ_HEADER_BYTES : NNADQ_HEADER_BYTES + n] = codes
        rec[0:8] = lo.to(torch.float64).reshape(1).view(torch.uint8)
        rec[8:16] = step.to(torch.float64).reshape(1).view(torch.uint8)
    rec[16:20] = torch.tensor([levels], dtype=torch.int32).view(torch.uint8).to(dev)
    return QuantizedTensor(rec, tuple(tensor.shape), codec)


class NeuralNetworkAdaptiveDeterministicQuant:
    """The client-side NNADQ quantiser (``NNADQ(weight)[0]``): every tensor of a parameter dict
    to an NNADQ record."""

    def __init__(self, weight: float) -> None:
        self.weight = float(weight)

    def __call__(self, parameter: Mapping[str, torch.Tensor]) -> dict[str, QuantizedTensor]:
        return {k: nnadq_quantize_tensor(v, self.weight) for k, v in parameter.items()}

    @staticmethod
    def check_compression_ratio(quantized_data: object, prefix: str = "") -> float:
        """Bytes of the records over the bytes of the dense tensors they replace (the endpoint's
        ``_after_quant`` log, quantized_endpoint.py:121-124,139-142); returned, not asserted."""
        parameter = getattr(quantized_data, "parameter", quantized_data)
        packed = dense = 0
        for v in parameter.values():
            if isinstance(v, QuantizedTensor):
                packed += v.record.numel()
                dense += v.numel * torch.empty((), dtype=v.codec.value_dtype).element_size()
        ratio = packed / dense if dense else 1.0
        _log.debug("%s compression ratio %.4f", prefix, ratio)
        return ratio


class NeuralNetworkAdaptiveDeterministicDequant:
    """The server-side NNADQ dequantiser (``NNADQServerEndpoint(weight=None)``'s dequant,
    quantized_endpoint.py:130-133): needs nothing but the records. The fused FedAvg path never
    calls it; dense consumers do."""

    def __call__(self, parameter: Mapping[str, object]) -> dict[str, object]:
        return dequantize_parameter(parameter)


def NNADQ(weight: float) -> tuple[NeuralNetworkAdaptiveDeterministicQuant, NeuralNetworkAdaptiveDeterministicDequant]:  # noqa: N802
    """The (quant, dequant) pair the NNADQ endpoints take (quantized_endpoint.py:117,135)."""
    return NeuralNetworkAdaptiveDeterministicQuant(weight), NeuralNetworkAdaptiveDeterministicDequant()


# -- the broadcast encoder (QuantServerEndpoint.send, quantized_endpoint.py:79-96) ----------------
#
# The server quantises the aggregated model before it goes out to every worker. On a GPU the
# records are written by fedavg_quant_encode (csrc/quant_kernels.hip) where the
# result lies; on the CPU the functions below produce the same bytes. QSGD's uniforms are a
# defined stream, not torch.rand, so both paths and a test restatement agree bit for bit.

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32(counter: np.ndarray, key: tuple[int, int]) -> np.ndarray:
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) of ``counter`` (uint32 [..., 4]) under
    ``key`` (two uint32 words): uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & _U32, int(key[1]) & _U32
    m0, m1 = np.uint64(_PHILOX_M0), np.uint64(_PHILOX_M1)
    mask, s32 = np.uint64(_U32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return np.stack(c, axis=-1).astype(np.uint32)


def _philox_uniforms_np(seed: int, draw: int, t: int, n: int, f64: bool) -> np.ndarray:
    seed, draw, t = int(seed), int(draw), int(t)
    if not 0 <= seed < 1 << 64 or not 0 <= draw < 1 << 32 or not 0 <= t < 1 << 32:
        raise ValueError("the seed is a uint64, the draw and the tensor index are uint32")
    per = 2 if f64 else 4
    blocks = np.arange((n + per - 1) // per, dtype=np.uint64)
    ctr = np.empty((blocks.size, 4), dtype=np.uint32)
    ctr[:, 0] = (blocks & np.uint64(_U32)).astype(np.uint32)
    ctr[:, 1] = (blocks >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = t
    ctr[:, 3] = draw
    out = philox4x32(ctr, (seed & _U32, seed >> 32))
    if not f64:
        return ((out >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24)).reshape(-1)[:n]
    lo, hi = out[:, 0::2].astype(np.uint64), out[:, 1::2].astype(np.uint64)
    m = ((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))  # 53 bits: exact in fp64
    return (m.astype(np.float64) * 2.0**-53).reshape(-1)[:n]


def philox_uniforms(seed: int, draw: int, t: int, n: int, dtype: torch.dtype) -> torch.Tensor:
    """The ``n`` uniforms in [0, 1) that the broadcast encoder's QSGD draws for tensor ``t``:
    Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)`` and counter ``(block & 0xffffffff,
    block >> 32, t, draw)``. fp32: ``block = i // 4``, ``u = (out[i % 4] >> 8) * 2**-24``; fp64:
    ``block = i // 2``, ``u = ((out[2 (i % 2) + 1] >> 5) * 2**26 + (out[2 (i % 2)] >> 6)) * 2**-53``.
    A CPU tensor of ``dtype`` (fp32 or fp64)."""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"the uniform stream is defined for fp32 and fp64, not {dtype}")
    return torch.from_numpy(_philox_uniforms_np(seed, draw, t, int(n), dtype == torch.float64).copy())


def _total_order_extrema(v: np.ndarray) -> tuple[np.floating, np.floating]:
    """(min, max) of a non-empty finite numpy vector with -0.0 < +0.0 (numpy's own min / max leave
    the sign of a zero extremum to the order of the elements)."""
    lo, hi = v.min(), v.max()
    if lo == 0:
        lo = v.dtype.type(-0.0 if np.any(np.signbit(v) & (v == 0)) else 0.0)
    if hi == 0:
        hi = v.dtype.type(0.0 if np.any(~np.signbit(v) & (v == 0)) else -0.0)
    return lo, hi


def _encode_host(v: np.ndarray, scheme: str, level: int, weight: float, seed: int, draw: int, t: int) -> np.ndarray:
    """One record (numpy uint8) of the flat fp32 / fp64 numpy vector ``v``: the same operations,
    each rounded in ``v``'s dtype, as quant_kernels.hip."""
    dt = v.dtype.type
    n = v.size
    if not np.isfinite(v).all():
        raise NaNAggregationError("input", f"tensor {t} of the model to broadcast holds a non-finite element")
    if scheme == "nnadq":
        rec = np.zeros(NNADQ_HEADER_BYTES + _align16(n), dtype=np.uint8)
        lo, step, levels = dt(0), dt(0), 1
        if n:
            lo, hi = _total_order_extrema(v)
            with np.errstate(all="ignore"):
                dlo, dhi = np.float64(lo), np.float64(hi)
                amax = max(abs(dlo), abs(dhi))
                r = (dhi - dlo) / (np.float64(weight) * amax) if amax > 0 and weight > 0 else np.float64("nan")
                if np.isfinite(r) and r > 0:
                    levels = int(min(NNADQ_MAX_LEVELS, max(1, math.ceil(r))))
                step = dt(hi - lo) / dt(levels)
                if step > 0 and np.isfinite(step):
                    codes = np.clip(np.rint((v - lo) / step), 0, levels).astype(np.uint8)
                    rec[NNADQ_HEADER_BYTES : NNADQ_HEADER_BYTES + n] = codes
        rec[0:8] = np.frombuffer(np.float64(lo).tobytes(), dtype=np.uint8)
        rec[8:16] = np.frombuffer(np.float64(step).tobytes(), dtype=np.uint8)
        rec[16:20] = np.frombuffer(np.int32(levels).tobytes(), dtype=np.uint8)
        return rec
    rec = np.zeros(record_bytes(n), dtype=np.uint8)
    norm = dt(0)
    if n:
        lo, hi = _total_order_extrema(v)
        norm = max(-lo, hi)
        if norm > 0:
            with np.errstate(all="ignore"):
                r = (np.abs(v) / norm) * dt(level)
                fl = np.floor(r)
                u = _philox_uniforms_np(seed, draw, t, n, v.dtype == np.float64)
                slots = fl + (u < (r - fl))
            rec[HEADER_BYTES : HEADER_BYTES + n] = np.clip(slots, 0, level).astype(np.uint8)
        else:
            norm = dt(0)
        packed = np.packbits(~(v < 0))
        so = sign_offset(n)
        rec[so : so + packed.size] = packed
    rec[0:8] = np.frombuffer(np.float64(norm).tobytes(), dtype=np.uint8)
    rec[8:12] = np.frombuffer(np.int32(level).tobytes(), dtype=np.uint8)
    return rec


class BroadcastQuantizer:
    """The server's broadcast encoder: ``quantizer(parameter, draw)`` turns a model into QSGD or
    NNADQ records (``scheme``), what the reference's quantised server endpoints do in ``send`` once
    ``use_quant()`` was called (quantized_endpoint.py:79-96).

    Tensors on a GPU are encoded there by ``fedavg_quant_encode`` (three launches per dtype group
    whatever the number of tensors) into one device blob that the quantizer keeps and reuses: the
    records returned are views of it and stay valid until the next call on that device.
    ``encode_to_host`` moves the blob to the host in one copy and returns records that own their
    memory. Tensors on the CPU are encoded by a numpy path that gives the same bytes. The dict may
    mix fp32 and fp64 tensors (encoded per dtype group); any other dtype is a ``TypeError``.

    QSGD's uniforms are the stream of ``philox_uniforms(seed, draw, t, ...)`` with ``t`` the
    tensor's position in the dict; ``draw`` is the caller's (the server passes its broadcast count,
    so rounds do not repeat a stream). NNADQ is deterministic: ``seed`` and ``draw`` play no part. A
    non-finite element is refused with ``NaNAggregationError`` (an ``AssertionError``), and no
    record is handed out. ``use_l2_norm`` is not offered: its summation order is unpinned."""

    def __init__(self, scheme: str = "qsgd", quantization_level: int = DEFAULT_LEVEL, weight: float = 0.01,
                 seed: int = 0, use_l2_norm: bool = False) -> None:
        if scheme not in ("qsgd", "nnadq"):
            raise ValueError(f"unknown scheme {scheme!r}: 'qsgd' or 'nnadq'")
        if use_l2_norm:
            raise NotImplementedError("the broadcast encoder offers the max norm only: the l2 norm's "
                                      "summation order is unpinned")
        if not isinstance(quantization_level, int) or not 1 <= quantization_level <= 255:
            raise ValueError("quantization_level must be an integer in [1, 255] (one byte per slot)")
        weight = float(weight)
        if not (weight > 0 and math.isfinite(weight)):
            raise ValueError("weight must be a finite number > 0")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed must be a uint64")
        self.scheme = scheme
        self.quantization_level = quantization_level
        self.weight = weight
        self.seed = int(seed)
        self._contexts: dict[torch.device, FedAvgContext] = {}
        self._blobs: dict[torch.device, torch.Tensor] = {}

    def _context(self, device: torch.device) -> FedAvgContext:
        ctx = self._contexts.get(device)
        if ctx is None:
            # the encoder does not depend on a context's layout: a one-element layout carries the
            # device, the stream order, the flag words and the call's workspace
            ctx = self._contexts[device] = FedAvgContext(ModelLayout.flat(1, "quant"), device)
        return ctx

    def device_blob(self, device: torch.device | str) -> torch.Tensor | None:
        """The uint8 blob that holds the records of the last call on ``device`` (None before the
        first): every record of a call is written whole, so its content between calls is free."""
        return self._blobs.get(torch.device(device))

    def _blob(self, device: torch.device, nbytes: int) -> torch.Tensor:
        blob = self._blobs.get(device)
        if blob is None or blob.numel() < nbytes:
            blob = self._blobs[device] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        return blob

    def detach_blobs(self) -> None:
        """Forget the device blobs: the records of the calls so far keep theirs alive and stay
        valid, and the next call on a device starts a new blob."""
        self._blobs.clear()

    def _plan(self, parameter: Mapping[str, torch.Tensor]) -> list[tuple[str, torch.Tensor, QuantizedDtype, int]]:
        plan = []
        for t, (name, value) in enumerate(parameter.items()):
            if not isinstance(value, torch.Tensor) or value.dtype not in (torch.float32, torch.float64):
                kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
                raise TypeError(f"{name}: the broadcast encoder takes fp32 and fp64 tensors, not {kind}")
            plan.append((name, value.detach(), codec_for(value.dtype, self.scheme), t))
        return plan

    def __call__(self, parameter: Mapping[str, torch.Tensor], draw: int = 0) -> dict[str, QuantizedTensor]:
        draw = int(draw)
        if not 0 <= draw < 1 << 32:
            raise ValueError("draw must be a uint32")
        plan = self._plan(parameter)
        out: dict[str, QuantizedTensor] = {}
        by_device: dict[torch.device, list[tuple[str, torch.Tensor, QuantizedDtype, int]]] = {}
        for item in plan:
            by_device.setdefault(item[1].device, []).append(item)
        for device, items in by_device.items():
            if device.type == "cpu":
                for name, value, codec, t in items:
                    v = value.contiguous().reshape(-1).numpy()
                    rec = _encode_host(v, self.scheme, self.quantization_level, self.weight, self.seed, draw, t)
                    out[name] = QuantizedTensor(torch.from_numpy(rec), tuple(value.shape), codec)
            else:
                out.update(self._encode_device(device, items, draw))
        return {name: out[name] for name in parameter}  # the model's own key order

    def _encode_device(self, device: torch.device, items: list[tuple[str, torch.Tensor, QuantizedDtype, int]],
                       draw: int) -> dict[str, QuantizedTensor]:
        ctx = self._context(device)
        sizes = [codec.record_bytes(value.numel()) for _, value, codec, _ in items]  # multiples of 16
        blob = self._blob(device, sum(sizes))
        views, off = [], 0
        for size in sizes:
            views.append(blob[off : off + size])
            off += size
        flat = [value.contiguous().reshape(-1) for _, value, _, _ in items]
        for code in sorted({codec.code for _, _, codec, _ in items}):
            group = [i for i, item in enumerate(items) if item[2].code == code]
            ctx.quant_encode(code, [flat[i] for i in group], [views[i] for i in group], self.quantization_level,
                             self.weight, self.seed, draw, [items[i][3] for i in group])
        ctx.raise_on_nan()  # waits for the stream; a non-finite element is an AssertionError
        return {name: QuantizedTensor(views[i], tuple(value.shape), codec)
                for i, (name, value, codec, _) in enumerate(items)}

    def encode_to_host(self, parameter: Mapping[str, torch.Tensor], draw: int = 0) -> dict[str, QuantizedTensor]:
        """``self(parameter, draw)`` with every record on the host: a device's records cross in one
        copy of its blob, and the host records do not alias the quantizer's reused device blob."""
        records = self(parameter, draw)
        out: dict[str, QuantizedTensor] = {}
        host_blobs: dict[torch.device, torch.Tensor] = {}
        for name, q in records.items():
            if q.record.device.type == "cpu":
                out[name] = q
                continue
            blob = self._blobs[q.record.device]
            host = host_blobs.get(q.record.device)
            if host is None:
                used = max(r.record.storage_offset() + r.record.numel() for r in records.values()
                           if r.record.device == q.record.device)
                host = host_blobs[q.record.device] = blob[:used].to("cpu")
            off = q.record.storage_offset()
            # a record of its own storage: a transport that pickles tensors sends a view's whole storage
            out[name] = QuantizedTensor(host[off : off + q.record.numel()].clone(), q.shape, q.codec)
        return out


# -- the worker's side (QuantClientEndpoint, quantized_endpoint.py:17-51, :102-105, :114-124) -------
#
# A worker behind a quantised endpoint receives the server's broadcast as records and sends its own
# update as records. On a GPU the records are decoded by fedavg_quant_decode (csrc/quant_kernels.hip,
# DESIGN.md §5u) where they lie, or after one upload of about 1.1 bytes per element, straight into
# the model's own parameters if the worker says so; host records are decoded on the host.

_FLAGGED = "a record's level lies outside [1, 255] or an element decodes to a non-finite value"


class BroadcastDequantizer:
    """The counterpart of ``BroadcastQuantizer``: ``dequantizer(records, device=None, out=None,
    f64_out=None)`` turns a dict of records into a dict of dense tensors in the codecs' dtypes,
    what the reference's quantised client endpoints do in ``get`` once ``dequant_server_data()`` was
    called (quantized_endpoint.py:32-39). Dense values in the dict pass through unchanged.

    Records on a GPU are decoded there by ``fedavg_quant_decode``, one launch per codec present.
    Host records with ``device=`` a GPU are packed into one pinned blob, cross in one copy (about
    1.1 bytes per element instead of the 4 or 8 of a dense tensor) and are decoded on that device.
    Host records without a ``device`` are decoded on the host. The bits are the same in every case.

    ``out`` maps names to existing tensors that are written in place and returned, e.g. the model's
    own parameters: the codec's dtype, the record's shape, on the device where the record is
    decoded, contiguous but aligned to the element only; anything else is a ``ValueError``. Names
    it does not hold get new tensors. ``f64_out`` likewise maps names of fp32 records to fp64
    tensors that receive the exact widening of the same values in the same pass (what a worker's
    model cache keeps); naming an fp64 record there is a ``ValueError``.

    A header whose level lies outside [1, 255], or an element that decodes to a non-finite value, is
    refused with ``NaNAggregationError`` (an ``AssertionError``, ``stage="input"``) and no tensor is
    handed out; what ``out`` holds then is unspecified. The dequantizer keeps one context and one
    reusable blob per device."""

    def __init__(self) -> None:
        self._contexts: dict[torch.device, FedAvgContext] = {}
        self._blobs: dict[torch.device, torch.Tensor] = {}
        self._pinned: dict[torch.device, torch.Tensor] = {}

    def _context(self, device: torch.device) -> FedAvgContext:
        ctx = self._contexts.get(device)
        if ctx is None:
            # the decoder does not depend on a context's layout: a one-element layout carries the
            # device, the stream order, the flag words and the call's workspace
            ctx = self._contexts[device] = FedAvgContext(ModelLayout.flat(1, "quant"), device)
        return ctx

    @staticmethod
    def _given(table: Mapping[str, torch.Tensor] | None, name: str, q: QuantizedTensor, dtype: torch.dtype,
               device: torch.device, what: str) -> torch.Tensor | None:
        t = None if table is None else table.get(name)
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            kind = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}[{name!r}]: a {dtype} tensor is required, not {kind}")
        if tuple(t.shape) != q.shape or t.device != device:
            raise ValueError(f"{what}[{name!r}]: shape {q.shape} on {device} is required, not {tuple(t.shape)} on "
                             f"{t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}[{name!r}]: the decoder writes contiguous tensors (any element alignment)")
        return t

    def _upload(self, device: torch.device,
                items: list[tuple[str, QuantizedTensor]]) -> list[tuple[str, QuantizedTensor]]:
        """The host records of ``items`` on ``device``: packed into the pinned blob, one copy."""
        total = sum(q.record.numel() for _, q in items)  # every record is a multiple of 16 bytes
        pinned = self._pinned.get(device)
        if pinned is None or pinned.numel() < total:
            pinned = self._pinned[device] = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
        blob = self._blobs.get(device)
        if blob is None or blob.numel() < total:
            blob = self._blobs[device] = torch.empty(max(total, 16), dtype=torch.uint8, device=device)
        off = 0
        moved = []
        for name, q in items:
            n = q.record.numel()
            pinned[off : off + n].copy_(q.record)
            moved.append((name, QuantizedTensor(blob[off : off + n], q.shape, q.codec)))
            off += n
        # the pinned blob is free again when this call returns: the flag check waits for the stream
        blob[:total].copy_(pinned[:total], non_blocking=True)
        return moved

    def __call__(self, records: Mapping[str, object], device: torch.device | str | None = None,
                 out: Mapping[str, torch.Tensor] | None = None,
                 f64_out: Mapping[str, torch.Tensor] | None = None) -> dict[str, object]:
        target = None if device is None else torch.device(device)
        if target is not None and target.type == "cuda" and target.index is None:
            target = torch.device("cuda", torch.cuda.current_device())
        result: dict[str, object] = {}
        on_host: list[tuple[str, QuantizedTensor]] = []
        to_upload: list[tuple[str, QuantizedTensor]] = []
        on_device: dict[torch.device, list[tuple[str, QuantizedTensor]]] = {}
        for name, v in records.items():
            if not isinstance(v, QuantizedTensor):
                result[name] = v
            elif v.record.device.type == "cuda":
                on_device.setdefault(v.record.device, []).append((name, v))
            elif target is not None and target.type == "cuda":
                to_upload.append((name, v))
            else:
                on_host.append((name, v))
        # every output is checked before anything is written
        plan: dict[str, tuple[torch.Tensor | None, torch.Tensor | None]] = {}
        for where, items in [(torch.device("cpu"), on_host), (target, to_upload), *on_device.items()]:
            for name, q in items:
                wide = self._given(f64_out, name, q, torch.float64, where, "f64_out")
                if wide is not None and q.codec.value_dtype == torch.float64:
                    raise ValueError(f"f64_out[{name!r}]: the fp64 copy is offered for fp32 records; this one "
                                     "decodes to fp64")
                plan[name] = (self._given(out, name, q, q.codec.value_dtype, where, "out"), wide)

        decoded = {name: self._decode_host(name, q) for name, q in on_host}
        if to_upload:
            on_device.setdefault(target, []).extend(self._upload(target, to_upload))
        for where, items in on_device.items():
            triples = []
            for name, q in items:
                dense, wide = plan[name]
                if dense is None:
                    dense = torch.empty(q.shape, dtype=q.codec.value_dtype, device=where)
                result[name] = dense
                triples.append((q, dense.reshape(-1), None if wide is None else wide.reshape(-1)))
            ctx = self._context(where)
            _decode_on_device(ctx, triples)
            if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
                ctx.reset()  # the flag is sticky until reset: the context stays usable
                raise NaNAggregationError("input", f"the records on {where}: {_FLAGGED}")
        for name, dense in decoded.items():
            given, wide = plan[name]
            if wide is not None:
                wide.copy_(dense)  # fp32 -> fp64: exact
            result[name] = dense if given is None else given.copy_(dense)
        return {name: result[name] for name in records}

    @staticmethod
    def _decode_host(name: str, q: QuantizedTensor) -> torch.Tensor:
        level = q.levels if q.codec.scheme == "nnadq" else q.level
        dense = _dequantize_host(q)
        if not 1 <= level <= 255 or not bool(torch.isfinite(dense).all()):
            raise NaNAggregationError("input", f"{name}: {_FLAGGED}")
        return dense


class QuantClientEndpoint:
    """Wraps a client endpoint (any object with ``get()`` and ``send(data)``) as the reference's
    ``QuantClientEndpoint`` does its base class (quantized_endpoint.py:17-51): ``send`` quantises a
    ``ParameterMessage``'s ``parameter`` with ``quant``, calls ``_after_quant`` and hands it on;
    ``get`` dequantises a ``ParameterMessage``'s ``parameter`` with ``dequant`` once
    ``dequant_server_data()`` was called. Every other message passes unchanged in both directions
    (the reference does not quantise a delta on the client), ``None`` included, and every other
    attribute is the wrapped endpoint's. Keyword arguments ``device`` and ``out`` (both optional)
    are passed to ``dequant`` where given: where to decode host records, and the tensors to decode
    into, e.g. the model's own parameters. Without an ``endpoint`` the remaining keyword arguments
    build the simulator's ``ClientEndpoint`` (the reference's base class), which is how
    ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, quant: Callable[..., dict[str, Any]], dequant: Callable[..., dict[str, Any]],
                 endpoint: Any = None, **kwargs: Any) -> None:
        self.device: torch.device | str | None = kwargs.pop("device", None)
        self.out: Mapping[str, torch.Tensor] | None = kwargs.pop("out", None)
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)) or not callable(getattr(endpoint, "get", None)):
            raise TypeError("the wrapped endpoint needs a get() and a send(data) method")
        self._endpoint = endpoint
        self._quant = quant
        self._dequant = dequant
        self._dequant_server_data = False

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def dequant_server_data(self) -> None:
        self._dequant_server_data = True

    def _quantize(self, parameter: Mapping[str, torch.Tensor]) -> dict[str, Any]:
        return self._quant(parameter)

    def _dequantize(self, parameter: Mapping[str, Any]) -> dict[str, Any]:
        options = {k: v for k, v in (("device", self.device), ("out", self.out)) if v is not None}
        return self._dequant(parameter, **options)

    def get(self, *args: Any, **kwargs: Any) -> Any:
        data = self._endpoint.get(*args, **kwargs)
        if not self._dequant_server_data or data is None:
            return data
        if not is_parameter_message(data):  # the reference's assert isinstance(data, ParameterMessage)
            raise AssertionError(f"a quantised broadcast is a ParameterMessage, not {type(data).__name__}")
        data.parameter = self._dequantize(data.parameter)
        return data

    def send(self, data: Any) -> None:
        if is_parameter_message(data):
            data.parameter = self._quantize(data.parameter)
            self._after_quant(data=data)
            _log.debug("after client quantization")
        self._endpoint.send(data)

    def _after_quant(self, data: Any) -> None:
        pass


class _BroadcastCodecEndpoint(QuantClientEndpoint):
    """A ``QuantClientEndpoint`` whose pair is a ``BroadcastQuantizer`` and a ``BroadcastDequantizer``:
    an update on a GPU is encoded there by ``fedavg_quant_encode``, a host update by the numpy path
    that gives the same bytes, and the records own their memory (the quantizer starts a new blob per
    send). ``draw`` starts at 0 and advances by one per ``send``, so no two sends of an endpoint
    share a stream of uniforms."""

    def __init__(self, quantizer: BroadcastQuantizer, **kwargs: Any) -> None:
        super().__init__(quant=quantizer, dequant=BroadcastDequantizer(), **kwargs)
        self.draw = 0

    def _next_draw(self) -> int:
        draw = self.draw
        self.draw = (draw + 1) & _U32
        return draw

    def _quantize(self, parameter: Mapping[str, torch.Tensor]) -> dict[str, Any]:
        records = self._quant(parameter, self._next_draw())
        self._quant.detach_blobs()  # the server may hold these records while the next update is encoded
        return records


class StochasticQuantClientEndpoint(_BroadcastCodecEndpoint):
    """The reference's ``StochasticQuantClientEndpoint`` (quantized_endpoint.py:102-105): QSGD at
    level 255 in both directions. Keyword argument ``seed`` (None: 64 bits of ``os.urandom`` per
    endpoint; a fixed seed is for tests and reproducible experiments), then those of
    ``QuantClientEndpoint``."""

    def __init__(self, **kwargs: Any) -> None:
        seed: int | None = kwargs.pop("seed", None)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        super().__init__(BroadcastQuantizer("qsgd", quantization_level=DEFAULT_LEVEL, seed=seed), **kwargs)

    @property
    def seed(self) -> int:
        return self._quant.seed


class NNADQClientEndpoint(_BroadcastCodecEndpoint):
    """The reference's ``NNADQClientEndpoint`` (quantized_endpoint.py:114-124): NNADQ records with the
    worker's ``weight`` going out, whatever NNADQ records the server sends coming in, and the
    compression ratio logged after every quantisation. ``weight`` has no default."""

    def __init__(self, weight: float, **kwargs: Any) -> None:
        _log.debug("use weight %s", weight)
        super().__init__(BroadcastQuantizer("nnadq", weight=weight), **kwargs)

    def _after_quant(self, data: Any) -> None:
        NeuralNetworkAdaptiveDeterministicQuant.check_compression_ratio(quantized_data=data, prefix="worker")
