"""The differential-privacy layer of a worker: clip an update's L2 norm to ``C`` and add Gaussian
noise ``N(0, (sigma * C)**2)`` before it leaves.

The reference's ``simulation_lib/dp.py`` (``compute_dp_sigma`` :7-10, ``add_dp_noise`` :13-26,
``add_dp_noise_to_parameter`` :29-47) and ``simulation_lib/topology/dp_endpoint.py`` (the two
endpoints), with the hot path — the norm, the clip, the noise and the cast, one streaming pass
family over tensors that already lie in HBM — in ``fedavg_dp_noise`` (csrc/dp_kernels.hip, DESIGN.md
§5r). Tensors on a GPU go through that kernel; host tensors, and dicts that mix dtypes or devices, go
through a numpy path that follows the same contract and gives the same bytes.

What differs from the reference:

* The noise is a defined stream, not ``torch.randn_like``: ``normal_stream(seed, draw, tensor_id,
  n)`` (Philox4x32-10, Box-Muller, a logarithm and a sine / cosine written as fixed sequences of
  separately rounded fp64 operations), so the GPU path, the CPU path and a numpy restatement give
  the same bits.
* The reference computes ``add_dp_noise`` in the feature's own dtype. Here the arithmetic is fp64
  (the element widened exactly, one rounded operation per line, the sum of squares in a pinned
  order) with one final rounding to nearest even into the tensor's dtype.
* A non-finite input raises ``ValueError`` on both paths; the reference would send NaNs that its
  server rejects (fed_avg_algorithm.py:35).
* Tensors that are not floating point (fp32, fp16, bf16, fp64) are a ``TypeError``.

``seed=None`` draws 64 bits from ``os.urandom``; a fixed seed is for tests and reproducible
experiments. The stream is a counter-based statistical generator, NOT a cryptographic one: whoever
knows the seed knows the noise. A floating-point Gaussian mechanism also has known weaknesses
against a determined adversary (Mironov, "On Significance of the Least Significant Bits for
Differential Privacy", CCS 2012): the set of reachable outputs depends on the input. That is as true
of the reference.
"""

from __future__ import annotations

import logging
import math
import os
from collections.abc import Mapping
from typing import Any

import numpy as np
import torch

from . import _native
from .fedavg import FedAvgContext, ModelLayout
from .message import is_delta_message, is_feature_message, is_parameter_message
from .quantized import philox4x32

_log = logging.getLogger(__name__)

_FLOAT_DTYPES = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.float64: "f64"}
_U32 = 0xFFFFFFFF

# 1/3 .. 1/21; -1/3! .. 1/17!; -1/2! .. 1/16! (include/fedavg_hip.h, fedavg_dp_noise)
_LN = [float.fromhex(h) for h in (
    "0x1.5555555555555p-2", "0x1.999999999999ap-3", "0x1.2492492492492p-3", "0x1.c71c71c71c71cp-4",
    "0x1.745d1745d1746p-4", "0x1.3b13b13b13b14p-4", "0x1.1111111111111p-4", "0x1.e1e1e1e1e1e1ep-5",
    "0x1.af286bca1af28p-5", "0x1.8618618618618p-5")]
_SIN = [float.fromhex(h) for h in (
    "-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19",
    "-0x1.ae64567f544e4p-26", "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41", "0x1.952c77030ad4ap-49")]
_COS = [float.fromhex(h) for h in (
    "-0x1p-1", "0x1.5555555555555p-5", "-0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-16",
    "-0x1.27e4fb7789f5cp-22", "0x1.1eed8eff8d898p-29", "-0x1.93974a8c07c9dp-37", "0x1.ae7f3e733b81fp-45")]
_LN2 = float.fromhex("0x1.62e42fefa39efp-1")
_PIO4 = float.fromhex("0x1.921fb54442d18p-1")
_SQRT2_FRAC = 0x6A09E667F3BCD


def compute_dp_sigma(epsilon: float = 4.0, delta: float = 1e-5) -> float:
    """Gaussian mechanism noise multiplier: sqrt(2 * ln(1.25 / delta)) / epsilon (dp.py:7-10)."""
    assert epsilon > 0 and 0 < delta < 1
    return math.sqrt(2 * math.log(1.25 / delta)) / epsilon


# -- the normal stream ------------------------------------------------------------------------
def box_muller(a: np.ndarray, b: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The Box-Muller pair of the 53-bit integers ``a``, ``b`` (uint64 arrays): ``u1 = (a + 1) *
    2**-53``, ``u2 = b * 2**-53``, ``r = sqrt(-2 ln u1)``, ``(r cos 2 pi u2, r sin 2 pi u2)`` with the
    logarithm, the sine and the cosine of the contract: every line one rounded fp64 operation."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    d = (a + np.uint64(1)).astype(np.float64)  # <= 2**53: exact
    bits = d.view(np.uint64)
    frac = bits & np.uint64((1 << 52) - 1)
    up = (frac >= np.uint64(_SQRT2_FRAC)).astype(np.int64)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1023 - 53 + up
    m = (frac | ((1023 - up).astype(np.uint64) << np.uint64(52))).view(np.float64)
    f = m - 1.0
    g = 2.0 + f
    s = f / g
    w = s * s
    p = np.full_like(w, _LN[9])
    for k in range(8, -1, -1):
        p = p * w
        p = p + _LN[k]
    p = p * w
    p = p * s
    q = s + p
    lm = q + q
    el = e.astype(np.float64) * _LN2
    t = (el + lm) * -2.0
    r = np.sqrt(t)

    k = (b >> np.uint64(50)).astype(np.int64)
    fi = b & np.uint64((1 << 50) - 1)
    gi = np.where(k & 1, np.uint64(1 << 50) - fi, fi)
    x = (gi.astype(np.float64) * 2.0**-50) * _PIO4
    w = x * x
    p = np.full_like(w, _SIN[7])
    for j in range(6, -1, -1):
        p = p * w
        p = p + _SIN[j]
    p = p * w
    p = p * x
    sn = x + p
    c = np.full_like(w, _COS[7])
    for j in range(6, -1, -1):
        c = c * w
        c = c + _COS[j]
    c = c * w
    cs = 1.0 + c
    swap = (((k + 1) >> 1) & 1).astype(bool)
    co, si = np.where(swap, sn, cs), np.where(swap, cs, sn)
    co = np.where(((k + 2) >> 2) & 1, -co, co)
    si = np.where(k >> 2, -si, si)
    return r * co, r * si


def _normal_blocks(seed: int, draw: int, tensor_id: int, first_block: int, num_blocks: int) -> np.ndarray:
    blocks = np.arange(first_block, first_block + num_blocks, dtype=np.uint64)
    ctr = np.empty((blocks.size, 4), dtype=np.uint32)
    ctr[:, 0] = (blocks & np.uint64(_U32)).astype(np.uint32)
    ctr[:, 1] = (blocks >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = tensor_id
    ctr[:, 3] = draw
    w = philox4x32(ctr, (seed & _U32, seed >> 32)).astype(np.uint64)
    a = ((w[:, 1] >> np.uint64(5)) << np.uint64(26)) | (w[:, 0] >> np.uint64(6))
    b = ((w[:, 3] >> np.uint64(5)) << np.uint64(26)) | (w[:, 2] >> np.uint64(6))
    z0, z1 = box_muller(a, b)
    return np.stack([z0, z1], axis=1).reshape(-1)


def normal_stream(seed: int, draw: int, tensor_id: int, n: int) -> np.ndarray:
    """The ``n`` standard normal deviates of tensor ``tensor_id`` (float64): element ``i`` comes from
    the Philox4x32-10 block ``i // 2`` with key ``(seed & 0xffffffff, seed >> 32)`` and counter
    ``(block & 0xffffffff, block >> 32, tensor_id, draw)``; its words give ``a = (w1 >> 5) * 2**26 +
    (w0 >> 6)`` and ``b = (w3 >> 5) * 2**26 + (w2 >> 6)``, and ``box_muller(a, b)`` gives elements
    ``2 * block`` and ``2 * block + 1`` (include/fedavg_hip.h, ``fedavg_dp_noise``). Not a
    cryptographic generator."""
    seed, draw, tensor_id, n = int(seed), int(draw), int(tensor_id), int(n)
    if not 0 <= seed < 1 << 64 or not 0 <= draw < 1 << 32 or not 0 <= tensor_id < 1 << 32:
        raise ValueError("the seed is a uint64, the draw and the tensor id are uint32")
    if n < 0:
        raise ValueError("a negative count")
    out = np.empty(n, dtype=np.float64)
    step = 1 << 20  # blocks per chunk: bounds the temporaries
    for first in range(0, (n + 1) // 2, step):
        z = _normal_blocks(seed, draw, tensor_id, first, min(step, (n + 1) // 2 - first))
        out[2 * first : 2 * first + z.size] = z[: n - 2 * first]
    return out


# -- the host path ----------------------------------------------------------------------------
def _tree(v: np.ndarray) -> np.ndarray:
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _lanes_then_tree(v: np.ndarray, lanes: int) -> np.ndarray:
    """[R, K] -> [R]: lane j adds entries j, j + lanes, ... in increasing index from +0.0, then the
    adjacent-pair tree over the lanes."""
    rows, k = v.shape
    steps = -(-k // lanes) if k else 0
    padded = np.zeros((rows, max(steps, 1) * lanes), dtype=np.float64)
    padded[:, :k] = v
    padded = padded.reshape(rows, -1, lanes)
    acc = np.zeros((rows, lanes), dtype=np.float64)
    for m in range(padded.shape[1]):
        acc = acc + padded[:, m, :]
    return _tree(acc)


def _piece_partials(q: np.ndarray, group: int) -> np.ndarray:
    """[R, L] squares -> [R, pieces] partials in the order of ``fedavg_dp_noise``."""
    tile, lanes = _native.kernel_constant("dp_tile"), _native.kernel_constant("dp_threads")
    rows, length = q.shape
    pieces = -(-length // tile)
    padded = np.zeros((rows, pieces * tile), dtype=np.float64)
    padded[:, :length] = q
    padded = padded.reshape(rows * pieces, tile // (lanes * group), lanes, group)
    acc = np.zeros((rows * pieces, lanes), dtype=np.float64)
    for m in range(padded.shape[1]):
        for i in range(group):
            acc = acc + padded[:, m, :, i]
    return _tree(acc).reshape(rows, pieces)


def _scale(acc: np.ndarray, C: float) -> np.ndarray:
    t = np.sqrt(acc) / np.float64(C)
    return np.where(t < 1.0, 1.0, t)  # a NaN t stays NaN


def _odd_float_bits(o: np.ndarray) -> np.ndarray:
    """The float32 nearest to ``o`` made odd where ``o`` is no float32: rounding it on to a narrower
    format gives what one rounding of ``o`` gives."""
    with np.errstate(over="ignore", under="ignore"):
        f = o.astype(np.float32)
    u = f.view(np.uint32).copy()
    back = f.astype(np.float64)
    inexact = back != o
    u[inexact & (np.abs(back) > np.abs(o))] -= np.uint32(1)
    u[inexact] |= np.uint32(1)
    return u


def _narrow(o: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> ``dtype``, one rounding to nearest even."""
    if dtype == torch.float64:
        return torch.from_numpy(np.ascontiguousarray(o))
    if dtype == torch.float32:
        with np.errstate(over="ignore", under="ignore"):
            return torch.from_numpy(o.astype(np.float32))
    u = _odd_float_bits(o)
    if dtype == torch.float16:
        with np.errstate(over="ignore", under="ignore"):
            return torch.from_numpy(u.view(np.float32).astype(np.float16))
    b = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return torch.from_numpy(b.view(np.int16)).view(torch.bfloat16)


def _widen(t: torch.Tensor, what: str) -> np.ndarray:
    if t.dtype not in _FLOAT_DTYPES:
        raise TypeError(f"{what}: the clip-and-noise pass takes fp32, fp16, bf16 and fp64 tensors, not {t.dtype}")
    x = t.detach().to(device="cpu", dtype=torch.float64).contiguous().reshape(-1).numpy()
    if not np.isfinite(x).all():
        raise ValueError(f"{what}: a non-finite element (the noise would hide it from the server's check)")
    return x


def _group(dtype: torch.dtype) -> int:
    return _native.kernel_constant(f"dp_ae_{_FLOAT_DTYPES[dtype]}")


def _check_scalars(C: float, sigma: float, seed: int | None, draw: int) -> tuple[float, float, int, int]:
    C, sigma = float(C), float(sigma)
    if not (math.isfinite(C) and C > 0):
        raise ValueError(f"the clipping norm C must be a finite number > 0, not {C}")
    noise_scale = sigma * C
    if not (math.isfinite(noise_scale) and noise_scale >= 0):
        raise ValueError(f"sigma * C must be a finite number >= 0, not {noise_scale}")
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    seed, draw = int(seed), int(draw)
    if not 0 <= seed < 1 << 64 or not 0 <= draw < 1 << 32:
        raise ValueError("the seed is a uint64 and the draw a uint32")
    return C, noise_scale, seed, draw


def _apply_host(x: np.ndarray, s: np.ndarray | np.float64, noise_scale: float, seed: int, draw: int,
                tensor_id: int) -> np.ndarray:
    y = x / s
    n = normal_stream(seed, draw, tensor_id, x.size) * np.float64(noise_scale)
    return y + n


_contexts: dict[torch.device, FedAvgContext] = {}


def _context(device: torch.device) -> FedAvgContext:
    ctx = _contexts.get(device)
    if ctx is None:
        # the pass does not depend on a context's layout: a one-element layout carries the device,
        # the stream order, the flag words and the call's workspace
        ctx = _contexts[device] = FedAvgContext(ModelLayout.flat(1, "dp"), device)
    return ctx


def _raise_on_input_flag(ctx: FedAvgContext, what: str) -> None:
    if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
        ctx.reset()  # the flag is sticky until reset: the context stays usable
        raise ValueError(f"{what}: a non-finite element (the noise would hide it from the server's check)")


def _rows_of(tensor: torch.Tensor) -> tuple[int, int]:
    """(rows, row length) as add_dp_noise sees them (dp.py:20-23)."""
    n = tensor.numel()
    if tensor.dim() <= 1:
        return 1, n
    rows = tensor.shape[0]
    return rows, (n // rows if rows else 0)


@torch.no_grad()
def add_dp_noise(tensor: torch.Tensor, C: float, sigma: float, *, seed: int | None, draw: int = 0,
                 tensor_id: int = 0) -> torch.Tensor:
    """Clip the L2 norm to ``C`` and add ``N(0, (sigma * C)**2)`` noise per element (dp.py:13-26): a
    2-D+ tensor row by row (``tensor.shape[0]`` rows), a 1-D tensor as one row. A new tensor of the
    same shape, dtype and device. Element ``i`` (counted through the whole tensor) takes deviate
    ``i`` of ``normal_stream(seed, draw, tensor_id, numel)``; ``seed=None`` draws a fresh seed from
    ``os.urandom`` (see the module docstring: not a cryptographic generator). Unlike the reference
    the arithmetic is fp64 with one final rounding into the tensor's dtype, and a non-finite element
    raises ``ValueError``."""
    if tensor.dtype not in _FLOAT_DTYPES:
        raise TypeError(f"the clip-and-noise pass takes fp32, fp16, bf16 and fp64 tensors, not {tensor.dtype}")
    C, noise_scale, seed, draw = _check_scalars(C, sigma, seed, draw)
    rows, length = _rows_of(tensor)
    if tensor.numel() == 0:
        return tensor.clone()
    if tensor.device.type == "cuda":
        ctx = _context(tensor.device)
        flat = tensor.detach().contiguous().reshape(-1)
        out = torch.empty_like(flat)
        ctx.dp_noise([flat], [out], C, noise_scale, seed, draw, [tensor_id], 0 if rows == 1 else length)
        _raise_on_input_flag(ctx, "add_dp_noise")
        return out.reshape(tensor.shape)
    x = _widen(tensor, "add_dp_noise")
    acc = _lanes_then_tree(_piece_partials((x * x).reshape(rows, length), _group(tensor.dtype)),
                           _native.kernel_constant("dp_threads"))
    s = np.repeat(_scale(acc, C), length)
    o = _apply_host(x, s, noise_scale, seed, draw, tensor_id)
    return _narrow(o, tensor.dtype).reshape(tensor.shape)


@torch.no_grad()
def add_dp_noise_to_parameter(parameter: Mapping[str, torch.Tensor], C: float, sigma: float, *, seed: int | None,
                              draw: int = 0) -> dict[str, torch.Tensor]:
    """Clip the total L2 norm of a parameter dict to ``C`` and add ``N(0, (sigma * C)**2)`` noise to
    every element (dp.py:29-47): a new dict of new tensors in the dtypes, shapes and devices of the
    inputs. Tensor ``k``'s stream id is its position in the dict. Tensors of one dtype on one GPU go
    through ``fedavg_dp_noise`` (three launches); host tensors and mixed dicts go through the numpy
    path, which gives the same bytes. A non-finite element raises ``ValueError``."""
    C, noise_scale, seed, draw = _check_scalars(C, sigma, seed, draw)
    items = list(parameter.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in _FLOAT_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: the clip-and-noise pass takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
    if not items:
        return {}
    devices, dtypes = {v.device for _, v in items}, {v.dtype for _, v in items}
    if len(devices) == 1 and len(dtypes) == 1 and items[0][1].device.type == "cuda":
        ctx = _context(items[0][1].device)
        flat = [v.detach().contiguous().reshape(-1) for _, v in items]
        outs = [torch.empty_like(f) for f in flat]
        ctx.dp_noise(flat, outs, C, noise_scale, seed, draw)
        _raise_on_input_flag(ctx, "add_dp_noise_to_parameter")
        return {name: o.reshape(v.shape) for (name, v), o in zip(items, outs)}
    xs = [_widen(v, name) for name, v in items]
    parts = [_piece_partials((x * x).reshape(1, -1), _group(v.dtype)) for x, (_, v) in zip(xs, items) if x.size]
    allparts = np.concatenate(parts, axis=1) if parts else np.zeros((1, 0))
    s = _scale(_lanes_then_tree(allparts, _native.kernel_constant("dp_threads")), C)[0]
    out = {}
    for t, (x, (name, v)) in enumerate(zip(xs, items)):
        o = _apply_host(x, s, noise_scale, seed, draw, t)
        out[name] = _narrow(o, v.dtype).reshape(v.shape).to(v.device)
    return out


# -- the endpoints (simulation_lib/topology/dp_endpoint.py) -----------------------------------
def _parameter_norm(parameter: Mapping[str, torch.Tensor]) -> float:
    return torch.linalg.vector_norm(torch.cat([v.reshape(-1).float() for v in parameter.values()])).item()


class _DifferentialPrivacyEndpointBase:
    """Wraps a client endpoint (any object with ``send(data)``): ``send`` clips and noises the
    update, then hands it on; every other attribute is the wrapped endpoint's. Keyword arguments
    ``C`` (1.0), ``epsilon`` (4.0), ``delta`` (1e-5) as in the reference (dp_endpoint.py:22-37), and
    ``seed`` (None: 64 bits of ``os.urandom`` per endpoint). ``draw`` starts at 0 and advances by
    one per ``send``, so no two sends of an endpoint share a stream. Without an ``endpoint`` the
    remaining keyword arguments build the simulator's ``ClientEndpoint`` (the reference's base
    class), which is how ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, endpoint: Any = None, **kwargs: Any) -> None:
        C: float = kwargs.pop("C", 1.0)
        epsilon: float = kwargs.pop("epsilon", 4.0)
        delta: float = kwargs.pop("delta", 1e-5)
        seed: int | None = kwargs.pop("seed", None)
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.C = float(C)
        self.sigma = compute_dp_sigma(epsilon=epsilon, delta=delta)
        self.seed = _check_scalars(self.C, self.sigma, seed, 0)[2]
        self.draw = 0
        _log.info("DP endpoint init: C=%.4f, epsilon=%.4f, delta=%.2e, sigma=%.4f", self.C, epsilon, delta,
                  self.sigma)

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def _next_draw(self) -> int:
        draw = self.draw
        self.draw = (draw + 1) & _U32
        return draw

    def _transform(self, data: Any) -> None:
        raise NotImplementedError

    def send(self, data: Any) -> None:
        self._transform(data)
        self._endpoint.send(data)


class DifferentialPrivacyEmbeddingEndpoint(_DifferentialPrivacyEndpointBase):
    """``FeatureMessage.feature`` goes out clipped and noised row by row (dp_endpoint.py:40-45);
    every other message passes unchanged."""

    def _transform(self, data: Any) -> None:
        if is_feature_message(data) and data.feature is not None:
            data.feature = add_dp_noise(data.feature, C=self.C, sigma=self.sigma, seed=self.seed,
                                        draw=self._next_draw())


class DifferentialPrivacyParameterEndpoint(_DifferentialPrivacyEndpointBase):
    """``ParameterMessage.parameter`` and ``DeltaParameterMessage.delta_parameter`` go out clipped to
    a total norm of ``C`` and noised (dp_endpoint.py:48-99), with the reference's noise statistics
    logged; every other message passes unchanged."""

    def _log_noise_stats(self, label: str, parameter: Mapping[str, torch.Tensor], pre_norm: float,
                         post_norm: float) -> None:
        n = sum(v.numel() for v in parameter.values())
        expected_noise_norm = self.sigma * self.C * math.sqrt(n)
        snr = pre_norm / expected_noise_norm if expected_noise_norm > 0 else float("inf")
        _log.info("DP endpoint%s: pre_noise_norm=%.6f, post_noise_norm=%.6f, expected_noise_norm=%.2f, SNR=%.4f, "
                  "C=%.4f, sigma=%.4f, num_params=%d", label, pre_norm, post_norm, expected_noise_norm, snr, self.C,
                  self.sigma, n)
        if snr < 1.0:
            _log.warning("DP endpoint%s: SNR=%.4f < 1.0, noise dominates signal! Consider increasing C "
                         "(currently %.4f) to at least %.2f", label, snr, self.C, pre_norm)

    def _noised(self, label: str, parameter: Mapping[str, torch.Tensor]) -> dict[str, torch.Tensor]:
        pre_norm = _parameter_norm(parameter)
        out = add_dp_noise_to_parameter(parameter, C=self.C, sigma=self.sigma, seed=self.seed,
                                        draw=self._next_draw())
        self._log_noise_stats(label, out, pre_norm, _parameter_norm(out))
        return out

    def _transform(self, data: Any) -> None:
        if is_parameter_message(data):
            data.parameter = self._noised("", data.parameter)
        elif is_delta_message(data):
            data.delta_parameter = self._noised(" (delta)", data.delta_parameter)
