"""Randomly rotated 1-bit compression of parameter diffs with error feedback (DRIVE: Vargaftik,
Ben-Basat, Portnoy, Mendelson, Ben-Itzhak, Mitzenmacher, "DRIVE: One-bit Distributed Mean Estimation",
NeurIPS 2021; the random rotation of Suresh, Yu, Kumar, McMahan, ICML 2017).

A client sends one bit per coordinate, as ``sign.SignDelta`` does, but the bits are the signs of the
diff after a randomised Walsh-Hadamard rotation ``y = H_B (D u)``, and one magnitude per block of
``B`` coordinates. The error of the plain scaled sign depends on the shape of the data (it keeps almost
nothing of a heavy-tailed or sparse diff); the error after the rotation does not. The rotation is
linear and shared by the clients of a round (one ``seed``, one ``draw`` per round), so the server folds
the bits in the rotated domain and inverts the rotation once (``RotatedSignFedAVGAlgorithm``,
``fedavg_rsign_aggregate_delta``); every other algorithm gets ``to_dense()`` from the server. On a GPU
the client step is ``fedavg_rsign_compress``: all tensors of a diff in one launch; host
tensors, and dicts that mix dtypes or devices, go through a numpy composition of the same contract,
which gives the same bits and is the kernel's oracle. ``RotatedSignErrorFeedback`` keeps the residuals
and ``RotatedSignEndpoint`` puts the step in front of a client endpoint.
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

MODES = {"unbiased": _native.RSIGN_UNBIASED, "mse": _native.RSIGN_MSE}
MAX_BLOCK, MIN_BLOCK = 4096, 64  # fedavg_kernel_constant "rsign_tile" and "rsign_min_block"
_U32 = 0xFFFFFFFF


def geometry(numel: int) -> tuple[int, int, int]:
    """``(B, nb, n_pad)`` of a tensor of ``numel >= 1`` elements: the block size ``min(4096, max(64,
    next_pow2(numel)))``, the number of blocks and the padded length."""
    B = min(MAX_BLOCK, max(MIN_BLOCK, 1 << (numel - 1).bit_length()))
    nb = (numel + B - 1) // B
    return B, nb, nb * B


def scale_dtype(dtype: torch.dtype) -> torch.dtype:
    """The dtype of the block magnitudes of a ``dtype`` diff: fp64 for fp64, fp32 otherwise."""
    return torch.float64 if dtype == torch.float64 else torch.float32


def _check_stream(seed: int, draw: int, tensor_id: int) -> None:
    if not 0 <= int(seed) < 1 << 64 or not 0 <= int(draw) < 1 << 32 or not 0 <= int(tensor_id) < 1 << 32:
        raise ValueError("the seed is a uint64, the draw and the tensor id are uint32")


def diagonal(seed: int, draw: int, tensor_id: int, n_pad: int) -> np.ndarray:
    """Where ``D`` is -1 (bool, ``n_pad`` elements): element ``e`` takes bit ``e % 32`` of word ``(e %
    128) // 32`` of the Philox4x32-10 block ``e // 128`` under the key ``(seed & 0xffffffff, seed >>
    32)`` and the counter ``(block & 0xffffffff, block >> 32, tensor_id, draw)``."""
    from .quantized import philox4x32  # quantized imports fedavg, which imports this package's payloads

    _check_stream(seed, draw, tensor_id)
    blocks = np.arange((n_pad + 127) // 128, dtype=np.uint64)
    ctr = np.empty((blocks.size, 4), dtype=np.uint32)
    ctr[:, 0] = (blocks & np.uint64(_U32)).astype(np.uint32)
    ctr[:, 1] = (blocks >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = tensor_id
    ctr[:, 3] = draw
    out = philox4x32(ctr, (int(seed) & _U32, int(seed) >> 32))
    bits = (out[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(-1)[:n_pad].astype(bool)


def hadamard(x: np.ndarray) -> np.ndarray:
    """``H_B`` of every row of the fp64 array ``x`` ([nb, B]), unnormalised: the levels ``h = 1, 2, 4,
    ..., B / 2`` in that order, every pair ``(i, i + h)`` with ``i & h == 0`` becoming ``(a + b, a -
    b)``, each one rounded fp64 operation."""
    nb, B = x.shape
    y = x.astype(np.float64, copy=True)
    h = 1
    with np.errstate(over="ignore", invalid="ignore"):
        while h < B:
            v = y.reshape(nb, B // (2 * h), 2, h)
            a, b = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
            v[:, :, 0, :] = a + b
            v[:, :, 1, :] = a - b
            h *= 2
    return y


def tree_sum(x: np.ndarray) -> np.ndarray:
    """The fp64 sum of every row of ``x`` ([nb, B], B a power of two) by the adjacent-pair tree in
    index order: one level is ``x[2 i] + x[2 i + 1]``."""
    with np.errstate(over="ignore", invalid="ignore"):
        while x.shape[1] > 1:
            x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _signed(neg: np.ndarray, x: np.ndarray) -> np.ndarray:
    return np.where(neg, -x, x)


@dataclass
class RotatedSignDelta:
    """The rotated signs and the block magnitudes of one tensor of ``shape``, with ``(B, nb, n_pad) =
    geometry(numel)``: ``bits`` is a uint8 tensor of ``n_pad / 8`` bytes, 8-byte aligned, in the bit
    layout of ``SignDelta`` (padding coordinates are real coordinates of the rotated block and carry
    bits); ``scales`` holds ``nb`` magnitudes, float32 for float32 / float16 / bfloat16 diffs and
    float64 for float64 diffs, on the device of ``bits``; ``dtype`` is the diff's. ``seed``, ``draw``
    and ``tensor_id`` name the diagonal ``D``. The tensor is ``D H_B (-+scale)``."""

    bits: torch.Tensor
    scales: torch.Tensor
    shape: tuple[int, ...]
    seed: int
    draw: int
    tensor_id: int
    dtype: torch.dtype = torch.float32

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        self.seed, self.draw, self.tensor_id = int(self.seed), int(self.draw), int(self.tensor_id)
        _check_stream(self.seed, self.draw, self.tensor_id)
        if not 1 <= self.numel <= INT32_MAX:
            raise ValueError(f"{self.numel} elements: a rotated sign delta holds between 1 and 2^31 - 1")
        if self.dtype not in VALUE_DTYPES:
            raise ValueError("the diff's dtype is float32 / float16 / bfloat16 / float64")
        _, nb, n_pad = geometry(self.numel)
        if self.bits.dtype != torch.uint8 or self.bits.dim() != 1 or self.bits.numel() != n_pad // 8:
            raise ValueError(f"the bits of {self.numel} elements are a 1-D uint8 tensor of {n_pad // 8} bytes")
        if self.scales.dtype != scale_dtype(self.dtype) or self.scales.dim() != 1 or self.scales.numel() != nb:
            raise ValueError(f"the scales of {self.numel} {self.dtype} elements are a 1-D {scale_dtype(self.dtype)} "
                             f"tensor of {nb} elements")
        if self.bits.device != self.scales.device:
            raise ValueError("bits and scales must be on one device")

    @property
    def numel(self) -> int:
        return math.prod(self.shape)

    @property
    def device(self) -> torch.device:
        return self.bits.device

    def to(self, device: torch.device | str) -> RotatedSignDelta:
        device = torch.device(device)
        if self.bits.device == device:
            return self
        return dataclasses.replace(self, bits=self.bits.to(device), scales=self.scales.to(device))

    def to_dense(self) -> torch.Tensor:
        """The dense delta ``D H_B (-+scale)`` rounded once into the diff's dtype, as a numpy
        composition of the contract (what ``fedavg_rsign_compress`` calls ``sent``)."""
        from .dp import _narrow  # dp imports fedavg, which imports this package's payloads

        n = self.numel
        B, nb, n_pad = geometry(n)
        neg = np.unpackbits(self.bits.cpu().numpy(), bitorder="little")[:n_pad].astype(bool).reshape(nb, B)
        s = self.scales.cpu().to(torch.float64).numpy()[:, None]
        z = hadamard(_signed(neg, np.broadcast_to(s, (nb, B)))).reshape(-1)
        sent = _signed(diagonal(self.seed, self.draw, self.tensor_id, n_pad), z)[:n]
        return _narrow(sent, self.dtype).view(self.shape).to(self.device)


def is_rotated(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, RotatedSignDelta) for v in parameter.values())


def densify_parameter(parameter: Mapping[str, object]) -> dict[str, object]:
    """Every ``RotatedSignDelta`` of ``parameter`` as its dense tensor, for consumers that take none."""
    return {k: v.to_dense() if isinstance(v, RotatedSignDelta) else v for k, v in parameter.items()}


def _check_mode(mode: str) -> None:
    if mode not in MODES:
        raise ValueError(f"the mode is one of {sorted(MODES)}, not {mode!r}")


@torch.no_grad()
def _rotated_sign_compress_numpy(delta: torch.Tensor, error: torch.Tensor | None = None, *, seed: int, draw: int,
                                 tensor_id: int = 0, mode: str = "unbiased") -> tuple[RotatedSignDelta, torch.Tensor]:
    """``rotated_sign_compress`` as a numpy composition of the contract (include/fedavg_hip.h,
    ``fedavg_rsign_compress``): the path of host tensors, and the oracle of the kernel."""
    from .dp import _narrow  # dp imports fedavg, which imports this package's payloads

    dtype, device = delta.dtype, delta.device
    total = (delta if error is None else delta + error).detach().to("cpu").reshape(-1)
    n = total.numel()
    B, nb, n_pad = geometry(n)
    t64 = total.to(torch.float64).numpy()
    if not np.isfinite(t64).all():
        raise ValueError("rotated_sign_compress: a non-finite element")
    D = diagonal(seed, draw, tensor_id, n_pad)
    u = np.zeros(n_pad, dtype=np.float64)
    u[:n] = _signed(D[:n], t64)
    y = hadamard(u.reshape(nb, B))
    with np.errstate(all="ignore"):
        l1, l2 = tree_sum(np.abs(y)), tree_sum(y * y)
        sigma = l2 / l1 if mode == "unbiased" else l1 / np.float64(B)
        s = np.where(l1 == 0, 0.0, sigma / np.float64(B))
    scales = _narrow(s, scale_dtype(dtype))
    neg = np.signbit(y)
    z = hadamard(_signed(neg, np.broadcast_to(scales.to(torch.float64).numpy()[:, None], (nb, B)))).reshape(-1)
    sent = _narrow(_signed(D, z)[:n], dtype).to(torch.float64).numpy()
    residual = _narrow(t64 - sent, dtype).view(delta.shape).to(device)  # exact in fp64 up to the one rounding
    bits = torch.from_numpy(np.packbits(neg.reshape(-1), bitorder="little"))
    return (RotatedSignDelta(bits.to(device), scales.to(device), tuple(delta.shape), seed, draw, tensor_id, dtype),
            residual)


def _for_kernel(delta: torch.Tensor, error: torch.Tensor | None) -> bool:
    """The kernel takes a non-empty floating tensor on a GPU of at most 2^31 - 1 elements, with a
    residual (if any) of its own shape, dtype and device; the composition takes everything else."""
    return (delta.device.type == "cuda" and delta.dtype in VALUE_DTYPES and 0 < delta.numel() <= INT32_MAX
            and (error is None or (error.shape == delta.shape and error.dtype == delta.dtype
                                   and error.device == delta.device)))


@torch.no_grad()
def _rotated_sign_compress_kernel(deltas: list[torch.Tensor], errors: list[torch.Tensor | None], seed: int, draw: int,
                                  tensor_ids: list[int], mode: str) -> list[tuple[RotatedSignDelta, torch.Tensor]]:
    """One ``fedavg_rsign_compress`` call over tensors of one dtype on one GPU."""
    from .sign import _context  # the layout-free context of a device, shared with the sign step

    device, dtype = deltas[0].device, deltas[0].dtype
    flat = [d.detach().contiguous().reshape(-1) for d in deltas]
    err = [None if e is None else e.detach().contiguous().reshape(-1) for e in errors]
    geo = [geometry(f.numel()) for f in flat]
    bits = [torch.empty(n_pad // 8, dtype=torch.uint8, device=device) for _, _, n_pad in geo]
    scales = [torch.empty(nb, dtype=scale_dtype(dtype), device=device) for _, nb, _ in geo]
    res = [torch.empty_like(f) for f in flat]
    ctx = _context(device)
    ctx.rsign_compress(flat, err, bits, scales, res, seed=seed, draw=draw, tensor_ids=tensor_ids, mode=mode)
    if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
        ctx.reset()  # the flag is sticky until reset: the context stays usable
        raise ValueError("rotated_sign_compress: a non-finite element")
    return [(RotatedSignDelta(b, s, tuple(d.shape), seed, draw, i, dtype), r.view(d.shape))
            for d, b, s, r, i in zip(deltas, bits, scales, res, tensor_ids)]


def rotated_sign_compress(delta: torch.Tensor, error: torch.Tensor | None = None, *, seed: int, draw: int,
                          tensor_id: int = 0, mode: str = "unbiased") -> tuple[RotatedSignDelta, torch.Tensor]:
    """One ``ErrorFeedbackWorker`` step with the rotated sign as the compressor: ``total = delta +
    error`` (rounded once into the dtype), ``y = H_B (D total)`` per block of ``B = min(4096, max(64,
    next_pow2(numel)))`` coordinates, one bit per padded coordinate (the sign of ``y``), and per block
    the magnitude ``|y|_2^2 / |y|_1 / B`` (``mode="unbiased"``: DRIVE's scale, for use without error
    feedback) or ``|y|_1 / B^2`` (``mode="mse"``: the contraction that error feedback wants);
    ``residual = total - D H_B (-+scale)`` (rounded once). ``seed`` and ``draw`` (one per round, shared
    by the clients) and ``tensor_id`` name the diagonal ``D``. Returns the ``RotatedSignDelta`` and the
    new residual. A floating tensor on a GPU goes through ``fedavg_rsign_compress``,
    which gives the same bits. An empty tensor and a non-finite element are a ``ValueError``."""
    _check_mode(mode)
    _check_stream(seed, draw, tensor_id)
    if delta.dtype not in VALUE_DTYPES:
        raise TypeError(f"rotated sign compression takes fp32, fp16, bf16 and fp64 tensors, not {delta.dtype}")
    if delta.numel() == 0:
        raise ValueError("rotated sign compression of an empty tensor: it has no block")
    if _for_kernel(delta, error):
        return _rotated_sign_compress_kernel([delta], [error], seed, draw, [tensor_id], mode)[0]
    return _rotated_sign_compress_numpy(delta, error, seed=seed, draw=draw, tensor_id=tensor_id, mode=mode)


def rotated_sign_compress_parameter(delta: Mapping[str, torch.Tensor], error: Mapping[str, torch.Tensor] | None = None,
                                    *, seed: int, draw: int, mode: str = "unbiased",
                                    ) -> tuple[dict[str, RotatedSignDelta], dict[str, torch.Tensor]]:
    """``rotated_sign_compress`` per tensor of a parameter diff, the tensor id being the name's
    position in ``delta`` (a name that ``error`` lacks has no residual yet). Returns the deltas and
    the new residuals, both by name. Tensors of one floating dtype on one GPU go through one
    ``fedavg_rsign_compress`` call; host tensors, mixed dtypes and dicts spread over several devices
    go tensor by tensor. A non-floating or empty tensor is refused."""
    _check_mode(mode)
    items = list(delta.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in VALUE_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: rotated sign compression takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
    errors = [None if error is None else error.get(name) for name, _ in items]
    results: list[Any] = [None] * len(items)
    fit = [k for k, ((_, v), e) in enumerate(zip(items, errors)) if _for_kernel(v, e)]
    if fit and len({items[k][1].device for k in fit}) == 1 and len({items[k][1].dtype for k in fit}) == 1:
        done = _rotated_sign_compress_kernel([items[k][1] for k in fit], [errors[k] for k in fit], seed, draw, fit, mode)
        for k, r in zip(fit, done):
            results[k] = r
    for k, ((_, v), e) in enumerate(zip(items, errors)):
        if results[k] is None:
            results[k] = rotated_sign_compress(v, e, seed=seed, draw=draw, tensor_id=k, mode=mode)
    return ({name: r[0] for (name, _), r in zip(items, results)},
            {name: r[1] for (name, _), r in zip(items, results)})


def fold_numpy(rows: list[list[RotatedSignDelta]], weights: list[float], divisor: float, base: list[torch.Tensor],
               out_dtype: torch.dtype) -> tuple[list[torch.Tensor], tuple[bool, bool, bool]]:
    """``fedavg_rsign_aggregate_delta`` restated in numpy, tensor by tensor: ``d_i = -+s_i``, ``p_i =
    d_i * w_i``, ``acc = p_0 + p_1 + ...`` in table order, ``m = acc / divisor``, ``z = H_B m``, ``out
    = base + D z``. Returns the outputs (CPU tensors of ``out_dtype``) and the three NaN flags (input,
    accumulator, result), collected over all tensors."""
    outs = []
    input_nan = acc_nan = result_nan = False
    for t, b in enumerate(base):
        first = rows[0][t]
        n = first.numel
        B, nb, n_pad = geometry(n)
        acc = None
        with np.errstate(all="ignore"):
            for row, w in zip(rows, weights):
                d = row[t]
                neg = np.unpackbits(d.bits.cpu().numpy(), bitorder="little")[:n_pad].astype(bool).reshape(nb, B)
                s = d.scales.cpu().to(torch.float64).numpy()[:, None]
                input_nan |= bool(np.isnan(s).any())
                p = _signed(neg, np.broadcast_to(s, (nb, B))) * np.float64(w)
                acc = p if acc is None else acc + p
            acc_nan |= bool(np.isnan(acc).any())
            z = hadamard(acc / np.float64(divisor)).reshape(-1)
            out = b.detach().cpu().reshape(-1).numpy() + _signed(
                diagonal(first.seed, first.draw, first.tensor_id, n_pad), z)[:n]
        result_nan |= bool(np.isnan(out).any())
        outs.append(torch.from_numpy(out).to(out_dtype))
    return outs, (input_nan, acc_nan, result_nan)


class RotatedSignErrorFeedback:
    """The ``_sparsify`` step of the reference's ``ErrorFeedbackWorker`` with the rotated sign as the
    scheme, and its ``_get_error`` / ``_set_error`` state: one residual per tensor name. The ``draw``
    of a round is the number of earlier ``compress`` calls, so clients that share ``seed`` and call
    once per round share the round's rotation."""

    def __init__(self, seed: int, mode: str = "mse") -> None:
        _check_mode(mode)
        _check_stream(seed, 0, 0)
        self.seed, self.mode = int(seed), mode
        self.draw = 0
        self._error: dict[str, torch.Tensor] = {}

    def error(self, name: str) -> torch.Tensor | None:
        """The residual kept for ``name``, or ``None`` before its first round."""
        return self._error.get(name)

    def reset(self) -> None:
        self._error.clear()
        self.draw = 0

    def compress(self, message: Any) -> Any:
        """A new message of the class of ``message`` (a ``DeltaParameterMessage``) whose non-empty
        floating tensors travel as ``RotatedSignDelta`` (tensor id: the name's position among
        them); every other field is copied, every other value passes unchanged. Keeps
        the new residuals and counts the draw. ``ValueError`` for a name whose shape or dtype changed."""
        dense = {n: v for n, v in message.delta_parameter.items()
                 if isinstance(v, torch.Tensor) and v.dtype in VALUE_DTYPES and v.numel() > 0}
        for name, value in dense.items():
            e = self._error.get(name)
            if e is not None and (e.shape != value.shape or e.dtype != value.dtype):
                raise ValueError(f"{name}: {tuple(value.shape)} {value.dtype} now, {tuple(e.shape)} {e.dtype} in the "
                                 "round before: reset() the residuals of a changed model")
            if e is not None and e.device != value.device:
                self._error[name] = e.to(value.device)
        sent, residual = rotated_sign_compress_parameter(dense, self._error, seed=self.seed, draw=self.draw,
                                                         mode=self.mode)
        self._error.update(residual)
        self.draw += 1
        return dataclasses.replace(
            message, delta_parameter={n: sent.get(n, v) for n, v in message.delta_parameter.items()})


class RotatedSignEndpoint:
    """Wraps a client endpoint (any object with ``send(data)``): a ``DeltaParameterMessage`` goes out
    compressed by the endpoint's ``RotatedSignErrorFeedback(seed, mode)``, everything else unchanged.
    Every client of a session takes the same ``seed``. Every other attribute is the wrapped endpoint's.
    Without an ``endpoint`` the keyword arguments build the simulator's ``ClientEndpoint``, which is
    how ``AlgorithmRepository.create_client`` constructs it (``endpoint_kwargs: {seed}``)."""

    def __init__(self, endpoint: Any = None, *, seed: int, mode: str = "mse", **kwargs: Any) -> None:
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.feedback = RotatedSignErrorFeedback(seed, mode)

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def send(self, data: Any) -> None:
        self._endpoint.send(self.feedback.compress(data) if is_delta_message(data) else data)
