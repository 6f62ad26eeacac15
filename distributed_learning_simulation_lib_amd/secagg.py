"""Secure aggregation by pairwise masking (Bonawitz, Ivanov, Kreuter, Marcedone, McMahan, Patel,
Ramage, Segal, Seth, "Practical Secure Aggregation for Privacy-Preserving Machine Learning", CCS 2017).

A client turns its parameter diff into fixed-point words of the ring Z/2^64, multiplies them by its
integer weight and adds masks that cancel in the sum: one per other worker of the round (``+`` towards
a higher id, ``-`` towards a lower one, both ends expanding the same pair seed) and one of its own
(the protocol's double masking). The server adds the words of the clients that reported, regenerates
and removes the survivors' own masks and the pair masks they share with workers that dropped out, and
learns the weighted sum and nothing else. ``MaskedDelta`` is what travels: a value of
``DeltaParameterMessage.delta_parameter[name]``. ``SecAggFedAVGAlgorithm`` is the server half. The
contract is DESIGN.md §5z and ``include/fedavg_hip.h``; on a GPU the client step is
``fedavg_secagg_mask`` (all tensors of a diff in one launch), and host tensors go through a numpy
composition of the same contract, which gives the same bits.

What is NOT here: ``SecAggSession`` derives every seed from one session seed with SHA-256. It stands
in for the protocol's Diffie-Hellman key agreement (which gives two clients their pair seed) and for
the Shamir secret sharing by which the server recovers the seeds of a round's dropouts and
survivors. Neither is simulated: whoever holds the session seed can unmask every client. And the
masks are expanded with Philox4x32-10, a counter-based generator made for simulation: it is not a
cryptographic generator. This module gives the arithmetic, the data flow and the cost of the
protocol, not its security.
"""

from __future__ import annotations

import dataclasses
import hashlib
import math
from collections.abc import Mapping, Sequence
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from . import _native
from .message import is_delta_message
from .quantized import philox4x32
from .sparse import INT32_MAX, VALUE_DTYPES

MAX_WEIGHT = (1 << 31) - 1
_U32 = 0xFFFFFFFF


@dataclass
class MaskedDelta:
    """The masked fixed-point words of one tensor of ``shape``: ``words`` is a flat int64 tensor of
    its element count (the bits of the ring words), ``frac_bits`` the encoding's fraction bits. On
    its own it is noise; only a round's sum can be decoded."""

    words: torch.Tensor
    shape: tuple[int, ...]
    frac_bits: int

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        if self.words.dtype != torch.int64 or self.words.dim() != 1 or self.words.numel() != math.prod(self.shape):
            raise ValueError(f"the words of shape {self.shape} are a 1-D int64 tensor of {math.prod(self.shape)} elements")
        if not 0 <= int(self.frac_bits) <= 52:
            raise ValueError(f"frac_bits is in 0 .. 52, not {self.frac_bits}")

    @property
    def device(self) -> torch.device:
        return self.words.device

    def to(self, device: torch.device | str) -> MaskedDelta:
        device = torch.device(device)
        return self if self.words.device == device else MaskedDelta(self.words.to(device), self.shape, self.frac_bits)


def is_masked(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, MaskedDelta) for v in parameter.values())


class SecAggSession:
    """The seeds of a session of ``worker_number`` workers, derived from ``seed`` with SHA-256: a
    stand-in for the protocol's key agreement and Shamir recovery, which are not simulated (see the
    module's docstring). ``pair_seed(i, j, round) == pair_seed(j, i, round)``."""

    def __init__(self, seed: int, worker_number: int) -> None:
        if not 1 <= int(worker_number) <= _native.SECAGG_MAX_CLIENTS:
            raise ValueError(f"a session has between 1 and {_native.SECAGG_MAX_CLIENTS} workers, not {worker_number}")
        self.seed, self.worker_number = int(seed), int(worker_number)

    def _derive(self, *what: object) -> int:
        text = "|".join(str(x) for x in ("secagg", self.seed, *what))
        return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")

    def _worker(self, i: int) -> int:
        if not 0 <= int(i) < self.worker_number:
            raise ValueError(f"worker {i} is not one of the session's {self.worker_number}")
        return int(i)

    def pair_seed(self, i: int, j: int, round: int) -> int:
        i, j = self._worker(i), self._worker(j)
        if i == j:
            raise ValueError("a pair seed belongs to two workers")
        return self._derive("pair", int(round), min(i, j), max(i, j))

    def self_seed(self, i: int, round: int) -> int:
        return self._derive("self", int(round), self._worker(i))

    def client_table(self, worker_id: int, round: int) -> tuple[list[int], list[int]]:
        """The seeds and signs of what worker ``worker_id`` adds to its words: its self seed, ``+``,
        and the pair seed of every other worker ``j``, ``+`` for ``worker_id < j``, ``-`` above."""
        i = self._worker(worker_id)
        others = [j for j in range(self.worker_number) if j != i]
        return ([self.self_seed(i, round)] + [self.pair_seed(i, j, round) for j in others],
                [1] + [1 if i < j else -1 for j in others])

    def server_table(self, reported: Sequence[int], dropped: Sequence[int], round: int) -> tuple[list[int], list[int]]:
        """The seeds and signs of what the server adds to the survivors' sum, i.e. the negated
        masks that did not cancel: every survivor's self seed and its pair seed with every dropout."""
        seeds = [self.self_seed(i, round) for i in reported]
        signs = [-1] * len(seeds)
        for i in reported:
            for d in dropped:
                seeds.append(self.pair_seed(i, d, round))
                signs.append(-1 if i < d else 1)
        return seeds, signs


def check_round_weights(weights: Sequence[float], value_bits: int) -> list[int]:
    """The integer weights of a round; ``ValueError`` for one that is no integer in 0 .. 2^31 - 1, or
    where ``value_bits + bit_length(sum)`` exceeds 63 (the true sum could wrap)."""
    out = []
    for w in weights:
        if w is None or float(w) != int(w) or not 0 <= int(w) <= MAX_WEIGHT:
            raise ValueError(f"a secure-aggregation weight is an integer in 0 .. 2^31 - 1, not {w}: scale the weights "
                             "to integers first")
        out.append(int(w))
    if not 1 <= int(value_bits) <= 62:
        raise ValueError(f"value_bits is in 1 .. 62, not {value_bits}")
    if int(value_bits) + sum(out).bit_length() > 63:
        raise ValueError(f"value_bits {value_bits} + {sum(out).bit_length()} bits of the total weight {sum(out)} exceed "
                         "63: the sum could wrap")
    return out


# ---- the numpy composition of the contract: host tensors, and the CPU device of the algorithm -------
def mask_words(seed: int, draw: int, t: int, n: int) -> np.ndarray:
    """``m(seed, draw, t, e)`` for ``e`` in ``0 .. n - 1`` as uint64."""
    blocks = np.arange((n + 1) // 2, dtype=np.uint64)
    ctr = np.empty((blocks.size, 4), dtype=np.uint32)
    ctr[:, 0] = (blocks & np.uint64(_U32)).astype(np.uint32)
    ctr[:, 1] = (blocks >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = t
    ctr[:, 3] = draw
    w = philox4x32(ctr, (seed & _U32, seed >> 32)).astype(np.uint64)
    return (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).reshape(-1)[:n]


def _masks(seeds: Sequence[int], signs: Sequence[int], draw: int, t: int, n: int) -> np.ndarray:
    acc = np.zeros(n, dtype=np.uint64)
    for seed, sign in zip(seeds, signs):
        m = mask_words(seed, draw, t, n)
        acc = acc + m if sign > 0 else acc - m
    return acc


def mask_numpy(x: torch.Tensor, weight: int, seeds: Sequence[int], signs: Sequence[int], draw: int, t: int,
               frac_bits: int, value_bits: int) -> torch.Tensor:
    """``fedavg_secagg_mask`` of one tensor (the ``t``-th of its call) in numpy: int64 words on the
    tensor's device. ``ValueError`` for an element out of range."""
    v = x.detach().reshape(-1).to(device="cpu", dtype=torch.float64).numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(v * 2.0 ** frac_bits)
        ok = np.abs(r) < 2.0 ** value_bits
    if not ok.all():
        raise ValueError("secagg_mask: an element is not finite or does not fit value_bits")
    q = r.astype(np.int64).astype(np.uint64) * np.uint64(weight)
    y = q + _masks(seeds, signs, draw, t, v.size)
    return torch.from_numpy(y.view(np.int64)).to(x.device)


def unmask_numpy(rows: Sequence[Sequence[torch.Tensor]], seeds: Sequence[int], signs: Sequence[int], draw: int,
                 frac_bits: int, total_weight: float, base: Sequence[torch.Tensor] | None,
                 out_dtype: torch.dtype) -> tuple[list[torch.Tensor], bool, bool]:
    """``fedavg_secagg_unmask`` in numpy: the outputs, and whether the result and the input flag
    would be latched."""
    outs, result_nan, input_nan = [], False, False
    for t in range(len(rows[0])):
        n = rows[0][t].numel()
        S = _masks(seeds, signs, draw, t, n)
        for row in rows:
            S = S + row[t].reshape(-1).cpu().numpy().view(np.uint64)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = (S.view(np.int64).astype(np.float64) * 2.0 ** -frac_bits) / np.float64(total_weight)
        result_nan |= bool(np.isnan(g).any())
        if base is not None:
            b = base[t].detach().reshape(-1).to(device="cpu", dtype=torch.float64).numpy()
            input_nan |= bool(np.isnan(b).any())
            g = b + g
        outs.append(torch.from_numpy(g).to(out_dtype))
    return outs, result_nan, input_nan


# ---- the client step ------------------------------------------------------------------------------
_contexts: dict[torch.device, Any] = {}


def _context(device: torch.device) -> Any:
    ctx = _contexts.get(device)
    if ctx is None:
        from .fedavg import FedAvgContext, ModelLayout  # fedavg imports this package's payloads

        # the step does not depend on a context's layout: a one-element layout carries the device,
        # the stream order, the flag words and the call's tables
        ctx = _contexts[device] = FedAvgContext(ModelLayout.flat(1, "secagg"), device)
    return ctx


def secagg_mask_parameter(delta: Mapping[str, torch.Tensor], weight: int, session: SecAggSession, worker_id: int,
                          round: int, frac_bits: int = 24, value_bits: int = 40) -> dict[str, MaskedDelta]:
    """A parameter diff as ``MaskedDelta`` values: per tensor (the ``t``-th non-empty one of ``delta``) and element,
    ``rint(x * 2^frac_bits) * weight`` plus worker ``worker_id``'s masks of ``round`` in Z/2^64.
    ``weight`` is an integer in 0 .. 2^31 - 1 (a fractional weight is a ``ValueError``), and so is an
    element that is not finite or whose scaled value reaches ``2^value_bits``. Non-empty tensors of
    one floating dtype on one GPU go through one ``fedavg_secagg_mask`` call; host tensors and every
    other mix go through the numpy composition, which gives the same bits."""
    (weight,) = check_round_weights([weight], value_bits)
    if not 0 <= int(frac_bits) <= 52:
        raise ValueError(f"frac_bits is in 0 .. 52, not {frac_bits}")
    items = list(delta.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in VALUE_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: secure aggregation takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
        if value.numel() > INT32_MAX:
            raise ValueError(f"{name}: more than 2^31 - 1 elements")
    seeds, signs = session.client_table(worker_id, round)
    values = [v for _, v in items if v.numel() > 0]  # tensor t of the stream is the t-th non-empty one
    on_gpu = (values and all(v.device.type == "cuda" for v in values)
              and len({v.device for v in values}) == 1 and len({v.dtype for v in values}) == 1)
    if on_gpu:
        flat = [v.detach().contiguous().reshape(-1) for v in values]
        words = [torch.empty(f.numel(), dtype=torch.int64, device=f.device) for f in flat]
        ctx = _context(flat[0].device)
        ctx.secagg_mask(flat, words, weight, seeds, signs, round, frac_bits, value_bits)
        if ctx.flags() & _native.FLAG_INPUT_NAN:  # waits for the stream
            ctx.reset()  # the flag is sticky until reset: the context stays usable
            raise ValueError("secagg_mask: an element is not finite or does not fit value_bits")
    else:
        words = [mask_numpy(v, weight, seeds, signs, round, t, frac_bits, value_bits) for t, v in enumerate(values)]
    full = iter(words)
    return {name: MaskedDelta(next(full) if v.numel() else torch.empty(0, dtype=torch.int64, device=v.device),
                              tuple(v.shape), frac_bits) for name, v in items}


class SecAggEndpoint:
    """Wraps a client endpoint (any object with ``send(data)``): a ``DeltaParameterMessage`` goes out
    with its ``delta_parameter`` masked for the round (the endpoint counts the deltas it sent: round
    0, 1, ...) under the message's ``aggregation_weight``; everything else passes unchanged. Every
    other attribute is the wrapped endpoint's. Without an ``endpoint`` the remaining keyword
    arguments build the simulator's ``ClientEndpoint``, which is how
    ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, endpoint: Any = None, *, session_seed: int, worker_id: int, worker_number: int,
                 frac_bits: int = 24, value_bits: int = 40, **kwargs: Any) -> None:
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.session = SecAggSession(session_seed, worker_number)
        self.worker_id, self.frac_bits, self.value_bits = int(worker_id), int(frac_bits), int(value_bits)
        self.round = 0

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def send(self, data: Any) -> None:
        if is_delta_message(data):
            masked = secagg_mask_parameter(data.delta_parameter, data.aggregation_weight, self.session, self.worker_id,
                                           self.round, self.frac_bits, self.value_bits)
            data = dataclasses.replace(data, delta_parameter=masked)
            self.round += 1
        self._endpoint.send(data)
