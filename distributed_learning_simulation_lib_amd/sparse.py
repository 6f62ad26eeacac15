"""Sparse parameter diffs: the payload type and the client-side top-k step with error feedback.

The reference's ``worker/error_feedback_worker.py`` (``ErrorFeedbackWorker``) sends a *sparsified
parameter diff* and keeps what it did not send as a residual; its ``_sparsify`` is abstract.
``topk_sparsify`` is the scheme everybody reaches for, and ``SparseDelta`` is what it sends: a value
of ``DeltaParameterMessage.delta_parameter[name]``, the way ``QuantizedTensor`` is a value of
``ParameterMessage.parameter[name]``. A sparse delta is exactly a dense delta whose missing entries
are ``+0.0``: ``SparseFedAVGAlgorithm`` folds it as it is
(``fedavg_sparse_aggregate_delta``), every other algorithm gets ``to_dense()`` from the server.
"""

from __future__ import annotations

import math
from collections import OrderedDict
from collections.abc import Mapping
from dataclasses import dataclass

import torch

VALUE_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)
INT32_MAX = 2**31 - 1

# SparseDelta.dense's index tensors, least recently used first. A model has a few dozen distinct
# tensor sizes, so 64 entries hold a round's worth; past that the oldest goes (deltas that still
# use it keep it alive), so the cache stays at 4 bytes per element of the 64 sizes last used.
_ARANGE_CACHE: OrderedDict[tuple[int, torch.device], torch.Tensor] = OrderedDict()
_ARANGE_CACHE_ENTRIES = 64


@dataclass
class SparseDelta:
    """``nnz`` entries of one tensor of ``shape``: ``indices`` are strictly increasing int32 flat
    positions in ``[0, numel)`` (int64 is accepted and converted once), ``values`` the ``nnz`` values
    at them (float32 / float16 / bfloat16 / float64); every other element is ``+0.0``. The order of
    the indices is not checked here (it costs a pass over them): ``validate()`` does it on the host,
    the GPU fold does it on the device in the same call."""

    indices: torch.Tensor
    values: torch.Tensor
    shape: tuple[int, ...]

    def __post_init__(self) -> None:
        self.shape = tuple(int(s) for s in self.shape)
        if self.indices.dim() != 1 or self.values.dim() != 1 or self.indices.numel() != self.values.numel():
            raise ValueError("a sparse delta holds one 1-D index tensor and one 1-D value tensor of the same length")
        if self.numel > INT32_MAX:
            raise ValueError(f"{self.numel} elements: sparse indices are int32")
        if self.indices.dtype == torch.int64:
            self.indices = self.indices.to(torch.int32)
        if self.indices.dtype != torch.int32:
            raise ValueError(f"indices must be int32 (or int64), not {self.indices.dtype}")
        if self.values.dtype not in VALUE_DTYPES:
            raise ValueError(f"values must be float32 / float16 / bfloat16 / float64, not {self.values.dtype}")
        if self.indices.device != self.values.device:
            raise ValueError("indices and values must be on one device")
        if self.nnz > self.numel:
            raise ValueError(f"{self.nnz} entries for a tensor of {self.numel} elements")

    @property
    def numel(self) -> int:
        return math.prod(self.shape)

    @property
    def nnz(self) -> int:
        return self.indices.numel()

    @property
    def dtype(self) -> torch.dtype:
        return self.values.dtype

    @property
    def device(self) -> torch.device:
        return self.values.device

    def to(self, device: torch.device | str) -> SparseDelta:
        device = torch.device(device)
        if self.indices.device == device:
            return self
        return SparseDelta(self.indices.to(device), self.values.to(device), self.shape)

    def validate(self) -> None:
        """ValueError unless the indices are strictly increasing inside ``[0, numel)``."""
        i = self.indices
        if self.nnz and (int(i[0]) < 0 or int(i[-1]) >= self.numel or bool((i[1:] <= i[:-1]).any())):
            raise ValueError(f"sparse indices must be strictly increasing inside [0, {self.numel})")

    def to_dense(self) -> torch.Tensor:
        """The dense delta: the values at their positions, ``+0.0`` everywhere else."""
        self.validate()
        flat = torch.zeros(self.numel, dtype=self.values.dtype, device=self.values.device)
        flat[self.indices.to(torch.int64)] = self.values
        return flat.view(self.shape)

    @classmethod
    def dense(cls, t: torch.Tensor) -> SparseDelta:
        """Every element of ``t`` as an entry (the ``arange`` is cached per size and device)."""
        key = (t.numel(), t.device)
        idx = _ARANGE_CACHE.get(key)
        if idx is None:
            idx = _ARANGE_CACHE[key] = torch.arange(t.numel(), dtype=torch.int32, device=t.device)
            if len(_ARANGE_CACHE) > _ARANGE_CACHE_ENTRIES:
                _ARANGE_CACHE.popitem(last=False)
        else:
            _ARANGE_CACHE.move_to_end(key)
        return cls(idx, t.detach().reshape(-1), tuple(t.shape))


def is_sparse(parameter: Mapping[str, object]) -> bool:
    return any(isinstance(v, SparseDelta) for v in parameter.values())


def densify_parameter(parameter: Mapping[str, object]) -> dict[str, object]:
    """Every ``SparseDelta`` of ``parameter`` as its dense tensor, for consumers that take none."""
    return {k: v.to_dense() if isinstance(v, SparseDelta) else v for k, v in parameter.items()}


def topk_count(numel: int, k: int | None = None, ratio: float | None = None) -> int:
    """The number of entries kept: ``k`` itself, or ``ceil(ratio * numel)``; at least 1 for a
    non-empty tensor, at most ``numel``."""
    if (k is None) == (ratio is None):
        raise ValueError("give exactly one of k and ratio")
    if k is None:
        if not 0 < float(ratio) <= 1:
            raise ValueError(f"ratio must be in (0, 1], not {ratio}")
        k = math.ceil(float(ratio) * numel)
    if int(k) != k or k < 0:
        raise ValueError(f"k must be an integer >= 0, not {k}")
    return min(max(int(k), 1 if numel else 0), numel)


def topk_sparsify(delta: torch.Tensor, k: int | None = None, ratio: float | None = None,
                  error: torch.Tensor | None = None) -> tuple[SparseDelta, torch.Tensor]:
    """One ``ErrorFeedbackWorker`` step with top-k as the sparsifier: add the residual ``error`` to
    ``delta``, keep the ``k`` (or ``ceil(ratio * numel)``) entries of largest magnitude — ties go to
    the lower index — with their indices sorted ascending, and return them with what was not sent,
    the new residual. ``sent.to_dense() + residual == delta + error`` exactly: an element is either
    sent whole or kept whole."""
    total = delta if error is None else delta + error
    flat = total.detach().reshape(-1)
    keep = topk_count(flat.numel(), k, ratio)
    # a stable descending sort of the magnitudes keeps equal magnitudes in index order
    order = torch.sort(flat.abs(), descending=True, stable=True).indices[:keep]
    idx = torch.sort(order).values
    residual = flat.clone()
    residual[idx] = 0
    return SparseDelta(idx.to(torch.int32), flat[idx].clone(), tuple(delta.shape)), residual.view(delta.shape)
