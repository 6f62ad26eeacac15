"""Sparse parameter diffs: the payload type and the client-side top-k step with error feedback.

The reference's ``worker/error_feedback_worker.py`` (``ErrorFeedbackWorker``) sends a *sparsified
parameter diff* and keeps what it did not send as a residual; its ``_sparsify`` is abstract.
``topk_sparsify`` is the scheme everybody reaches for, and ``SparseDelta`` is what it sends: a value
of ``DeltaParameterMessage.delta_parameter[name]``, the way ``QuantizedTensor`` is a value of
``ParameterMessage.parameter[name]``. A sparse delta is exactly a dense delta whose missing entries
are ``+0.0``: ``SparseFedAVGAlgorithm`` folds it as it is
(``fedavg_sparse_aggregate_delta``), every other algorithm gets ``to_dense()`` from the server.
On a GPU the top-k step is ``fedavg_topk_sparsify``: a radix select instead of the
two sorts, for all tensors of a diff in one call; ``TopKErrorFeedback`` keeps the residuals and
``TopKSparseEndpoint`` puts the step in front of a client endpoint.
"""

from __future__ import annotations

import dataclasses
import math
from collections import OrderedDict
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Any

import torch

from .message import is_delta_message

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


def _topk_sparsify_torch(delta: torch.Tensor, k: int | None = None, ratio: float | None = None,
                          error: torch.Tensor | None = None) -> tuple[SparseDelta, torch.Tensor]:
    """``topk_sparsify`` as a torch composition: the path of host tensors, and the oracle of the kernel."""
    total = delta if error is None else delta + error
    flat = total.detach().reshape(-1)
    keep = topk_count(flat.numel(), k, ratio)
    # a stable descending sort of the magnitudes keeps equal magnitudes in index order
    order = torch.sort(flat.abs(), descending=True, stable=True).indices[:keep]
    idx = torch.sort(order).values
    residual = flat.clone()
    residual[idx] = 0
    return SparseDelta(idx.to(torch.int32), flat[idx].clone(), tuple(delta.shape)), residual.view(delta.shape)


_contexts: dict[torch.device, Any] = {}


def _context(device: torch.device) -> Any:
    ctx = _contexts.get(device)
    if ctx is None:
        from .fedavg import FedAvgContext, ModelLayout  # fedavg imports this module

        # the step does not depend on a context's layout: a one-element layout carries the device,
        # the stream order and the call's workspace
        ctx = _contexts[device] = FedAvgContext(ModelLayout.flat(1, "topk"), device)
    return ctx


def _for_kernel(delta: torch.Tensor, error: torch.Tensor | None) -> bool:
    """The kernel takes a floating tensor on a GPU of at most 2^31 - 1 elements, with a residual (if
    any) of its own shape, dtype and device; the torch composition takes everything else."""
    return (delta.device.type == "cuda" and delta.dtype in VALUE_DTYPES and delta.numel() <= INT32_MAX
            and (error is None or (error.shape == delta.shape and error.dtype == delta.dtype
                                   and error.device == delta.device)))


@torch.no_grad()
def _topk_sparsify_kernel(deltas: list[torch.Tensor], keeps: list[int],
                          errors: list[torch.Tensor | None]) -> list[tuple[SparseDelta, torch.Tensor]]:
    """One ``fedavg_topk_sparsify`` call over tensors of one dtype on one GPU."""
    device, dtype = deltas[0].device, deltas[0].dtype
    flat = [d.detach().contiguous().reshape(-1) for d in deltas]
    err = [None if e is None else e.detach().contiguous().reshape(-1) for e in errors]
    idx = [torch.empty(k, dtype=torch.int32, device=device) for k in keeps]
    val = [torch.empty(k, dtype=dtype, device=device) for k in keeps]
    res = [torch.empty_like(f) for f in flat]
    _context(device).topk_sparsify(flat, err, keeps, idx, val, res)
    return [(SparseDelta(i, v, tuple(d.shape)), r.view(d.shape)) for d, i, v, r in zip(deltas, idx, val, res)]


def topk_sparsify(delta: torch.Tensor, k: int | None = None, ratio: float | None = None,
                  error: torch.Tensor | None = None) -> tuple[SparseDelta, torch.Tensor]:
    """One ``ErrorFeedbackWorker`` step with top-k as the sparsifier: add the residual ``error`` to
    ``delta``, keep the ``k`` (or ``ceil(ratio * numel)``) entries of largest magnitude — ties go to
    the lower index — with their indices sorted ascending, and return them with what was not sent,
    the new residual. ``sent.to_dense() + residual == delta + error`` exactly: an element is either
    sent whole or kept whole. A floating tensor on a GPU goes through ``fedavg_topk_sparsify``
    (DESIGN.md §5s), which gives the same bits without a sort."""
    if _for_kernel(delta, error):
        return _topk_sparsify_kernel([delta], [topk_count(delta.numel(), k, ratio)], [error])[0]
    return _topk_sparsify_torch(delta, k, ratio, error)


def topk_sparsify_parameter(delta: Mapping[str, torch.Tensor], k: int | None = None, ratio: float | None = None,
                            error: Mapping[str, torch.Tensor] | None = None,
                            ) -> tuple[dict[str, SparseDelta], dict[str, torch.Tensor]]:
    """``topk_sparsify`` per tensor of a parameter diff: tensor ``n`` keeps ``topk_count(numel_n, k,
    ratio)`` entries of ``delta[n] + error[n]`` (a name that ``error`` lacks has no residual yet).
    Returns the sent entries and the new residuals, both by name. Tensors of one floating dtype on
    one GPU go through one ``fedavg_topk_sparsify`` call; host tensors, mixed dtypes and dicts spread
    over several devices go tensor by tensor. A non-floating tensor is a ``TypeError``."""
    items = list(delta.items())
    for name, value in items:
        if not isinstance(value, torch.Tensor) or value.dtype not in VALUE_DTYPES:
            kind = value.dtype if isinstance(value, torch.Tensor) else type(value).__name__
            raise TypeError(f"{name}: top-k takes fp32, fp16, bf16 and fp64 tensors, not {kind}")
    keeps = [topk_count(v.numel(), k, ratio) for _, v in items]
    errors = [None if error is None else error.get(name) for name, _ in items]
    if (items and len({v.device for _, v in items}) == 1 and len({v.dtype for _, v in items}) == 1
            and all(_for_kernel(v, e) for (_, v), e in zip(items, errors))):
        results = _topk_sparsify_kernel([v for _, v in items], keeps, errors)
    else:
        results = [topk_sparsify(v, k=keep, error=e) for (_, v), keep, e in zip(items, keeps, errors)]
    return ({name: r[0] for (name, _), r in zip(items, results)},
            {name: r[1] for (name, _), r in zip(items, results)})


class TopKErrorFeedback:
    """The ``_sparsify`` step of the reference's ``ErrorFeedbackWorker`` with top-k as the scheme, and
    its ``_get_error`` / ``_set_error`` state: one residual per tensor name, added to the next
    round's diff before the top ``k`` (or ``ceil(ratio * numel)``) entries of each tensor go out."""

    def __init__(self, k: int | None = None, ratio: float | None = None) -> None:
        topk_count(1, k, ratio)  # refuses what every later call would refuse
        self.k, self.ratio = k, ratio
        self._error: dict[str, torch.Tensor] = {}

    def error(self, name: str) -> torch.Tensor | None:
        """The residual kept for ``name``, or ``None`` before its first round."""
        return self._error.get(name)

    def reset(self) -> None:
        self._error.clear()

    def sparsify(self, message: Any) -> Any:
        """A new message of the class of ``message`` (a ``DeltaParameterMessage``) whose floating
        tensors travel as ``SparseDelta``; every other field is copied, every other value of
        ``delta_parameter`` (an integer tensor, a value that is sparse already) passes unchanged.
        Keeps the new residuals. ``ValueError`` for a name whose shape or dtype changed."""
        dense = {n: v for n, v in message.delta_parameter.items()
                 if isinstance(v, torch.Tensor) and v.dtype in VALUE_DTYPES}
        for name, value in dense.items():
            e = self._error.get(name)
            if e is not None and (e.shape != value.shape or e.dtype != value.dtype):
                raise ValueError(f"{name}: {tuple(value.shape)} {value.dtype} now, {tuple(e.shape)} {e.dtype} in the "
                                 "round before: reset() the residuals of a changed model")
            if e is not None and e.device != value.device:
                self._error[name] = e.to(value.device)
        sent, residual = topk_sparsify_parameter(dense, self.k, self.ratio, self._error)
        self._error.update(residual)
        return dataclasses.replace(
            message, delta_parameter={n: sent.get(n, v) for n, v in message.delta_parameter.items()})


class TopKSparseEndpoint:
    """Wraps a client endpoint (any object with ``send(data)``): a ``DeltaParameterMessage`` goes out
    sparsified by the endpoint's ``TopKErrorFeedback``, everything else unchanged (a full
    ``ParameterMessage`` is no diff: the reference's worker asserts ``_send_parameter_diff``). Every
    other attribute is the wrapped endpoint's. Keyword arguments ``k`` or ``ratio`` (neither: a
    ratio of 0.01). Without an ``endpoint`` the remaining keyword arguments build the simulator's
    ``ClientEndpoint``, which is how ``AlgorithmRepository.create_client`` constructs it."""

    def __init__(self, endpoint: Any = None, **kwargs: Any) -> None:
        k: int | None = kwargs.pop("k", None)
        ratio: float | None = kwargs.pop("ratio", None)
        if k is None and ratio is None:
            ratio = 0.01
        if endpoint is None:
            from cyy_naive_lib.topology.cs_endpoint import ClientEndpoint  # the simulator's, not vendored

            endpoint = ClientEndpoint(**kwargs)
        elif kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if not callable(getattr(endpoint, "send", None)):
            raise TypeError("the wrapped endpoint needs a send(data) method")
        self._endpoint = endpoint
        self.feedback = TopKErrorFeedback(k=k, ratio=ratio)

    def __getattr__(self, name: str) -> Any:  # only what this object does not have itself
        endpoint = self.__dict__.get("_endpoint")
        if endpoint is None:
            raise AttributeError(name)
        return getattr(endpoint, name)

    def send(self, data: Any) -> None:
        self._endpoint.send(self.feedback.sparsify(data) if is_delta_message(data) else data)
