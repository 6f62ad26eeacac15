"""Host-side handle on the HIP FedAvg library: model layouts, client tables, error mapping.

A ``ModelLayout`` is the ordered list of named tensors of a model — the keys of
``ParameterMessage.parameter`` (reference ``simulation_lib/message.py:24-31``). A
``FedAvgContext`` owns one native context (``include/fedavg_hip.h``) for one layout on one
device: the fp64 accumulator the streaming path folds clients into
(``fed_avg_algorithm.py:43-64``), the per-segment total weights, and the fused
finalize/NaN checks (``fed_avg_algorithm.py:76-99``).

Every method launches asynchronously on the current torch stream of the context's device
(``torch.cuda.current_stream``); PyTorch is only the allocator and stream provider here. The
device arithmetic runs in the HIP kernels of ``csrc/``; a missing kernel is an error, never a quiet
CPU fall-back. The host arithmetic that the side rules do between two kernel calls (and that the
algorithms' own CPU paths share) lives in ``rules.py`` and is re-exported here.

The side-kernel wrappers of ``FedAvgContext`` (``robust_aggregate`` to ``server_opt_step``) refuse
every operand a kernel would read or write out of bounds before anything is launched; the checks
they share are the private helpers above them.
"""

from __future__ import annotations

import ctypes
import math
import weakref
from collections.abc import Mapping, Sequence
from dataclasses import dataclass
from functools import cached_property
from typing import Any

import numpy as np
import torch

from . import _native
from .rules import (  # noqa: F401 - re-exported: ``from ...fedavg import krum_select`` keeps working
    ROBUST_MODES, SERVER_OPT_MODES, _sqrt_rn, bulyan_select, check_robust_rule, check_server_opt,
    clipping_coefficients, geometric_median_step, krum_select, robust_trim, server_opt_update, trust_coefficients,
)
from .sparse import SparseDelta

DTYPE_CODES: dict[torch.dtype, int] = {
    torch.float32: _native.F32,
    torch.float16: _native.F16,
    torch.bfloat16: _native.BF16,
    torch.float64: _native.F64,
}
OUT_CODES: dict[torch.dtype, int] = {torch.float32: _native.F32, torch.float64: _native.F64}

_PTR = ctypes.POINTER(ctypes.c_void_p)
_DBL = ctypes.POINTER(ctypes.c_double)


class NaNAggregationError(AssertionError):
    """Raised where the reference's NaN assertions fire (fed_avg_algorithm.py:35,93,97).

    Subclasses ``AssertionError`` so callers that expect the reference's ``assert`` keep
    working. ``stage`` is ``"input"`` (:35), ``"accumulator"`` (:93) or ``"result"`` (:97).
    """

    def __init__(self, stage: str, message: str, bad_clients: Sequence[int] = ()) -> None:
        super().__init__(message)
        self.stage = stage
        self.bad_clients = list(bad_clients)


@dataclass(frozen=True)
class ModelLayout:
    """Names, shapes and element counts of a model's tensors, in dict order."""

    names: tuple[str, ...]
    shapes: tuple[tuple[int, ...], ...]

    @classmethod
    def from_parameters(cls, parameter: Mapping[str, torch.Tensor]) -> ModelLayout:
        return cls(
            names=tuple(parameter.keys()),
            shapes=tuple(tuple(t.shape) for t in parameter.values()),
        )

    @classmethod
    def flat(cls, numel: int, name: str = "bucket") -> ModelLayout:
        return cls(names=(name,), shapes=((int(numel),),))

    @cached_property
    def numels(self) -> list[int]:
        # cached: the staging path asks for it per client (np.prod per tensor is ~2 us)
        return [int(np.prod(s, dtype=np.int64)) for s in self.shapes]

    @property
    def num_segments(self) -> int:
        return len(self.names)

    @property
    def total_numel(self) -> int:
        return sum(self.numels)

    def padded_offsets(self, elem_bytes: int) -> tuple[list[int], int]:
        """Element offsets of each tensor in a flat buffer whose segments start 16-B aligned."""
        cache = self.__dict__.setdefault("_padded_cache", {})
        if elem_bytes not in cache:
            cache[elem_bytes] = self._padded_offsets(elem_bytes)
        offs, total = cache[elem_bytes]
        return list(offs), total

    def _padded_offsets(self, elem_bytes: int) -> tuple[list[int], int]:
        align = max(1, 16 // elem_bytes)
        offs, pos = [], 0
        for n in self.numels:
            offs.append(pos)
            pos += (n + align - 1) // align * align
        return offs, pos


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_EMPTY_ARRAYS = (np.zeros(1, np.uint64), np.zeros(1, np.float64))  # module-lifetime storage
_EMPTY_TABLE = (_EMPTY_ARRAYS[0].ctypes.data, _EMPTY_ARRAYS[1].ctypes.data)


def _table_args(table: ClientTable) -> tuple[Any, Any]:
    """The client table's pointer and weight arrays as C-ABI arguments: the staging extension's
    raw addresses when the table has them, else ctypes pointers that keep its numpy arrays alive
    for the call."""
    addresses = getattr(table, "addresses", None)
    if addresses is not None:
        return addresses()
    p, w = table.arrays()
    return p.ctypes.data_as(_PTR), w.ctypes.data_as(_DBL)


def _stream_handle(device: torch.device) -> ctypes.c_void_p:
    """torch's current stream on ``device`` (the raw handle without building a Stream object:
    this runs on every launch)."""
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dtype) -> int:
    """C-ABI input format of a torch dtype, or of a quantised record format
    (``quantized.QSGD_F32`` / ``QSGD_F64`` / ``NNADQ_F32`` / ``NNADQ_F64``, which carry their
    own code)."""
    if not isinstance(dtype, torch.dtype):
        code = getattr(dtype, "code", None)
        if code in _native.RECORD_CODES:
            return int(code)
        raise TypeError(f"no HIP FedAvg kernel for input format {dtype}")
    try:
        return DTYPE_CODES[dtype]
    except KeyError:
        raise TypeError(f"no HIP FedAvg kernel for input dtype {dtype}") from None


def out_code(dtype: torch.dtype) -> int:
    try:
        return OUT_CODES[dtype]
    except KeyError:
        raise TypeError(f"aggregated output dtype must be float32 or float64, not {dtype}") from None


def robust_trim_counts(table: ClientTable, mode: str, trim: float) -> list[int]:
    """Per segment k for the table's clients, after the refusals that need no device."""
    check_robust_rule(mode, trim)
    if table.num_clients == 0:
        raise ValueError("robust aggregation of no clients")
    T = table.num_segments
    sent = (np.asarray(table.arrays()[0]).reshape(table.num_clients, T) != 0).sum(axis=0)
    ks = []
    for t, n in enumerate(int(x) for x in sent):
        if n > _native.ROBUST_MAX_CLIENTS:
            raise NotImplementedError(
                f"tensor {t} was sent by {n} clients: the register-resident sort holds at most "
                f"{_native.ROBUST_MAX_CLIENTS} values per element")
        if n == 0:
            raise ValueError(f"tensor {t} was sent by no client")
        ks.append(robust_trim(mode, trim, n))
    return ks


class ClientTable:
    """Row-major [num_clients][num_segments] device pointers + fp64 weights for one call.

    ``None`` entries are absent tensors (skipped, never counted in the segment's total
    weight). The tensors are kept alive by the table until the caller drops it.
    """

    def __init__(self, num_segments: int) -> None:
        self.num_segments = num_segments
        self._ptrs: list[int] = []
        self._weights: list[float] = []
        self._keep: list[torch.Tensor] = []
        # per entry: element count, element size, device (-1 = host) — checked against the
        # layout and input format before any launch (an undersized operand would be read out
        # of bounds by the kernel); -1 / 0 / -2 for absent entries
        self._numel: list[int] = []
        self._esize: list[int] = []
        self._dev: list[int] = []
        self._validated: set = set()
        self.num_clients = 0
        self._arrays: tuple[np.ndarray, np.ndarray] | None = None
        # per-element weights (fedavg_accumulate_elementwise): pointer + dtype code per entry
        self._wptrs: list[int] = []
        self._wdts: list[int] = []

    def add_client(self, tensors: Sequence[torch.Tensor | None], weights: Sequence[float],
                   weight_tensors: Sequence[torch.Tensor | None] | None = None) -> None:
        """One client row. ``weight_tensors`` (optional): per-element weight tensors (fp32 / fp64,
        the segment's size) where a _get_weight override returned one; None = the scalar."""
        T = self.num_segments
        if len(tensors) != T or len(weights) != T:
            raise ValueError("client row does not match the layout")
        if weight_tensors is not None and len(weight_tensors) != T:
            raise ValueError("weight row does not match the layout")
        # the row is built in locals and committed at the end: a rejected row leaves the table as
        # it was (this runs once per client on the plugin path, so it is kept lean)
        ptrs, ws, numel, esize, dev, keep = [], [], [], [], [], []
        for t, w in zip(tensors, weights):
            if t is None:
                ptrs.append(0)
                ws.append(0.0)
                numel.append(-1)
                esize.append(0)
                dev.append(-2)
            else:
                if not t.is_contiguous():
                    raise ValueError("client tensors must be contiguous (the kernel reads them as flat buffers)")
                ptrs.append(t.data_ptr())
                ws.append(float(w))
                numel.append(t.numel())
                esize.append(t.element_size())
                dev.append(t.get_device())  # -1 for host tensors
                keep.append(t)
        wptrs, wdts = [0] * T, [_native.F64] * T
        if weight_tensors is not None:
            for i, (t, wt) in enumerate(zip(tensors, weight_tensors)):
                if t is None or wt is None:
                    continue
                if wt.dtype not in (torch.float32, torch.float64) or not wt.is_contiguous() \
                        or wt.numel() != t.numel() or wt.device != t.device:
                    raise ValueError("per-element weights: contiguous fp32 / fp64 of the tensor's size and device")
                wptrs[i] = wt.data_ptr()
                wdts[i] = _native.F32 if wt.dtype == torch.float32 else _native.F64
                keep.append(wt)
        self._ptrs += ptrs
        self._weights += ws
        self._numel += numel
        self._esize += esize
        self._dev += dev
        self._wptrs += wptrs
        self._wdts += wdts
        self._keep += keep
        self._validated.clear()
        self.num_clients += 1
        self._arrays = None

    def add_resident_client(self, ptrs: list[int], weights: list[float], numels: list[int], esize: int,
                            device_index: int, keep: list[torch.Tensor]) -> None:
        """One client row whose present tensors the caller has already checked: contiguous, on
        ``device_index``, ``esize``-byte elements, ``numels[seg]`` elements each (``ptrs[seg]``
        == 0 and ``numels[seg]`` == -1 for an absent tensor). The plugin's staging pass proves
        all of that while it recognises the common arrival, so the row is committed without
        touching the tensors again; ``validate`` still checks the recorded sizes before a launch."""
        T = self.num_segments
        if len(ptrs) != T or len(weights) != T or len(numels) != T:
            raise ValueError("client row does not match the layout")
        self._ptrs += ptrs
        self._weights += weights
        self._numel += numels
        self._esize += [esize if n >= 0 else 0 for n in numels]
        self._dev += [device_index if n >= 0 else -2 for n in numels]
        self._wptrs += [0] * T
        self._wdts += [_native.F64] * T
        self._keep += keep
        self._validated.clear()
        self.num_clients += 1
        self._arrays = None

    def elementwise_arrays(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Weight pointers and dtype codes, [num_clients][num_segments] (0 = scalar weight)."""
        return (np.asarray(self._wptrs or [0], dtype=np.uint64), np.asarray(self._wdts or [0], dtype=np.int32),
                np.asarray(self._weights or [0.0], dtype=np.float64))

    def validate(self, numels: Sequence[int], esize: int, device_index: int, key) -> None:
        """Every present entry holds exactly ``numels[seg]`` elements of ``esize`` bytes on the
        device (checked once per table and ``key``). Raises ValueError naming the first bad one."""
        if key in self._validated or self.num_clients == 0:
            return
        T = self.num_segments
        have = np.asarray(self._numel, dtype=np.int64).reshape(self.num_clients, T)
        es = np.asarray(self._esize, dtype=np.int64).reshape(self.num_clients, T)
        dev = np.asarray(self._dev, dtype=np.int64).reshape(self.num_clients, T)
        want = np.broadcast_to(np.asarray(numels, dtype=np.int64), have.shape)
        present = have >= 0
        bad = present & ((have != want) | (es != esize) | (dev != device_index))
        if bad.any():
            k, t = (int(x) for x in np.argwhere(bad)[0])
            raise ValueError(
                f"client {k}, tensor {t}: {have[k, t]} elements of {es[k, t]} bytes on device {dev[k, t]}; "
                f"the layout and input format need {want[k, t]} of {esize} bytes on device {device_index}")
        self._validated.add(key)

    def arrays(self) -> tuple[np.ndarray, np.ndarray]:
        """The C-ABI arrays (built once per table and cached: a table can be reduced many times)."""
        if self._arrays is None:
            ptrs = np.asarray(self._ptrs, dtype=np.uint64) if self._ptrs else np.zeros(1, np.uint64)
            ws = np.asarray(self._weights, dtype=np.float64) if self._weights else np.zeros(1, np.float64)
            self._arrays = (ptrs, ws)
        return self._arrays

    def set_weights(self, weights: Sequence[float]) -> None:
        """Replace the weights in place, one per client (every present tensor of client k gets
        ``weights[k]``; absent entries keep 0.0). The pointers are not restaged: the arrays of
        ``arrays()`` stay where they are, so a table folded many times with new weights (the
        geometric median's iterations) is built once."""
        if len(weights) != self.num_clients:
            raise ValueError("one weight per client is required")
        T = self.num_segments
        p, w = self.arrays()
        n = self.num_clients * T
        if n:
            w[:n] = np.where(p[:n] != 0, np.repeat(np.asarray(weights, dtype=np.float64), T), 0.0)
            self._weights = w[:n].tolist()

    def rows(self) -> list[list[int]]:
        T = self.num_segments
        return [self._ptrs[k * T : (k + 1) * T] for k in range(self.num_clients)]


class OutputTable:
    """Validated per-segment output tensors of one dtype (built once, reusable across calls)."""

    def __init__(self, outs: Sequence[torch.Tensor], layout: ModelLayout, device: torch.device,
                 dtype: torch.dtype) -> None:
        if len(outs) != layout.num_segments:
            raise ValueError("one output tensor per segment is required")
        for o, n in zip(outs, layout.numels):
            if o.dtype != dtype or o.device != device or o.numel() != n or not o.is_contiguous():
                raise ValueError("output tensors must be contiguous, on the context device, of the layout size")
        self.tensors = list(outs)
        self.dtype = dtype
        self.layout = layout
        self.device = device
        self.c_array = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])

    @classmethod
    def from_flat(cls, flat: torch.Tensor, offsets: Sequence[int], layout: ModelLayout) -> OutputTable:
        """Segments of one flat contiguous buffer at element ``offsets`` (no tensor per segment:
        the pointer array is computed from the buffer's address)."""
        if flat.dim() != 1 or not flat.is_contiguous() or len(offsets) != layout.num_segments:
            raise ValueError("a flat contiguous buffer and one offset per segment are required")
        offs = np.asarray(offsets, dtype=np.int64)
        if layout.num_segments and (offs.min() < 0 or int((offs + np.asarray(layout.numels)).max()) > flat.numel()):
            raise ValueError("segment outside the flat output buffer")
        self = cls.__new__(cls)
        self.tensors = [flat]
        self.dtype = flat.dtype
        self.layout = layout
        self.device = flat.device
        ptrs = np.uint64(flat.data_ptr()) + offs.astype(np.uint64) * np.uint64(flat.element_size())
        self.c_array = (ctypes.c_void_p * layout.num_segments).from_buffer_copy(ptrs.tobytes())
        return self


SPARSE_INDEX_MESSAGE = ("a sparse delta's indices are not strictly increasing inside [0, numel): "
                        "duplicate, descending, negative or past the tensor's end")


class SparseTable:
    """Validated rows of sparse deltas as the C-ABI arrays of ``fedavg_sparse_aggregate_delta``:
    ``rows[i][t]`` is client ``i``'s ``SparseDelta`` of segment ``t`` of ``layout`` on ``device``, all
    of one value dtype (built once, reusable across calls; it keeps the tensors alive)."""

    def __init__(self, rows: Sequence[Sequence[SparseDelta]], layout: ModelLayout, device: torch.device) -> None:
        n, T = len(rows), layout.num_segments
        if n == 0:
            raise ValueError("the sparse fold of no clients")
        if n > _native.POINT_MAX_CLIENTS:
            raise NotImplementedError(f"{n} clients: the sparse fold takes at most {_native.POINT_MAX_CLIENTS}")
        dtypes = set()
        self.iptr = np.zeros(n * T, dtype=np.uint64)
        self.vptr = np.zeros(n * T, dtype=np.uint64)
        self.nnz = np.zeros(n * T, dtype=np.int64)
        for i, row in enumerate(rows):
            if len(row) != T:
                raise ValueError(f"client {i}: one sparse delta per segment is required")
            for t, (d, numel) in enumerate(zip(row, layout.numels)):
                if not isinstance(d, SparseDelta):
                    raise TypeError(f"client {i}, tensor {t}: a SparseDelta is required, not {type(d).__name__}")
                if d.numel != numel or d.indices.device != device or d.values.device != device \
                        or not d.indices.is_contiguous() or not d.values.is_contiguous():
                    raise ValueError(f"client {i}, tensor {t}: a contiguous sparse delta of {numel} elements on "
                                     f"{device} is required")
                dtypes.add(d.values.dtype)
                k = i * T + t
                self.nnz[k] = d.nnz
                if d.nnz:
                    self.iptr[k] = d.indices.data_ptr()
                    self.vptr[k] = d.values.data_ptr()
        if len(dtypes) != 1:
            raise ValueError(f"the sparse deltas of one call share one value dtype, not {sorted(map(str, dtypes))}")
        self.dtype = dtypes.pop()
        self.num_clients = n
        self.layout = layout
        self.device = device
        self._keep = [list(row) for row in rows]


NOT_IN_PLACE = "the step is not in-place, ping-pong two buffers"


def _pointer_array(tensors: Sequence[torch.Tensor]) -> ctypes.Array:
    return (ctypes.c_void_p * len(tensors))(*[z.data_ptr() for z in tensors])


def _first(T: int, *faults: int) -> tuple[int, int]:
    """Which refusal a call over T tensors reports. Each of ``faults`` is the first tensor at which
    one kind of fault holds (T: nowhere), the kinds in the order in which one tensor is checked.
    Returns ``(t, kind)`` of the first fault in tensor order, ``(T, -1)`` if there is none."""
    t = min(faults)
    return (t, faults.index(t)) if t < T else (T, -1)


def _first_shared(a: Sequence[torch.Tensor], b: Sequence[torch.Tensor]) -> int:
    """The first index at which ``a`` and ``b`` hold the same storage address; ``len(a)`` if none."""
    return next((t for t, (x, y) in enumerate(zip(a, b)) if x.data_ptr() == y.data_ptr()), len(a))


def _addresses(tensors: Sequence[torch.Tensor | None], counts: Sequence[int]) -> np.ndarray:
    """The C-ABI address table of a layout-free call: 0 for an absent or an empty (``counts[t] == 0``) tensor."""
    return np.array([z.data_ptr() if z is not None and n else 0 for z, n in zip(tensors, counts)], dtype=np.uint64)


def _client_scalars(values: Sequence[float], n: int, what: str) -> np.ndarray:
    """One finite fp64 ``what`` ("coefficient", "weight") per client, as the C-ABI array."""
    v = np.ascontiguousarray([float(x) for x in values], dtype=np.float64)
    if v.shape != (n,):
        raise ValueError(f"one {what} per client is required: {v.size} for {n} clients")
    if not np.isfinite(v).all():
        raise ValueError(f"the {what}s must be finite")
    return v


def _divisor(divisor: float) -> float:
    divisor = float(divisor)
    if not (divisor > 0 and math.isfinite(divisor)):
        raise ValueError(f"the divisor must be a finite number > 0, not {divisor}")
    return divisor


def _stream_ids(seed: int, draw: int, tensor_ids: Sequence[int] | None, T: int) -> np.ndarray:
    """The random stream's words of a call over T tensors: the seed and the draw in range, then one
    uint32 id per tensor (default: its position)."""
    if not 0 <= int(seed) < 1 << 64 or not 0 <= int(draw) < 1 << 32:
        raise ValueError("the seed is a uint64 and the draw a uint32")
    ids = np.arange(T, dtype=np.uint32) if tensor_ids is None else np.ascontiguousarray(tensor_ids, dtype=np.uint32)
    if ids.shape != (T,):
        raise ValueError("one stream id per tensor is required")
    return ids


class FedAvgContext:
    """One native FedAvg context: layout + device + fp64 accumulator."""

    def __init__(
        self,
        layout: ModelLayout,
        device: torch.device | str | int | None = None,
        split_policy: int | None = None,
        lib: ctypes.CDLL | None = None,
    ) -> None:
        self._lib = lib if lib is not None else _native.load()
        self._plans: weakref.WeakSet[AggregatePlan] = weakref.WeakSet()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("the FedAvg HIP path runs on a GPU device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.layout = layout
        if layout.num_segments == 0 or min(layout.numels) <= 0:
            raise ValueError("a native layout needs at least one tensor and no empty tensors")
        numels = (ctypes.c_int64 * layout.num_segments)(*layout.numels)
        # the accumulator is a torch tensor so collectives (RCCL) can run on it
        acc_numel = self._padded_acc_numel(layout, self._lib)
        self.accumulator = torch.zeros(acc_numel, dtype=torch.float64, device=device)
        handle = ctypes.c_void_p()
        _native.check(
            self._lib.fedavg_ctx_create(
                ctypes.byref(handle),
                device.index,
                numels,
                layout.num_segments,
                ctypes.c_void_p(self.accumulator.data_ptr()),
            )
        )
        self._h = handle
        assert self._lib.fedavg_acc_numel(self._h) == acc_numel
        if split_policy is not None:
            _native.check(self._lib.fedavg_set_split_policy(self._h, split_policy))

    @classmethod
    def borrowed(cls, lib: ctypes.CDLL, handle: int, layout: ModelLayout, device: torch.device,
                 accumulator: torch.Tensor) -> FedAvgContext:
        """A view of a native context owned by another object (a device entry of
        ``multi_device.MultiDeviceContext``): same methods, but ``close`` leaves it alone."""
        self = cls.__new__(cls)
        self._lib = lib
        self._plans = weakref.WeakSet()
        self.device = device
        self.layout = layout
        self.accumulator = accumulator
        self._h = ctypes.c_void_p(handle)
        self._borrowed = True
        return self

    @staticmethod
    def _padded_acc_numel(layout: ModelLayout, lib: ctypes.CDLL) -> int:
        """Accumulator elements: every segment starts at a multiple of FEDAVG_ACC_ALIGN (32)."""
        numels = (ctypes.c_int64 * layout.num_segments)(*layout.numels)
        n = int(lib.fedavg_layout_acc_numel(numels, layout.num_segments))
        if n < 0:
            raise ValueError("bad layout")
        return n

    @property
    def acc_numel(self) -> int:
        return self.accumulator.numel()

    # -- lifecycle -------------------------------------------------------------------
    def close(self) -> None:
        for plan in list(getattr(self, "_plans", ())):
            plan.close()  # before the native context goes: a plan reads it
        if getattr(self, "_borrowed", False):
            self._h = ctypes.c_void_p()  # the owner destroys it
            return
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.fedavg_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------
    @property
    def stream(self) -> ctypes.c_void_p:
        return _stream_handle(self.device)

    def segment_offset(self, seg: int) -> int:
        return int(self._lib.fedavg_segment_offset(self._h, seg))

    @property
    def num_tiles(self) -> int:
        return int(self._lib.fedavg_num_tiles(self._h))

    def tile_range(self, tile_begin: int, tile_end: int) -> tuple[int, int]:
        b, e = ctypes.c_int64(), ctypes.c_int64()
        _native.check(self._lib.fedavg_tile_range(self._h, tile_begin, tile_end, ctypes.byref(b), ctypes.byref(e)))
        return b.value, e.value

    def total_weights(self) -> list[float]:
        out = (ctypes.c_double * self.layout.num_segments)()
        _native.check(self._lib.fedavg_total_weights(self._h, out))
        return list(out)

    def _out_table(self, outs: Sequence[torch.Tensor] | OutputTable, out_dtype: torch.dtype) -> ctypes.Array:
        if isinstance(outs, OutputTable):
            if outs.dtype != out_dtype or outs.layout != self.layout or outs.device != self.device:
                raise ValueError("output table was built for another dtype, layout or device")
            return outs.c_array
        return OutputTable(outs, self.layout, self.device, out_dtype).c_array

    def _check_table(self, table: ClientTable, in_dtype: torch.dtype) -> None:
        if table.num_segments != self.layout.num_segments:
            raise ValueError("client table does not match the layout")
        code = dtype_code(in_dtype)
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if code in _native.RECORD_CODES:
            # one uint8 record per tensor (include/fedavg_hip.h record layouts)
            nbytes = (self._lib.fedavg_qsgd_record_bytes if code in (_native.QSGD_F32, _native.QSGD_F64)
                      else self._lib.fedavg_nnadq_record_bytes)
            need = [int(nbytes(n)) for n in self.layout.numels]
            table.validate(need, 1, dev, ("record", tuple(need), dev))
        else:
            # the key is built once per (dtype, device): this runs per wave launch
            keys = self.__dict__.setdefault("_dense_keys", {})
            key = keys.get((in_dtype, dev))
            if key is None:
                key = keys[(in_dtype, dev)] = (in_dtype, tuple(self.layout.numels), dev)
            table.validate(self.layout.numels, in_dtype.itemsize, dev, key)

    # -- hot path --------------------------------------------------------------------
    def accumulate(self, table: ClientTable, in_dtype: torch.dtype) -> None:
        """Fold a wave of clients into the accumulator (fed_avg_algorithm.py:43-64)."""
        self._check_table(table, in_dtype)
        if table.num_clients == 0:
            return
        p, w = _table_args(table)
        _native.check(
            self._lib.fedavg_accumulate(self._h, p, dtype_code(in_dtype), w, table.num_clients, self.stream)
        )

    def aggregate(
        self,
        table: ClientTable | None,
        in_dtype: torch.dtype,
        outs: Sequence[torch.Tensor] | OutputTable,
        out_dtype: torch.dtype,
    ) -> None:
        """Fold the last wave (optional) then out = acc / total_weight (fed_avg_algorithm.py:76-99)."""
        n = 0 if table is None else table.num_clients
        if table is not None:
            self._check_table(table, in_dtype)
            p, w = _table_args(table)
        else:
            p, w = _EMPTY_TABLE
        ot = self._out_table(outs, out_dtype)
        _native.check(
            self._lib.fedavg_aggregate(
                self._h, p, dtype_code(in_dtype) if n else _native.F32, w, n, ot, out_code(out_dtype), self.stream,
            )
        )

    def _base_table(self, base: Sequence[torch.Tensor] | OutputTable) -> ctypes.Array:
        return self._out_table(base, torch.float64)

    def accumulate_delta(self, table: ClientTable, in_dtype: torch.dtype,
                         base: Sequence[torch.Tensor] | OutputTable) -> None:
        """Fold a wave of DELTA clients: x = base + delta (fp64), message.py:40-61 fused."""
        self._check_table(table, in_dtype)
        if table.num_clients == 0:
            return
        p, w = table.arrays()
        bt = self._base_table(base)
        _native.check(
            self._lib.fedavg_accumulate_delta(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), w.ctypes.data_as(_DBL),
                table.num_clients, bt, self.stream,
            )
        )

    def aggregate_delta(self, table: ClientTable, in_dtype: torch.dtype,
                        base: Sequence[torch.Tensor] | OutputTable,
                        outs: Sequence[torch.Tensor] | OutputTable, out_dtype: torch.dtype) -> None:
        """Last wave of delta clients + divide (fedavg_aggregate with the restore fused)."""
        self._check_table(table, in_dtype)
        p, w = table.arrays()
        bt = self._base_table(base)
        ot = self._out_table(outs, out_dtype)
        _native.check(
            self._lib.fedavg_aggregate_delta(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), w.ctypes.data_as(_DBL),
                table.num_clients, bt, ot, out_code(out_dtype), self.stream,
            )
        )

    def weighted_avg(
        self, table: ClientTable, in_dtype: torch.dtype, outs: Sequence[torch.Tensor], out_dtype: torch.dtype
    ) -> None:
        """out = sum_k ratio_k * x_k in fp64, table weights are the ratios (aggregation_algorithm.py:51-76)."""
        self._check_table(table, in_dtype)
        p, w = table.arrays()
        ot = self._out_table(outs, out_dtype)
        _native.check(
            self._lib.fedavg_weighted_avg(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), w.ctypes.data_as(_DBL),
                table.num_clients, ot, out_code(out_dtype), self.stream,
            )
        )

    # -- what the side wrappers refuse, each check once ----------------------------
    # These refusals are all that keeps an undersized or misplaced operand from a kernel that would
    # read or write it out of bounds. ``what`` is the call's noun phrase, ``s`` its verb ending.
    def _refuse_records(self, in_dtype: torch.dtype, what: str, s: str) -> None:
        if dtype_code(in_dtype) in _native.RECORD_CODES:
            raise NotImplementedError(f"{what} read{s} dense tensors: dequantise records first")

    def _refuse_before_table(self, table: ClientTable, in_dtype: torch.dtype, what: str, s: str, limit: int) -> None:
        """A whole-update call's refusals that come before the table check: an empty table, more
        than ``limit`` clients, quantised records."""
        if table.num_clients == 0:
            raise ValueError(f"{what} of no clients")
        if table.num_clients > limit:
            raise NotImplementedError(f"{table.num_clients} clients: {what} take{s} at most {limit}")
        self._refuse_records(in_dtype, what, s)

    def _whole_updates(self, table: ClientTable, in_dtype: torch.dtype, whole: str) -> np.ndarray:
        """The table check, then the first absent entry refused (the call ``whole``, as in
        "distances compare", whole updates). Returns the table's pointer array."""
        self._check_table(table, in_dtype)
        n, T = table.num_clients, table.num_segments
        p, _ = table.arrays()
        absent = np.argwhere(np.asarray(p)[: n * T].reshape(n, T) == 0)
        if len(absent):
            k, t = (int(x) for x in absent[0])
            raise ValueError(f"client {k} lacks tensor {t}: {whole} whole updates")
        return p

    def _first_unfit(self, tensors: Sequence[torch.Tensor | None], dtype: torch.dtype,
                     sizes: Sequence[int] | None = None) -> int:
        """The index of the first of ``tensors`` that is not a contiguous ``dtype`` tensor (of
        ``sizes[t]`` elements) on the context's device; ``len(tensors)`` if every one is. ``None``
        entries are skipped. One loop per group and no call per tensor: a model has tens of tensors."""
        device = self.device
        if sizes is None:
            for t, z in enumerate(tensors):
                if z.dtype != dtype or z.device != device or not z.is_contiguous():
                    return t
        else:
            for t, (z, size) in enumerate(zip(tensors, sizes)):
                if z is not None and (z.dtype != dtype or z.device != device or z.numel() != size
                                      or not z.is_contiguous()):
                    return t
        return len(tensors)

    def _segment_refusal(self, what: str, t: int, dtype: torch.dtype | None = None) -> ValueError:
        """For a per-segment group's tensor ``t``: fp64, or the outputs' ``dtype``."""
        return ValueError(f"{what} tensor {t}: contiguous {dtype or 'fp64'} of {self.layout.numels[t]} elements on "
                          f"{self.device} is required")

    def _flat_refusal(self, what: str, t: int, dtype: torch.dtype, numel: int | None = None) -> ValueError:
        """For a layout-free call's operand ``t``."""
        size = "" if numel is None else f" of {numel} elements"
        return ValueError(f"{what} {t}: a contiguous {dtype} tensor{size} on {self.device} is required")

    def _record_refusal(self, t: int, need: int) -> ValueError:
        return ValueError(f"record {t}: a contiguous uint8 tensor of {need} bytes on {self.device} is required")

    def _segment_array(self, what: str, tensors: Sequence[torch.Tensor]) -> ctypes.Array:
        """The pointer array of one contiguous fp64 tensor per segment on the context's device."""
        T = self.layout.num_segments
        if len(tensors) != T:
            raise ValueError(f"one {what} tensor per segment is required")
        t = self._first_unfit(tensors, torch.float64, self.layout.numels)
        if t < T:
            raise self._segment_refusal(what, t)
        return _pointer_array(tensors)

    def _source_and_outputs(self, what: str, src: Sequence[torch.Tensor], outs: Sequence[torch.Tensor],
                            out_dtype: torch.dtype, why: str) -> tuple[ctypes.Array, ctypes.Array]:
        """The pointer arrays of the fp64 ``what`` ("point", "base") tensors and of the outputs: one
        contiguous ``out_dtype`` tensor per segment, none of them its source's own storage."""
        T, numels = self.layout.num_segments, self.layout.numels
        if len(src) != T or len(outs) != T:
            raise ValueError(f"one {what} tensor and one output tensor per segment are required")
        zs, os_ = [z.data_ptr() for z in src], [o.data_ptr() for o in outs]
        t, fault = _first(T, self._first_unfit(src, torch.float64, numels), self._first_unfit(outs, out_dtype, numels),
                          next((t for t in range(T) if zs[t] == os_[t]), T))
        if fault == 0:
            raise self._segment_refusal(what, t)
        if fault == 1:
            raise self._segment_refusal("output", t, out_dtype)
        if fault == 2:
            raise ValueError(f"output tensor {t} is its {what}: {why}")
        return (ctypes.c_void_p * T)(*zs), (ctypes.c_void_p * T)(*os_)

    # -- the side kernels --------------------------------------------------------------------------
    def robust_aggregate(
        self,
        table: ClientTable,
        in_dtype: torch.dtype,
        mode: str,
        trim: float,
        outs: Sequence[torch.Tensor] | OutputTable,
        out_dtype: torch.dtype = torch.float64,
    ) -> None:
        """Coordinate-wise trimmed mean (``mode="trimmed_mean"``, 0 <= trim < 0.5) or median
        (``mode="median"``) of the table's clients, one launch (``fedavg_robust_aggregate``; not a
        reference algorithm, DESIGN.md "Robust rules"). Per tensor the n clients that sent it count,
        k = floor(trim * n) values are dropped at each end; the table's weights are ignored — both
        rules are unweighted. Refused before any launch: ``trim`` outside [0, 0.5), a tensor sent
        by more than 64 clients, quantised records."""
        k_per_seg = robust_trim_counts(table, mode, trim)
        self._refuse_records(in_dtype, "robust aggregation", "s")
        self._check_table(table, in_dtype)
        p, _ = table.arrays()
        ot = self._out_table(outs, out_dtype)
        ks = (ctypes.c_int32 * self.layout.num_segments)(*k_per_seg)
        _native.check(
            self._lib.fedavg_robust_aggregate(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), table.num_clients,
                _native.ROBUST_MEDIAN if mode == "median" else _native.ROBUST_TRIMMED_MEAN, ks, ot,
                out_code(out_dtype), self.stream,
            )
        )

    def mean_around_median(
        self,
        table: ClientTable,
        in_dtype: torch.dtype,
        keep: int | Sequence[int],
        outs: Sequence[torch.Tensor] | OutputTable,
        out_dtype: torch.dtype = torch.float64,
    ) -> None:
        """Per element the mean of the ``keep`` sorted values closest to the lower median of the
        table's clients, one launch (``fedavg_mean_around_median``; not a reference algorithm,
        DESIGN.md §5k): the coordinate step of Bulyan. ``keep`` is one int for every tensor or one
        per tensor, ``1 <= keep <= n`` with n the clients that sent the tensor; ``keep == n`` is the
        sorted-order mean, ``keep == 1`` the lower median. The table's weights are ignored and the
        accumulator is not touched. Refused before any launch: ``keep`` out of range, a tensor sent
        by more than 64 clients, quantised records."""
        T = table.num_segments
        keeps = [int(keep)] * T if isinstance(keep, (int, np.integer)) else [int(k) for k in keep]
        if len(keeps) != T:
            raise ValueError(f"keep has {len(keeps)} entries for {T} tensors")
        robust_trim_counts(table, "median", 0.0)  # the refusals that need no device: 0 or > 64 senders
        sent = (np.asarray(table.arrays()[0]).reshape(table.num_clients, T) != 0).sum(axis=0)
        for t, (k, n) in enumerate(zip(keeps, (int(x) for x in sent))):
            if not 1 <= k <= n:
                raise ValueError(f"tensor {t}: keep {k} is not in [1, {n}]")
        self._refuse_records(in_dtype, "the mean around the median", "s")
        self._check_table(table, in_dtype)
        p, _ = table.arrays()
        ot = self._out_table(outs, out_dtype)
        ks = (ctypes.c_int32 * T)(*keeps)
        _native.check(
            self._lib.fedavg_mean_around_median(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), table.num_clients, ks, ot,
                out_code(out_dtype), self.stream,
            )
        )

    def pairwise_sqdist(self, table: ClientTable, in_dtype: torch.dtype) -> torch.Tensor:
        """The n x n fp64 matrix (on the device) of squared distances between the table's clients'
        whole updates, ``D[i][j] = sum_e (x_i[e] - x_j[e])^2`` in fp64 (``fedavg_pairwise_sqdist``;
        not a reference algorithm): the device half of Krum. Exactly symmetric, +0.0
        on the diagonal, the same bits on every run. The table's weights are ignored and the
        accumulator is not touched. Refused before any launch: an empty table, more than 256
        clients, an absent entry (distances compare whole updates), quantised records."""
        self._refuse_before_table(table, in_dtype, "pairwise distances", "", _native.KRUM_MAX_CLIENTS)
        p = self._whole_updates(table, in_dtype, "distances compare")
        n = table.num_clients
        out = torch.empty((n, n), dtype=torch.float64, device=self.device)
        _native.check(
            self._lib.fedavg_pairwise_sqdist(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), n, ctypes.c_void_p(out.data_ptr()), self.stream,
            )
        )
        return out

    def sqdist_to_point(self, table: ClientTable, in_dtype: torch.dtype,
                        point: Sequence[torch.Tensor] | None = None) -> torch.Tensor:
        """The length-n fp64 tensor (on the device) of squared distances of the table's clients'
        whole updates to ``point``, ``out[i] = sum_e (x_i[e] - z[e])^2`` in fp64 with separately
        rounded subtract, square and add (``fedavg_sqdist_to_point``; not a reference algorithm,
        DESIGN.md §5i): the device half of the geometric median. ``point`` is one contiguous fp64
        tensor per segment on the context's device; ``None`` is the origin (the squared norms). The
        same bits on every run, whatever the other clients of the table. The table's weights are
        ignored and the accumulator is not touched. Refused before any launch: an empty table, more
        than 1024 clients, an absent entry, quantised records, a point that does not match."""
        self._refuse_before_table(table, in_dtype, "distances to a point", "", _native.POINT_MAX_CLIENTS)
        p = self._whole_updates(table, in_dtype, "distances compare")
        zp = None if point is None else self._segment_array("point", point)
        n = table.num_clients
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        _native.check(
            self._lib.fedavg_sqdist_to_point(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), n, zp, ctypes.c_void_p(out.data_ptr()),
                self.stream,
            )
        )
        return out

    def moments_about_point(self, table: ClientTable, in_dtype: torch.dtype,
                            centre: Sequence[torch.Tensor] | None,
                            direction: Sequence[torch.Tensor]) -> tuple[torch.Tensor, torch.Tensor]:
        """``(dots, sqnorms)``: two length-n fp64 tensors (on the device) with
        ``dots[i] = sum_e (x_i[e] - v[e]) * g[e]`` and ``sqnorms[i] = sum_e (x_i[e] - v[e])^2`` over
        the table's clients' whole updates, from one pass over the client bytes
        (``fedavg_moments_about_point``; not a reference algorithm): the device half
        of FLTrust's trust scores. Per element five separately rounded fp64 operations — subtract,
        square, multiply, two adds — in the pinned order of §5i, so ``sqnorms`` is bit for bit
        ``sqdist_to_point(table, in_dtype, centre)``. ``centre`` (``None``: the origin) and
        ``direction`` are one contiguous fp64 tensor per segment on the context's device. The table's
        weights are ignored and the accumulator is not touched. Refused before any launch: an empty
        table, more than 1024 clients, an absent entry, quantised records, a centre or a direction
        that does not match."""
        self._refuse_before_table(table, in_dtype, "moments about a point", "", _native.POINT_MAX_CLIENTS)
        p = self._whole_updates(table, in_dtype, "moments compare")
        if direction is None:
            raise ValueError("the direction is required")
        vp = None if centre is None else self._segment_array("centre", centre)
        gp = self._segment_array("direction", direction)
        n = table.num_clients
        out = torch.empty((2, n), dtype=torch.float64, device=self.device)
        _native.check(
            self._lib.fedavg_moments_about_point(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), n, vp, gp, ctypes.c_void_p(out.data_ptr()),
                self.stream,
            )
        )
        return out[0], out[1]

    def fold_about_point(self, table: ClientTable, in_dtype: torch.dtype, coefficients: Sequence[float],
                         divisor: float, point: Sequence[torch.Tensor], outs: Sequence[torch.Tensor],
                         out_dtype: torch.dtype = torch.float64) -> None:
        """``outs[t][e] = z[e] + (sum_i c_i * (x_i[e] - z[e])) / divisor`` for every element of every
        segment, ``z = point[t]`` (``fedavg_fold_about_point``; not a reference algorithm, DESIGN.md
        §5j): the device half of centred clipping's step. Per element five separately rounded fp64
        operations — subtract, multiply, add in table order (the first product starts the sum),
        IEEE divide, add — and, for ``out_dtype=float32``, one rounding to nearest even. ``point`` is
        one contiguous fp64 tensor per segment on the context's device, ``outs`` one contiguous
        ``out_dtype`` tensor per segment, none of them the point's own storage. The table's weights
        are ignored and the accumulator is not touched. Refused before any launch: an empty table,
        more than 1024 clients, an absent entry, quantised records, a non-finite coefficient, a
        divisor that is not finite and > 0, a point or an output that does not match, an output
        that is its point."""
        self._refuse_before_table(table, in_dtype, "the fold about a point", "s", _native.POINT_MAX_CLIENTS)
        ocode = out_code(out_dtype)
        p = self._whole_updates(table, in_dtype, "the fold about a point takes")
        n = table.num_clients
        coef = _client_scalars(coefficients, n, "coefficient")
        divisor = _divisor(divisor)
        zp, op = self._source_and_outputs("point", point, outs, out_dtype, NOT_IN_PLACE)
        _native.check(
            self._lib.fedavg_fold_about_point(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), coef.ctypes.data_as(_DBL), n, divisor, zp, op,
                ocode, self.stream,
            )
        )

    def sparse_aggregate_delta(self, rows: Sequence[Sequence[SparseDelta]] | SparseTable, weights: Sequence[float],
                               divisor: float,
                               base: Sequence[torch.Tensor], outs: Sequence[torch.Tensor],
                               out_dtype: torch.dtype = torch.float64, check_indices: bool = True) -> None:
        """FedAvg of sparse deltas against ``base`` in one launch (``fedavg_sparse_aggregate_delta``,
        DESIGN.md §5n): ``outs[t][e] = (sum_i (base[t][e] + d_i[e]) * w_i) / divisor`` with ``d_i[e]``
        the value client ``i`` stores for ``e`` or ``+0.0`` — bit for bit the reference's ``restore()``
        + ``FedAVGAlgorithm`` on the densified deltas, and ``aggregate_delta`` on them. ``rows[i][t]``
        is client ``i``'s ``SparseDelta`` of segment ``t`` on the context's device, all of one value
        dtype (or a ``SparseTable`` built from such rows once, for a table that is folded many times);
        ``base`` one contiguous fp64 tensor per segment, ``outs`` one contiguous ``out_dtype``
        tensor per segment, none of them its base's own storage. The accumulator is not touched; the
        NaN flags are the caller's to read (``raise_on_nan``). With ``check_indices`` the call then
        waits for the stream and raises ``ValueError`` if an index array is not strictly increasing
        inside its tensor (the outputs are unspecified then, nothing outside them was written; a NaN
        flag that the same fold latched stays latched, since clearing it is ``reset()``, which also
        forgets the accumulator: a caller that keeps the context reads ``flags()`` and resets).
        Refused before any launch: no clients, more than 1024, a delta that does not match its
        segment, mixed value dtypes, a non-finite weight, a divisor that is not finite and > 0, a
        base or an output that does not match, an output that is its base."""
        ocode = out_code(out_dtype)
        table = rows if isinstance(rows, SparseTable) else SparseTable(rows, self.layout, self.device)
        if table.layout != self.layout or table.device != self.device:
            raise ValueError("the sparse table was built for another layout or device")
        n, iptr, vptr, nnz, vcode = table.num_clients, table.iptr, table.vptr, table.nnz, dtype_code(table.dtype)
        w = _client_scalars(weights, n, "weight")
        divisor = _divisor(divisor)
        zp, op = self._source_and_outputs("base", base, outs, out_dtype, "the sparse fold is not in-place")
        _native.check(
            self._lib.fedavg_sparse_aggregate_delta(
                self._h, iptr.ctypes.data_as(_PTR), vptr.ctypes.data_as(_PTR),
                nnz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), vcode, w.ctypes.data_as(_DBL), n, divisor, zp, op,
                ocode, self.stream,
            )
        )
        if check_indices and self.sparse_index_errors():
            raise ValueError(SPARSE_INDEX_MESSAGE)

    def quant_encode(self, codec: int, tensors: Sequence[torch.Tensor], records: Sequence[torch.Tensor],
                     level: int = 255, weight: float = 0.01, seed: int = 0, draw: int = 0,
                     tensor_ids: Sequence[int] | None = None) -> None:
        """Encode ``tensors`` (contiguous fp32 or fp64 tensors of one dtype on the context's device,
        of any sizes: the context's layout plays no part) into QSGD or NNADQ records in three
        launches (``fedavg_quant_encode``). ``codec`` is one of ``_native.QSGD_F32 /
        QSGD_F64 / NNADQ_F32 / NNADQ_F64`` and names the tensors' dtype; ``records[t]`` is a 16-byte
        aligned uint8 tensor of the record's size, every byte of which is written (it may be
        uninitialised). ``tensor_ids[t]`` is the tensor's word of the uniform stream's counter
        (default: its position). Asynchronous; a non-finite element latches the input flag, which
        ``raise_on_nan`` turns into ``NaNAggregationError``."""
        if codec not in _native.RECORD_CODES:
            raise ValueError(f"codec {codec} is not a record format")
        dt = torch.float64 if codec in (_native.QSGD_F64, _native.NNADQ_F64) else torch.float32
        T = len(tensors)
        if T == 0 or len(records) != T:
            raise ValueError("one record per tensor and at least one tensor are required")
        ids = _stream_ids(seed, draw, tensor_ids, T)
        numels = [x.numel() for x in tensors]
        needs = [_native.record_bytes(codec, n) for n in numels]
        t, fault = _first(T, self._first_unfit(tensors, dt), self._first_unfit(records, torch.uint8, needs))
        if fault == 0:
            raise self._flat_refusal("tensor", t, dt)
        if fault == 1:
            raise self._record_refusal(t, needs[t])
        iptr, rptr, numels = _addresses(tensors, numels), _addresses(records, needs), np.array(numels, dtype=np.int64)
        _native.check(
            self._lib.fedavg_quant_encode(
                self._h, codec, iptr.ctypes.data, numels.ctypes.data, ids.ctypes.data, T, rptr.ctypes.data,
                int(level), float(weight), int(seed), int(draw), self.stream,
            )
        )

    def quant_decode(self, codec: int, records: Sequence[torch.Tensor], outs: Sequence[torch.Tensor],
                     outs64: Sequence[torch.Tensor] | None = None) -> None:
        """Decode QSGD or NNADQ ``records`` of one codec (16-byte aligned uint8 tensors on the
        context's device: the context's layout plays no part) into ``outs`` in one launch
        (``fedavg_quant_decode``). ``codec`` is one of ``_native.QSGD_F32 / QSGD_F64 /
        NNADQ_F32 / NNADQ_F64`` and names the outputs' dtype; ``outs[t]`` is a contiguous tensor of
        that dtype, aligned to its element only, whose element count is the record's, and exactly
        those elements are written. ``outs64`` (fp32 codecs only) are fp64 tensors of the same sizes
        that receive the exact widening of the same values in the same pass. Asynchronous; a header
        whose level lies outside [1, 255] or a decoded element that is not finite latches the input
        flag, which ``raise_on_nan`` turns into ``NaNAggregationError``."""
        if codec not in _native.RECORD_CODES:
            raise ValueError(f"codec {codec} is not a record format")
        f64 = codec in (_native.QSGD_F64, _native.NNADQ_F64)
        dt = torch.float64 if f64 else torch.float32
        T = len(records)
        if T == 0 or len(outs) != T or (outs64 is not None and len(outs64) != T):
            raise ValueError("one output per record and at least one record are required")
        if outs64 is not None and f64:
            raise ValueError("the fp64 copy is offered for the fp32 codecs: an fp64 codec's output is fp64")
        numels = [o.numel() for o in outs]
        needs = [_native.record_bytes(codec, n) for n in numels]
        t, fault = _first(T, self._first_unfit(outs, dt), self._first_unfit(records, torch.uint8, needs),
                          T if outs64 is None else self._first_unfit(outs64, torch.float64, numels))
        if fault == 0:
            raise self._flat_refusal("output", t, dt)
        if fault == 1:
            raise self._record_refusal(t, needs[t])
        if fault == 2:
            raise self._flat_refusal("fp64 output", t, torch.float64, numels[t])
        rptr, optr = _addresses(records, needs), _addresses(outs, numels)
        wptr = None if outs64 is None else _addresses(outs64, numels)
        numels = np.array(numels, dtype=np.int64)
        _native.check(
            self._lib.fedavg_quant_decode(
                self._h, codec, rptr.ctypes.data, numels.ctypes.data, T, optr.ctypes.data,
                None if wptr is None else wptr.ctypes.data, self.stream,
            )
        )

    def dp_noise(self, tensors: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], C: float, noise_scale: float,
                 seed: int = 0, draw: int = 0, tensor_ids: Sequence[int] | None = None, row_len: int = 0) -> None:
        """Clip and noise ``tensors`` (contiguous tensors of one floating dtype on the context's
        device, of any sizes: the context's layout plays no part) into ``outs`` in three launches
        (``fedavg_dp_noise``). ``row_len == 0``: all tensors together are one vector
        with one L2 norm; ``row_len > 0``: one tensor whose rows of ``row_len`` elements each have
        their own. ``outs[t]`` has the dtype and size of ``tensors[t]`` and may be ``tensors[t]``
        itself. ``noise_scale`` is ``sigma * C``; ``tensor_ids[t]`` is the tensor's word of the normal
        stream's counter (default: its position). Asynchronous; a non-finite element latches the
        input flag (``flags()``)."""
        T = len(tensors)
        if T == 0 or len(outs) != T:
            raise ValueError("one output per tensor and at least one tensor are required")
        ids = _stream_ids(seed, draw, tensor_ids, T)
        dt = tensors[0].dtype
        if dt not in DTYPE_CODES:
            raise TypeError(f"the clip-and-noise pass takes fp32, fp16, bf16 or fp64 tensors, not {dt}")
        numels = [x.numel() for x in tensors]
        t, fault = _first(T, self._first_unfit(tensors, dt), self._first_unfit(outs, dt, numels))
        if fault == 0:
            raise self._flat_refusal("tensor", t, dt)
        if fault == 1:
            raise self._flat_refusal("output", t, dt, numels[t])
        iptr, optr, numels = _addresses(tensors, numels), _addresses(outs, numels), np.array(numels, dtype=np.int64)
        _native.check(
            self._lib.fedavg_dp_noise(
                self._h, DTYPE_CODES[dt], iptr.ctypes.data, numels.ctypes.data, ids.ctypes.data, T, optr.ctypes.data,
                int(row_len), float(C), float(noise_scale), int(seed), int(draw), self.stream,
            )
        )

    def topk_sparsify(self, deltas: Sequence[torch.Tensor], errors: Sequence[torch.Tensor | None] | None,
                      keeps: Sequence[int], indices: Sequence[torch.Tensor], values: Sequence[torch.Tensor],
                      residuals: Sequence[torch.Tensor]) -> None:
        """The top-k step with error feedback on ``deltas`` (contiguous tensors of one floating dtype
        on the context's device, of any sizes: the context's layout plays no part) in a fixed number
        of launches (``fedavg_topk_sparsify``): tensor ``t`` sends the ``keeps[t]``
        entries of largest magnitude of ``deltas[t] + errors[t]`` (``errors`` or an entry of it may
        be ``None``: no residual yet), ties to the lower index, as ascending int32 ``indices[t]`` and
        ``values[t]`` (``keeps[t]`` entries each), and leaves what it did not send in
        ``residuals[t]``, which may be ``errors[t]`` or ``deltas[t]`` itself. Asynchronous."""
        T = len(deltas)
        if T == 0 or not (len(keeps) == len(indices) == len(values) == len(residuals) == T) or (
                errors is not None and len(errors) != T):
            raise ValueError("one keep count, index, value and residual tensor per delta and at least one delta "
                             "are required")
        dt = deltas[0].dtype
        if dt not in DTYPE_CODES:
            raise TypeError(f"the top-k step takes fp32, fp16, bf16 or fp64 tensors, not {dt}")
        ns, ks = [x.numel() for x in deltas], [int(k) for k in keeps]
        groups = (("error", errors or (), dt, ns), ("index", indices, torch.int32, ks), ("value", values, dt, ks),
                  ("residual", residuals, dt, ns))
        t, fault = _first(T, self._first_unfit(deltas, dt),
                          next((t for t, (k, n) in enumerate(zip(ks, ns)) if not 0 <= k <= n), T),
                          *[self._first_unfit(g, dty, sizes) if g else T for _, g, dty, sizes in groups])
        if fault == 0:
            raise self._flat_refusal("delta", t, dt)
        if fault == 1:
            raise ValueError(f"delta {t}: keeps {ks[t]} of {ns[t]} elements")
        if fault >= 2:
            what, _, dty, sizes = groups[fault - 2]
            raise self._flat_refusal(what, t, dty, sizes[t])
        xptr, iptr, vptr, rptr = (_addresses(deltas, ns), _addresses(indices, ks), _addresses(values, ks),
                                  _addresses(residuals, ns))
        eptr = None if errors is None else _addresses(errors, ns)
        ns, ks = np.array(ns, dtype=np.int64), np.array(ks, dtype=np.int64)
        _native.check(
            self._lib.fedavg_topk_sparsify(
                self._h, DTYPE_CODES[dt], xptr.ctypes.data, None if eptr is None else eptr.ctypes.data,
                ns.ctypes.data, ks.ctypes.data, T, iptr.ctypes.data, vptr.ctypes.data, rptr.ctypes.data, self.stream,
            )
        )

    def sparse_index_errors(self) -> bool:
        """Wait for the stream and report (once) whether a sparse fold since the last report met an
        index violation (``fedavg_sparse_index_errors``)."""
        out = ctypes.c_int32()
        _native.check(self._lib.fedavg_sparse_index_errors(self._h, self.stream, ctypes.byref(out)))
        return bool(out.value)

    def server_opt_step(self, table: ClientTable, in_dtype: torch.dtype, coefficients: Sequence[float],
                        divisor: float, point: Sequence[torch.Tensor], m_in: Sequence[torch.Tensor],
                        v_in: Sequence[torch.Tensor] | None, m_out: Sequence[torch.Tensor],
                        v_out: Sequence[torch.Tensor] | None, outs: Sequence[torch.Tensor],
                        out_dtype: torch.dtype = torch.float64, *, mode: str, lr: float, beta1: float,
                        beta2: float, tau: float) -> None:
        """One server optimiser step (``fedavg_server_opt_step``; not a reference algorithm, DESIGN.md
        §5m): the pseudo-gradient ``delta = (sum_i c_i * (x_i - z)) / divisor`` of
        ``fold_about_point``, the moments ``m_out``, ``v_out`` from ``m_in``, ``v_in`` by ``mode``
        (``"avgm"``, ``"adagrad"``, ``"yogi"``, ``"adam"``: ``server_opt_update`` states the lines)
        and ``outs = z + u``, in one pass over the client bytes. Every line is one separately rounded
        fp64 operation, the square root is correctly rounded, ``1 - beta`` is computed once here.
        ``point``, ``m_in``, ``v_in``, ``m_out``, ``v_out`` are one contiguous fp64 tensor per segment
        on the context's device (``v_in`` / ``v_out`` are ignored for ``"avgm"`` and may be ``None``),
        ``outs`` one contiguous ``out_dtype`` tensor per segment. Not in-place: ``outs`` is not the
        point and no ``*_out`` is its ``*_in``; the caller swaps its buffers once ``flags()`` came back
        clean. Refused before any launch: what ``fold_about_point`` refuses, the hyper-parameters
        ``check_server_opt`` refuses, moments that do not match or alias."""
        self._refuse_before_table(table, in_dtype, "the server optimiser step", "s", _native.POINT_MAX_CLIENTS)
        ocode = out_code(out_dtype)
        code, lr, beta1, omb1, beta2, omb2, tau = check_server_opt(mode, lr, beta1, beta2, tau)
        p = self._whole_updates(table, in_dtype, "the server optimiser step takes")
        n, T = table.num_clients, table.num_segments
        coef = _client_scalars(coefficients, n, "coefficient")
        divisor = _divisor(divisor)
        adaptive = code != _native.OPT_AVGM
        groups = [("point", point), ("first-moment input", m_in), ("first-moment output", m_out)]
        if adaptive:
            if v_in is None or v_out is None:
                raise ValueError(f"mode {mode!r} needs second-moment tensors")
            groups += [("second-moment input", v_in), ("second-moment output", v_out)]
        if len(outs) != T or any(len(g) != T for _, g in groups):
            raise ValueError("one point, moment and output tensor per segment are required")
        zp, mi, mo, vi, vo = [self._segment_array(what, g) for what, g in groups] + [None] * (5 - len(groups))
        t, fault = _first(T, self._first_unfit(outs, out_dtype, self.layout.numels), _first_shared(point, outs),
                          min(_first_shared(m_in, m_out), _first_shared(v_in, v_out) if adaptive else T))
        if fault == 0:
            raise self._segment_refusal("output", t, out_dtype)
        if fault == 1:
            raise ValueError(f"output tensor {t} is its point: {NOT_IN_PLACE}")
        if fault == 2:
            raise ValueError(f"moment tensor {t}: {NOT_IN_PLACE}")
        op = _pointer_array(outs)
        _native.check(
            self._lib.fedavg_server_opt_step(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), coef.ctypes.data_as(_DBL), n, divisor,
                zp, mi, vi, mo, vo, code, lr, beta1, omb1, beta2, omb2, tau, op, ocode, self.stream,
            )
        )

    def partial(
        self,
        table: ClientTable | None,
        in_dtype: torch.dtype,
        zero_init: bool = True,
        tile_begin: int = 0,
        tile_end: int = -1,
    ) -> None:
        """acc[tiles] = (0 | acc) + sum_k w_k x_k (the shard step of the multi-GPU path)."""
        n = 0 if table is None else table.num_clients
        if table is not None:
            self._check_table(table, in_dtype)
            p, w = table.arrays()
        else:
            p, w = np.zeros(1, np.uint64), np.zeros(1, np.float64)
        _native.check(
            self._lib.fedavg_partial(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype) if n else _native.F32,
                w.ctypes.data_as(_DBL), n, 1 if zero_init else 0, tile_begin, tile_end, self.stream,
            )
        )

    def segment_state(self) -> tuple[list[float], list[int]]:
        """(per-segment total weight, 1 = the accumulator holds folded data) — what
        ``set_segment_state`` sets."""
        tw = (ctypes.c_double * self.layout.num_segments)()
        vv = (ctypes.c_int32 * self.layout.num_segments)()
        _native.check(self._lib.fedavg_segment_state(self._h, tw, vv))
        return list(tw), list(vv)

    def set_segment_state(self, total_weights: Sequence[float], valid: Sequence[int]) -> None:
        """Per-segment accumulated state (a layout grown mid-round keeps its folded segments)."""
        tw = (ctypes.c_double * self.layout.num_segments)(*[float(x) for x in total_weights])
        vv = (ctypes.c_int32 * self.layout.num_segments)(*[1 if v else 0 for v in valid])
        _native.check(self._lib.fedavg_set_segment_state(self._h, tw, vv))

    def accumulate_elementwise(self, table: ClientTable, in_dtype: torch.dtype, totals: torch.Tensor,
                               total_fp32: Sequence[bool]) -> None:
        """Fold a wave with per-element weights (fed_avg_algorithm.py:51-62 with a tensor-valued
        _get_weight): acc += x * w and totals += w elementwise; ``totals`` is an fp64 buffer in
        accumulator coordinates, rounded to fp32 per segment where ``total_fp32``."""
        self._check_table(table, in_dtype)
        if table.num_clients == 0:
            return
        if totals.dtype != torch.float64 or totals.numel() < self.acc_numel or totals.device != self.device:
            raise ValueError("totals: an fp64 buffer of the accumulator's size on the context device")
        p, _ = table.arrays()
        wp, wd, ws = table.elementwise_arrays()
        flags = (ctypes.c_int32 * self.layout.num_segments)(*[1 if f else 0 for f in total_fp32])
        _native.check(self._lib.fedavg_accumulate_elementwise(
            self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), wp.ctypes.data_as(_PTR),
            wd.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ws.ctypes.data_as(_DBL), flags, table.num_clients,
            ctypes.c_void_p(totals.data_ptr()), self.stream))

    def finalize_elementwise(self, totals: torch.Tensor, outs: Sequence[torch.Tensor] | OutputTable,
                             out_dtype: torch.dtype) -> None:
        """out = acc / totals elementwise (fed_avg_algorithm.py:94-97); resets the state."""
        ot = self._out_table(outs, out_dtype)
        _native.check(self._lib.fedavg_finalize_elementwise(self._h, ctypes.c_void_p(totals.data_ptr()), ot,
                                                            out_code(out_dtype), self.stream))

    def set_accumulated(self, total_weights: Sequence[float]) -> None:
        tw = (ctypes.c_double * self.layout.num_segments)(*[float(x) for x in total_weights])
        _native.check(self._lib.fedavg_set_accumulated(self._h, tw))

    def finalize_range(
        self, outs: Sequence[torch.Tensor], out_dtype: torch.dtype, tile_begin: int = 0, tile_end: int = -1
    ) -> None:
        ot = self._out_table(outs, out_dtype)
        _native.check(
            self._lib.fedavg_finalize_range(self._h, ot, out_code(out_dtype), tile_begin, tile_end, self.stream)
        )

    def plan(
        self, table: ClientTable, in_dtype: torch.dtype, outs: Sequence[torch.Tensor] | OutputTable,
        out_dtype: torch.dtype,
    ) -> AggregatePlan:
        """Prepare ``aggregate(table, in_dtype, outs, out_dtype)`` once; ``plan.run()`` repeats it
        with no host staging (the table's tensors and the outputs must stay alive)."""
        self._check_table(table, in_dtype)
        p, w = table.arrays()
        ot = self._out_table(outs, out_dtype)
        h = ctypes.c_void_p()
        _native.check(
            self._lib.fedavg_plan_create(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), w.ctypes.data_as(_DBL),
                table.num_clients, ot, out_code(out_dtype), ctypes.byref(h),
            )
        )
        return AggregatePlan(self, h, keep=(table, outs))

    def plan_partial(self, table: ClientTable | None, in_dtype: torch.dtype, zero_init: bool = True) -> AggregatePlan:
        """Prepared shard partial; ``plan.run_range(tb, te)`` == ``partial(table, ..., tb, te)``."""
        n = 0 if table is None else table.num_clients
        if table is not None:
            self._check_table(table, in_dtype)
            p, w = table.arrays()
        else:
            p, w = np.zeros(1, np.uint64), np.zeros(1, np.float64)
        h = ctypes.c_void_p()
        _native.check(
            self._lib.fedavg_plan_create_partial(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype) if n else _native.F32,
                w.ctypes.data_as(_DBL), n, 1 if zero_init else 0, ctypes.byref(h),
            )
        )
        return AggregatePlan(self, h, keep=(table,))

    def plan_finalize(self, total_weights: Sequence[float], outs: Sequence[torch.Tensor] | OutputTable,
                      out_dtype: torch.dtype) -> AggregatePlan:
        """Prepared finalize with baked totals; ``plan.run_range(tb, te)`` == ``finalize_range``."""
        ot = self._out_table(outs, out_dtype)
        tw = (ctypes.c_double * self.layout.num_segments)(*[float(x) for x in total_weights])
        h = ctypes.c_void_p()
        _native.check(self._lib.fedavg_plan_create_finalize(self._h, tw, ot, out_code(out_dtype), ctypes.byref(h)))
        return AggregatePlan(self, h, keep=(outs,))

    def set_fused_fold(self, enable: bool) -> None:
        """Allow the one-instruction fold when every product is provably exact (default on)."""
        _native.check(self._lib.fedavg_set_fused_fold(self._h, 1 if enable else 0))

    def reset(self) -> None:
        _native.check(self._lib.fedavg_reset(self._h, self.stream))

    # -- dynamic waves (fedavg_dyn_*: the round's first wave folded while clients arrive) -
    def dyn_open(self, in_dtype: torch.dtype, max_clients: int) -> None:
        _native.check(self._lib.fedavg_dyn_open(self._h, dtype_code(in_dtype), int(max_clients), self.stream))

    def dyn_publish(self, table: ClientTable) -> int:
        """Hand the table's unpublished rows to the open wave; the rows published now (0 while
        the current stream still has unfinished work). NativeError for a row the wave cannot take
        (its ``published``: the rows before it, published)."""
        p, w = _table_args(table)
        n = ctypes.c_int32()
        st = self._lib.fedavg_dyn_publish(self._h, p, w, table.num_clients, self.stream, ctypes.byref(n))
        if st != _native.OK:  # the rows before the one it cannot take were published: e.published
            err = _native.NativeError(st, _native.last_error())
            err.published = int(n.value)
            raise err
        return int(n.value)

    def dyn_close(self, outs: Sequence[torch.Tensor] | OutputTable | None = None,
                  out_dtype: torch.dtype = torch.float64, join: bool = True) -> tuple[int, bool]:
        """(rows folded, finalized): with ``outs`` the wave divides into them (finalized), else —
        or when it ended itself — it leaves rows [0, folded) in the accumulator. ``join=False``:
        a finalized wave's outputs are complete after the next ``flags`` / ``raise_on_nan``."""
        ot = self._out_table(outs, out_dtype) if outs is not None else None
        folded, fin = ctypes.c_int32(), ctypes.c_int32()
        _native.check(self._lib.fedavg_dyn_close(self._h, ot, out_code(out_dtype), 1 if join else 0, self.stream,
                                                 ctypes.byref(folded), ctypes.byref(fin)))
        return int(folded.value), bool(fin.value)

    def dyn_prof_collect(self) -> tuple[float, int]:
        """(ms, waves): the closed dynamic waves' body launches, enqueue to end, while profiling."""
        ms, n = ctypes.c_double(), ctypes.c_int32()
        _native.check(self._lib.fedavg_dyn_prof_collect(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def dyn_state(self) -> tuple[bool, int]:
        a, p = ctypes.c_int32(), ctypes.c_int32()
        _native.check(self._lib.fedavg_dyn_state(self._h, ctypes.byref(a), ctypes.byref(p)))
        return bool(a.value), int(p.value)

    def dyn_configure(self, idle_us: int = 0, life_us: int = 0) -> None:
        """The wave's idle limit / lifetime (µs) for the following launches (0: unchanged)."""
        _native.check(self._lib.fedavg_dyn_configure(self._h, int(idle_us), int(life_us)))

    def dyn_timing(self) -> dict[str, float]:
        """fedavg_dyn_timing of the last completed wave (µs, GPU clock; -1 where not recorded)."""
        v = (ctypes.c_double * 3)()
        _native.check(self._lib.fedavg_dyn_timing(self._h, v, 3))
        return dict(zip(("rows_to_end_us", "close_to_end_us", "rows_to_close_us"), (float(x) for x in v)))

    def dyn_info(self) -> dict[str, int]:
        """fedavg_dyn_info: the open wave's state and this context's continued waves / launches."""
        v = (ctypes.c_int32 * 5)()
        _native.check(self._lib.fedavg_dyn_info(self._h, v, 5))
        return dict(zip(("active", "published", "base", "reopens", "launches"), (int(x) for x in v)))

    # -- fault reporting ---------------------------------------------------------------
    def flags(self) -> int:
        """Synchronise the stream and return the latched NaN flag bits."""
        f = ctypes.c_uint32()
        st = self._lib.fedavg_check(self._h, self.stream, ctypes.byref(f))
        if st not in (_native.OK, _native.ERR_NAN_INPUT, _native.ERR_NAN_ACCUM, _native.ERR_NAN_RESULT):
            _native.check(st)
        return int(f.value)

    def find_nan_clients(self, table: ClientTable, in_dtype: torch.dtype) -> list[int]:
        p, _ = table.arrays()
        out = (ctypes.c_int32 * table.num_clients)()
        _native.check(
            self._lib.fedavg_find_nan_clients(
                self._h, p.ctypes.data_as(_PTR), dtype_code(in_dtype), table.num_clients, out, self.stream
            )
        )
        return [i for i in range(table.num_clients) if out[i]]

    def raise_on_nan(self, tables: Sequence[tuple[ClientTable, torch.dtype]] = ()) -> None:
        """Map the latched flags onto the reference's assertions.

        Input NaN (fed_avg_algorithm.py:35) and an accumulator NaN (:93) both leave the fp64
        accumulator NaN; the client tables still held by the caller are scanned to tell them
        apart and name the offending clients.
        """
        f = self.flags()
        if f == 0:
            return
        # the flag is sticky until reset: clear it so the context stays usable
        self.reset()
        if f & _native.FLAG_INPUT_NAN:  # the robust rules check their inputs in the same pass
            for table, dt in tables:
                bad = self.find_nan_clients(table, dt)
                if bad:
                    raise NaNAggregationError("input", f"NaN in client update(s) at table rows {bad}", bad)
            raise NaNAggregationError("input", "NaN in a client update")
        if f & _native.FLAG_ACC_NAN:
            for table, dt in tables:
                bad = self.find_nan_clients(table, dt)
                if bad:
                    raise NaNAggregationError("input", f"NaN in client update(s) at table rows {bad}", bad)
            raise NaNAggregationError("accumulator", "NaN in the weighted sum (e.g. inf - inf)")
        raise NaNAggregationError("result", "NaN after dividing by the total weight (e.g. 0 / 0)")

    # -- measurement -------------------------------------------------------------------
    def prof_enable(self, on: bool = True) -> None:
        _native.check(self._lib.fedavg_prof_enable(self._h, 1 if on else 0))

    def prof_collect(self) -> tuple[float, int]:
        ms, n = ctypes.c_double(), ctypes.c_int32()
        _native.check(self._lib.fedavg_prof_collect(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


class AggregatePlan:
    """A prepared fused aggregation (``fedavg_plan_*``)."""

    def __init__(self, ctx: FedAvgContext, handle: ctypes.c_void_p, keep: tuple) -> None:
        self.ctx = ctx
        self._h = handle
        self._keep = keep
        ctx._plans.add(self)  # closed with the context (a native plan points at its context)

    def run(self) -> None:
        _native.check(self.ctx._lib.fedavg_plan_run(self._h, self.ctx.stream))

    def run_range(self, tile_begin: int, tile_end: int) -> None:
        _native.check(self.ctx._lib.fedavg_plan_run_range(self._h, tile_begin, tile_end, self.ctx.stream))

    # -- scatter exchange pieces (finalize plans; sharded.py) ---------------------------
    @property
    def out_dtype(self) -> torch.dtype:
        code = int(self.ctx._lib.fedavg_plan_out_dtype(self._h))
        return {_native.F32: torch.float32, _native.F64: torch.float64}[code]

    def finalize_window(self, src: torch.Tensor, lo: int, hi: int, res: torch.Tensor) -> None:
        """res[p] = src[p - lo] / W[seg(p)] over accumulator positions [lo, hi) (padding skipped);
        ``res`` is in accumulator coordinates, of the plan's out dtype."""
        if src.dtype != torch.float64 or src.numel() < hi - lo or res.dtype != self.out_dtype \
                or res.numel() < self.ctx.acc_numel or not (src.is_contiguous() and res.is_contiguous()):
            raise ValueError("window buffers do not match the plan")
        _native.check(self.ctx._lib.fedavg_plan_finalize_window(
            self._h, ctypes.c_void_p(src.data_ptr()), lo, hi, ctypes.c_void_p(res.data_ptr()), self.ctx.stream))

    def copy_out(self, res: torch.Tensor) -> None:
        """The plan's outputs <- res (accumulator coordinates)."""
        if res.dtype != self.out_dtype or res.numel() < self.ctx.acc_numel or not res.is_contiguous():
            raise ValueError("result buffer does not match the plan")
        _native.check(self.ctx._lib.fedavg_plan_copy_out(self._h, ctypes.c_void_p(res.data_ptr()), self.ctx.stream))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            self.ctx._lib.fedavg_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def bw_probe(src: torch.Tensor, dst: torch.Tensor, mode: int) -> None:
    """HBM ceiling probe: mode 0 copies src->dst (16-B lanes), mode 1 only reads src."""
    lib = _native.load()
    nbytes = src.numel() * src.element_size()
    _native.check(
        lib.fedavg_bw_probe(
            ctypes.c_void_p(src.data_ptr()), nbytes, ctypes.c_void_p(dst.data_ptr()), mode,
            _stream_handle(src.device),
        )
    )


class RowRouter:
    """One native routing handle (``fedavg_route_*`` of ``include/fedavg_hip.h``): the dense table
    node -> sent row, the call's workspace and the error bits, on one device. It owns no model
    layout. Calls launch on the current torch stream of the device; one stream at a time."""

    def __init__(self, device: torch.device | str | int | None = None, lib: ctypes.CDLL | None = None) -> None:
        self._lib = lib if lib is not None else _native.load()
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("the routed row gather runs on a GPU device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        handle = ctypes.c_void_p()
        _native.check(self._lib.fedavg_route_create(ctypes.byref(handle), device.index))
        self._h = handle

    def route_rows(self, sources: Sequence[torch.Tensor], src_ids: torch.Tensor | None, want_ids: torch.Tensor | None,
                   want_off: np.ndarray, node_space: int, out_rows: torch.Tensor | None, out_ids: torch.Tensor | None,
                   out_count: torch.Tensor, row_bytes: int, elem_bytes: int) -> None:
        """One ``fedavg_route_rows`` call. ``sources`` are contiguous row blocks on the device
        (``sources[s][i]`` is a row of ``row_bytes`` bytes), ``src_ids`` / ``want_ids`` / ``out_ids``
        int64 device tensors, ``want_off`` a host int64 array of ``len(out_count) + 1`` offsets and
        ``out_count`` an int32 device tensor. The library validates the rest."""
        S = len(sources)
        ptrs = np.fromiter((t.data_ptr() for t in sources), dtype=np.uint64, count=S)
        rows = np.fromiter((t.shape[0] for t in sources), dtype=np.int64, count=S)
        want_off = np.ascontiguousarray(want_off, dtype=np.int64)

        def addr(t: torch.Tensor | None) -> int | None:
            return None if t is None else t.data_ptr()

        _native.check(self._lib.fedavg_route_rows(
            self._h, ptrs.ctypes.data if S else None, rows.ctypes.data if S else None, S, row_bytes, elem_bytes,
            addr(src_ids), addr(want_ids), want_off.ctypes.data, len(want_off) - 1, node_space, addr(out_rows),
            addr(out_ids), addr(out_count), _stream_handle(self.device)))

    def errors(self) -> int:
        """Wait for the stream, report the error bits latched since the last report
        (``_native.ROUTE_ERR_*``) and clear them."""
        out = ctypes.c_int32(0)
        _native.check(self._lib.fedavg_route_errors(self._h, _stream_handle(self.device), ctypes.byref(out)))
        return int(out.value)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.fedavg_route_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass
