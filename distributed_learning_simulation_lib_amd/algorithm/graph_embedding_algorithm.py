"""The reference's ``GraphNodeEmbeddingPassingAlgorithm``
(``simulation_lib/algorithm/graph_embedding_algorithm.py:9-65``) with the routing on the GPU.

Once per GNN layer and mini-batch every graph worker sends the embeddings of its boundary nodes as
an in-round ``FeatureMessage`` (``feature[i]`` is the row of node ``other_data["node_indices"][i]``)
together with the set of foreign nodes it needs (``other_data["boundary"]``), and blocks for the
answer: per worker, the sorted ids of its boundary that somebody sent and those nodes' rows.

The reference answers from nested Python loops over a dict; here the whole round is one
``fedavg_route_rows`` call (``include/fedavg_hip.h``, ``csrc/route_kernels.hip``): a routed copy, so
the rows are the reference's bytes by construction. On a CPU ``device`` the same rule (a dense
lookup table, ``index_select``) runs in torch and gives the same bytes.

Differences from the reference, all of them in what is accepted or when an error shows:

* a boundary may be a ``set`` (as the reference sends it) or a sorted int64 tensor, on the host or
  on the device (the fast path: no per-call sort); ``node_indices`` may be any sequence or tensor;
* a node id sent twice is an ``AssertionError`` as in the reference, but it is raised by
  ``aggregate_worker_data`` (the kernel finds it by write-then-verify), not at arrival;
* ``ValueError`` naming the worker for mixed dtypes, mixed row shapes, a negative sent id,
  ``len(node_indices) != feature.shape[0]`` or a tensor boundary that is not strictly increasing;
* ``NotImplementedError`` for more than 1024 feature messages or a node id of 2^28 or more;
* the features stay on ``device`` (``output_device="cpu"`` returns host tensors like the reference,
  by one copy of the packed buffer; the per-worker features are views of it).
"""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from .. import _native
from ..message import Message, is_feature_message, wire_class
from .aggregation_algorithm import AggregationAlgorithm, default_device


def _ids_to_host(ids: Any) -> np.ndarray:
    if isinstance(ids, torch.Tensor):
        return ids.detach().to(device="cpu", dtype=torch.int64).reshape(-1).numpy()
    if isinstance(ids, np.ndarray):
        return np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    return np.fromiter(ids, dtype=np.int64)


class GraphNodeEmbeddingPassingAlgorithm(AggregationAlgorithm):
    def __init__(self, device: torch.device | str | None = None,
                 output_device: torch.device | str | None = None) -> None:
        super().__init__()
        self._device = torch.device(device) if device is not None else None
        self._output_device = torch.device(output_device) if output_device is not None else None
        self.__features: list[tuple[int, torch.Tensor, np.ndarray]] = []  # (worker, rows, their node ids)
        # worker -> its boundary: a sorted int64 host array, or a device tensor (taken as sorted)
        self.__boundaries: dict[int, np.ndarray | torch.Tensor] = {}
        self.__like: Any = None
        self.__router: Any = None

    @property
    def device(self) -> torch.device:
        if self._device is None:
            self._device = default_device()
        if self._device.type == "cuda" and self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    # ---- arrival (graph_embedding_algorithm.py:16-32) ---------------------------------------
    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is None or not is_feature_message(worker_data):
            return False
        feature = worker_data.feature
        if feature is not None:
            node_indices = _ids_to_host(worker_data.other_data.pop("node_indices"))
            if feature.dim() < 1 or node_indices.shape[0] != feature.shape[0]:
                raise ValueError(f"worker {worker_id}: {node_indices.shape[0]} node indices for a feature of shape "
                                 f"{tuple(feature.shape)}")
            if node_indices.size and int(node_indices.min()) < 0:
                raise ValueError(f"worker {worker_id}: a negative node index")
            if self.__features:
                first = self.__features[0][1]
                if feature.dtype != first.dtype:
                    raise ValueError(f"worker {worker_id}: feature dtype {feature.dtype}, the round's is {first.dtype}")
                if feature.shape[1:] != first.shape[1:]:
                    raise ValueError(f"worker {worker_id}: feature rows of shape {tuple(feature.shape[1:])}, the "
                                     f"round's are {tuple(first.shape[1:])}")
            if len(self.__features) >= _native.ROUTE_MAX_SOURCES:
                raise NotImplementedError(f"more than {_native.ROUTE_MAX_SOURCES} feature messages in one round")
            if node_indices.size and int(node_indices.max()) >= _native.ROUTE_MAX_NODE_SPACE:
                raise NotImplementedError(f"worker {worker_id}: a node index of 2^28 or more")
            device = self.device
            if feature.device != device:
                feature = feature.to(device)
            self.__features.append((worker_id, feature.detach().contiguous(), node_indices))
        boundary = worker_data.other_data.pop("boundary")
        assert not worker_data.other_data
        if isinstance(boundary, torch.Tensor):
            if boundary.dtype != torch.int64 or boundary.dim() != 1:
                raise ValueError(f"worker {worker_id}: a tensor boundary is a 1-d int64 tensor")
            if boundary.device.type == "cpu" or self.device.type == "cpu":
                boundary = boundary.detach().cpu().contiguous().numpy()
                if boundary.size > 1 and not bool((boundary[1:] > boundary[:-1]).all()):
                    raise ValueError(f"worker {worker_id}: a tensor boundary must be strictly increasing")
            else:
                boundary = boundary.detach().to(self.device).contiguous()
        else:
            boundary = np.fromiter(boundary, dtype=np.int64, count=len(boundary))
            boundary.sort()
        self.__boundaries[worker_id] = boundary
        self.__like = worker_data
        return True

    # ---- the round (graph_embedding_algorithm.py:38-59) -------------------------------------
    def aggregate_worker_data(self) -> Message:
        assert self.__features or self.__boundaries
        workers = list(self.__boundaries)
        counts, ids, rows = self._route_cpu() if self.device.type == "cpu" else self._route_gpu()
        feature_cls = wire_class(self.__like, "FeatureMessage")
        worker_data: dict[int, Message] = {}
        pos = 0
        for j, worker_id in enumerate(workers):
            n = len(self.__boundaries[worker_id])
            c = int(counts[j])
            worker_data[worker_id] = feature_cls(
                feature=rows[pos: pos + c] if c else None,
                other_data={"node_indices": tuple(ids[pos: pos + c].tolist())},
                in_round=True,
            )
            pos += n
        return wire_class(self.__like, "MultipleWorkerMessage")(in_round=True, worker_data=worker_data)

    def _sent(self) -> tuple[np.ndarray, int]:
        """The sent node ids in source order and the node space they span."""
        if not self.__features:
            return np.zeros(0, np.int64), 0
        src_ids = np.concatenate([ids for _, _, ids in self.__features])
        return src_ids, (int(src_ids.max()) + 1 if src_ids.size else 0)

    def _to_output(self, rows: torch.Tensor | None) -> torch.Tensor | None:
        if rows is None or self._output_device is None or rows.device == self._output_device:
            return rows
        return rows.to(self._output_device)  # the packed buffer, once

    def _route_cpu(self) -> tuple[np.ndarray, np.ndarray, torch.Tensor | None]:
        src_ids, node_space = self._sent()
        table = np.full(node_space, -1, dtype=np.int64)
        table[src_ids] = np.arange(src_ids.size, dtype=np.int64)
        # write-then-verify, as the kernel does
        assert bool((table[src_ids] == np.arange(src_ids.size)).all()), "a node index was sent twice"
        lists = [self.__boundaries[w] for w in self.__boundaries]
        total = sum(len(b) for b in lists)
        counts = np.zeros(len(lists), np.int32)
        ids = np.zeros(total, np.int64)
        picks = np.zeros(total, np.int64)
        pos = 0
        for j, b in enumerate(lists):
            inside = b[(b >= 0) & (b < node_space)]
            hit = inside[table[inside] >= 0]
            counts[j] = hit.size
            ids[pos: pos + hit.size] = hit
            picks[pos: pos + hit.size] = table[hit]
            pos += len(b)
        rows = None
        if self.__features and total:
            cat = torch.cat([f for _, f, _ in self.__features]) if len(self.__features) > 1 else self.__features[0][1]
            rows = cat.index_select(0, torch.from_numpy(picks)) if cat.shape[0] else cat.new_empty((total,) + cat.shape[1:])
        return counts, ids, self._to_output(rows)

    def _route_gpu(self) -> tuple[np.ndarray, np.ndarray, torch.Tensor | None]:
        from ..fedavg import RowRouter

        device = self.device
        if self.__router is None:
            self.__router = RowRouter(device)
        src_ids, node_space = self._sent()
        lists = [self.__boundaries[w] for w in self.__boundaries]
        N = len(lists)
        want_off = np.zeros(N + 1, np.int64)
        np.cumsum([len(b) for b in lists], out=want_off[1:])
        B, R = int(want_off[N]), int(src_ids.size)
        # one upload: the sent ids, then the boundaries that live on the host
        host = [src_ids] + [b for b in lists if isinstance(b, np.ndarray)]
        dev_ids = torch.from_numpy(np.concatenate(host)).to(device) if R + B else None
        if all(isinstance(b, np.ndarray) for b in lists):
            want = dev_ids[R:] if dev_ids is not None else None
        else:
            pieces, pos = [], R
            for b in lists:
                if isinstance(b, np.ndarray):
                    pieces.append(dev_ids[pos: pos + len(b)])
                    pos += len(b)
                else:
                    pieces.append(b)
            want = torch.cat(pieces)
        sources = [f for _, f, _ in self.__features]
        if sources:
            first = sources[0]
            elem = first.element_size()
            row_bytes = elem * int(np.prod(first.shape[1:], dtype=np.int64))
            if row_bytes == 0:
                raise ValueError("feature rows hold no element")
            out_rows = rows = torch.empty((B,) + tuple(first.shape[1:]), dtype=first.dtype, device=device)
        else:  # nobody sent a feature: every list misses, into one-byte rows that are never written
            elem, row_bytes, rows = 1, 1, None
            out_rows = torch.empty(B, dtype=torch.uint8, device=device)
        # out_ids [B] int64 and out_count [N] int32 share one buffer: one copy brings both back
        meta = torch.empty(B + (N + 1) // 2, dtype=torch.int64, device=device)
        out_count = meta[B:].view(torch.int32)[:N]
        self.__router.route_rows(sources, dev_ids[:R] if R else None, want if B else None, want_off, node_space,
                                 out_rows if B else None, meta[:B] if B else None, out_count, row_bytes, elem)
        meta_host = meta.cpu().numpy()
        errors = self.__router.errors()
        assert not errors & _native.ROUTE_ERR_DUPLICATE, "a node index was sent twice"
        if errors & _native.ROUTE_ERR_ORDER:
            raise ValueError("a tensor boundary must be strictly increasing")
        assert not errors, f"routing error bits {errors}"
        counts = meta_host[B:].view(np.int32)[:N]
        return counts, meta_host[:B], self._to_output(rows)

    def clear_worker_data(self) -> None:
        super().clear_worker_data()
        self.__features = []
        self.__boundaries = {}

    def exit(self) -> None:
        if self.__router is not None:
            self.__router.close()
            self.__router = None
