"""An independent numpy restatement of the graph embedding exchange, for the
property tests: dicts and ``np.intersect1d``, no table, no torch arithmetic.

``route(sources, boundaries)``: ``sources`` = [(node id list, rows as a numpy array of raw bytes
[n, row_bytes])], ``boundaries`` = [id list] per want list. Returns per list the sorted ids that
somebody sent and those nodes' rows as raw bytes. A node id sent twice is an AssertionError."""

from __future__ import annotations

import numpy as np
import torch


def as_bytes(t: torch.Tensor) -> np.ndarray:
    """The rows of ``t`` as raw bytes [rows, row_bytes]."""
    t = t.detach().cpu().contiguous()
    return t.reshape(t.shape[0], -1).view(torch.uint8).numpy().reshape(t.shape[0], -1)


def route(sources, boundaries):
    where: dict[int, tuple[int, int]] = {}
    for s, (ids, _) in enumerate(sources):
        for i, node in enumerate(ids):
            assert int(node) not in where, "a node index was sent twice"
            where[int(node)] = (s, i)
    sent = np.fromiter(where.keys(), dtype=np.int64, count=len(where))
    out = []
    for boundary in boundaries:
        hits = np.intersect1d(np.asarray(sorted(boundary), dtype=np.int64), sent)  # sorted, unique
        rows = [sources[where[int(n)][0]][1][where[int(n)][1]] for n in hits]
        out.append(([int(n) for n in hits], np.stack(rows) if rows else None))
    return out


def route_round(arrivals):
    """``route`` over a round in the golden cases' form [(worker, feature | None, ids, boundary)]:
    {worker: (id tuple, raw rows | None)} in arrival order."""
    sources = [(ids, as_bytes(feature)) for _, feature, ids, _ in arrivals if feature is not None]
    res = route(sources, [b for _, _, _, b in arrivals])
    return {w: (tuple(ids), rows) for (w, _, _, _), (ids, rows) in zip(arrivals, res)}
