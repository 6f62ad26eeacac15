"""Shared by the sparse tests: the golden cases (tests/golden/sparse_golden.npz, generated from the
reference by tests/golden/gen_sparse_golden.py) as messages, bit comparison, random sparse deltas."""

from __future__ import annotations

import functools
import json
import math
from pathlib import Path

import numpy as np
import torch

from distributed_learning_simulation_lib_amd import DeltaParameterMessage, SparseDelta

GOLDEN = Path(__file__).resolve().parent / "golden"
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "float64": torch.float64}


POOL_OF = {torch.float32: "f32", torch.float16: "u16", torch.bfloat16: "u16", torch.float64: "f64"}


def _tensor(a: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """A copy of ``a`` as ``dtype``; 16-bit values are stored as their bits."""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


@functools.lru_cache(maxsize=None)
def golden_cases() -> dict[str, dict]:
    """name -> dict(dtype, names, shapes, old, arrivals=[(worker id, weight, {name: SparseDelta |
    tensor} | None)], out={name: float64 array}). Loaded once, left unchanged. The file holds one
    pool per number format, written in the order in which this function reads it (the generator's
    docstring states it); the manifest holds the shapes and the entry counts (null: dense)."""
    manifest = json.loads((GOLDEN / "sparse_manifest.json").read_text())
    with np.load(GOLDEN / "sparse_golden.npz") as f:
        pools = {k: f[k] for k in f.files}
    at = dict.fromkeys(pools, 0)

    def take(pool: str, count: int) -> np.ndarray:
        at[pool] += count
        assert at[pool] <= pools[pool].size
        return pools[pool][at[pool] - count:at[pool]]

    cases = {}
    for c in manifest["cases"]:
        name, dtype = c["name"], DTYPES[c["dtype"]]
        vpool = POOL_OF[dtype]
        shapes = {n: tuple(s) for n, s in zip(c["names"], c["shapes"])}
        numel = {n: math.prod(s) for n, s in shapes.items()}
        old = {n: torch.from_numpy(take("f64", numel[n]).copy()).view(shapes[n]) for n in shapes}
        arrivals = []
        for a in c["arrivals"]:
            if a["nnz"] is None:
                arrivals.append((a["worker_id"], None, None))
                continue
            entries = {}
            for n, k in zip(shapes, a["nnz"]):
                if k is None:
                    entries[n] = _tensor(take(vpool, numel[n]), dtype).view(shapes[n])
                else:
                    idx = torch.from_numpy(take("i32", k).copy())
                    entries[n] = SparseDelta(idx, _tensor(take(vpool, k), dtype), shapes[n])
            arrivals.append((a["worker_id"], a["weight"], entries))
        cases[name] = dict(dtype=dtype, names=list(shapes), shapes=shapes, old=old, arrivals=arrivals,
                           out={n: take("f64", numel[n]).reshape(shapes[n]) for n in shapes})
    assert all(at[k] == pools[k].size for k in pools), "the golden pools were not read to their ends"
    return cases


CASES = ["f32_int", "f16_frac", "bf16_int", "f64_frac", "one_client", "nine_clients", "skipped", "empty_client",
         "signed_zero", "dense_among_sparse"]


def run_round(algo, case):
    algo.set_old_parameter(case["old"])
    for wid, msg in messages(case):
        algo.process_worker_data(wid, msg)
    return algo.aggregate_worker_data()


def messages(case) -> list[tuple[int, DeltaParameterMessage | None]]:
    return [(wid, None if entries is None else DeltaParameterMessage(delta_parameter=dict(entries), aggregation_weight=w))
            for wid, w, entries in case["arrivals"]]


def reference_rows(case):
    """The case for tests/sparse_reference.fold: rows of (indices, values), weights, base."""
    rows, weights = [], []
    for _, w, entries in case["arrivals"]:
        if entries is None:
            continue
        row = []
        for n in case["names"]:
            e = entries[n]
            row.append((e.indices, e.values) if isinstance(e, SparseDelta)
                       else (np.arange(e.numel()), e.reshape(-1)))
        rows.append(row)
        weights.append(w)
    return rows, weights, [case["old"][n] for n in case["names"]]


def bits(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def assert_same_bits(got, want, what="") -> None:
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if not np.array_equal(g, w):
        at = int(np.argwhere(g != w)[0][0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} elements differ in bits; first at {at}")


def random_sparse(gen: torch.Generator, numel: int, nnz: int, dtype: torch.dtype, scale: float = 0.05) -> SparseDelta:
    """``nnz`` uniformly placed strictly increasing indices with N(0, scale) values."""
    idx = torch.sort(torch.randperm(numel, generator=gen)[:nnz]).values.to(torch.int32)
    val = (torch.randn(nnz, generator=gen, dtype=torch.float64) * scale).to(dtype)
    return SparseDelta(idx, val, (numel,))
