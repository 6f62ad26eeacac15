"""Shared by the graph tests: the golden cases (tests/golden/graph_golden.npz, generated from the
reference's own classes by tests/golden/gen_graph_golden.py) as rounds of messages, byte
comparison and random embedding rounds."""

from __future__ import annotations

import functools
import json
from pathlib import Path
from typing import Any

import numpy as np
import torch

from distributed_learning_simulation_lib_amd import FeatureMessage, Message, ParameterMessage

GOLDEN = Path(__file__).resolve().parent / "golden"
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "float64": torch.float64}


def _tensor(a: np.ndarray, dtype: torch.dtype, shape) -> torch.Tensor:
    """A copy of ``a`` as ``dtype``; 16-bit values are stored as their bits."""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype).reshape(shape)
    return torch.from_numpy(a.copy()).reshape(shape)


@functools.lru_cache(maxsize=None)
def golden_cases() -> dict[str, dict]:
    """name -> dict(composite, rounds=[dict(kind, arrivals, out)]). Loaded once, left unchanged.

    embedding: arrivals = [(worker, feature | None, node index list | None, sorted boundary list)],
    out = [(worker, node index tuple, feature | None)] in the reference's answer order.
    topology: arrivals = out = [(worker, sorted node list)]. fedavg: arrivals = [(worker, {name:
    tensor}, weight)], out = {name: float64 tensor}."""
    manifest = json.loads((GOLDEN / "graph_manifest.json").read_text())
    cases = {}
    with np.load(GOLDEN / "graph_golden.npz") as f:
        for c in manifest["cases"]:
            rounds = []
            for r, rec in enumerate(c["rounds"]):
                key, kind = f"{c['name']}/{r}", rec["kind"]
                if kind == "topology":
                    arrivals = [(a["worker_id"], a["training_node_indices"]) for a in rec["arrivals"]]
                    out = [(o["worker_id"], o["training_node_indices"]) for o in rec["out"]]
                elif kind == "embedding":
                    arrivals, out = [], []
                    for j, a in enumerate(rec["arrivals"]):
                        feature = ids = None
                        if a["feature"]:
                            feature = _tensor(f[f"{key}/in/{j}/feature"], DTYPES[a["dtype"]], a["shape"])
                            ids = [int(x) for x in f[f"{key}/in/{j}/node_indices"]]
                        arrivals.append((a["worker_id"], feature, ids, a["boundary"]))
                    for j, o in enumerate(rec["out"]):
                        feature = None
                        if o["feature"]:
                            feature = _tensor(f[f"{key}/out/{j}/feature"], DTYPES[o["dtype"]], o["shape"])
                        out.append((o["worker_id"], tuple(int(x) for x in f[f"{key}/out/{j}/node_indices"]), feature))
                else:
                    arrivals = [(a["worker_id"],
                                 {n: _tensor(f[f"{key}/in/{j}/{n}"], torch.float32, s) for n, s in zip(a["names"], a["shapes"])},
                                 a["weight"]) for j, a in enumerate(rec["arrivals"])]
                    out = {n: _tensor(f[f"{key}/out/{n}"], torch.float64, s)
                           for n, s in zip(rec["out"]["names"], rec["out"]["shapes"])}
                rounds.append(dict(kind=kind, arrivals=arrivals, out=out))
            cases[c["name"]] = dict(composite=c["composite"], rounds=rounds)
    return cases


EMBEDDING_CASES = ["f32_row64_n4", "f16_row3_n2", "bf16_row257_n3", "f64_row1_n5", "f32_row257_n9", "f16_row64_n6",
                   "bf16_row1_n7", "f64_row3_n8", "f32_scalar_rows", "f32_matrix_rows", "silent_worker", "stranger",
                   "silent_and_stranger", "nobody_sends", "two_rounds"]


def raw_bytes(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy()


def assert_same_bytes(got: torch.Tensor, want: torch.Tensor, what="") -> None:
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype,
                                                                               tuple(got.shape), tuple(want.shape))
    assert np.array_equal(raw_bytes(got), raw_bytes(want)), f"{what}: the bytes differ"


def feature_message(feature, ids, boundary, feature_cls=FeatureMessage, device=None, tensor_boundary=False):
    """One arrival of an embedding round as a fresh message (the algorithms pop its other_data)."""
    other: dict[str, Any] = {}
    if feature is not None:
        other["node_indices"] = list(ids)
        feature = feature.clone() if device is None else feature.to(device)
    if tensor_boundary:
        b = torch.tensor(sorted(boundary), dtype=torch.int64)
        other["boundary"] = b if device is None else b.to(device)
    else:
        other["boundary"] = set(boundary)
    return feature_cls(feature=feature, other_data=other, in_round=True)


def run_embedding_round(algo, arrivals, **kw):
    for w, feature, ids, boundary in arrivals:
        assert algo.process_worker_data(worker_id=w, worker_data=feature_message(feature, ids, boundary, **kw))
    res = algo.aggregate_worker_data()
    algo.clear_worker_data()
    return res


def check_embedding_result(res, want, message_cls=None, feature_cls=None, device_type="cpu", what="") -> None:
    """``res`` against the reference's answer ``want`` = [(worker, node index tuple, feature | None)]."""
    assert res.in_round and not res.end_training
    if message_cls is not None:
        assert type(res) is message_cls
    assert list(res.worker_data) == [w for w, _, _ in want], what  # the reference's worker order
    for (w, ids, feature), m in zip(want, res.worker_data.values()):
        if feature_cls is not None:
            assert type(m) is feature_cls
        assert m.in_round and list(m.other_data) == ["node_indices"]
        got_ids = m.other_data["node_indices"]
        assert type(got_ids) is tuple and all(type(i) is int for i in got_ids)
        assert got_ids == ids, (what, w)
        if feature is None:
            assert m.feature is None, (what, w)
        else:
            assert m.feature is not None and m.feature.device.type == device_type, (what, w)
            assert_same_bytes(m.feature, feature, f"{what} worker {w}")


def topology_message(nodes, message_cls=Message):
    return message_cls(other_data={"training_node_indices": set(nodes)}, in_round=True)


def parameter_message(params, weight):
    return ParameterMessage(parameter={k: v.clone() for k, v in params.items()}, aggregation_weight=weight)


def random_round(seed: int, n_workers: int, dtype: torch.dtype, row_shape: tuple[int, ...], nodes: int,
                 owned: int, wanted: int):
    """A random embedding round in the golden cases' form: disjoint owned node sets of ``owned`` ids,
    boundaries of ``wanted`` ids drawn from twice the owned range (about half of them hit)."""
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    perm = rng.permutation(nodes)
    arrivals = []
    for w in rng.permutation(n_workers):
        ids = perm[w * owned: (w + 1) * owned]
        feature = torch.randn((owned,) + tuple(row_shape), generator=gen, dtype=torch.float32).to(dtype)
        boundary = rng.choice(2 * n_workers * owned, size=wanted, replace=False)
        arrivals.append((int(w), feature, [int(x) for x in ids], sorted(int(x) for x in boundary)))
    return arrivals
