"""Generate the golden fixtures of the graph algorithms from the REFERENCE's own code.

The reference's four server-side graph classes are loaded unmodified —
  simulation_lib/algorithm/composite_aggregation_algorithm.py, graph_topology_algorithm.py,
  graph_embedding_algorithm.py, graph_algorithm.py
— on top of the three files and the stubs of ``gen_golden._load_reference``; nothing of them is
copied. A no-op where the reference is absent.

Every case is a sequence of rounds driven the way the reference's server drives an algorithm
(process_worker_data per arrival, aggregate_worker_data, clear_worker_data). An "embedding" round
records, per arrival, the worker id, the feature (or none), its node indices and the boundary, and
per worker of the reference's answer — in the answer's own order — the node-index tuple and the
stacked feature (or none). A "topology" round records what every worker sent; a "fedavg" round the
parameters, weights and the reference's float64 result. The embedding cases run the reference's
GraphNodeEmbeddingPassingAlgorithm alone; the case "graph_sequence" runs its GraphAlgorithm through
a topology round, two embedding rounds and a FedAvg round.

Output: tests/golden/graph_golden.npz (arrays by key; float16 / bfloat16 as their bits) and
tests/golden/graph_manifest.json (everything else). tests/graph_cases.py reads them.
Re-run: `python tests/golden/gen_graph_golden.py`.
"""

from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

OUT_DIR = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT_DIR))
import gen_golden  # noqa: E402  (the loader of the reference and its stubs)

NODES = 300  # node ids of the graph; ids from NODES up are owned by nobody


def embedding_round(seed, n_workers, dtype, row_shape, silent=(), strangers=(), order=None, everybody_silent=False):
    """One round's arrivals: [(worker id, feature | None, node indices | None, boundary set)].

    The workers own disjoint random node sets. A worker of ``silent`` sends ``feature=None`` (its
    nodes are then nobody's), one of ``strangers`` wants only ids nobody owns; every other boundary
    mixes foreign owned ids, ids of silent workers and ids past the graph."""
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    perm = rng.permutation(NODES)
    sizes = rng.integers(4, 16, size=n_workers)
    owned, pos = [], 0
    for s in sizes:
        owned.append(np.sort(perm[pos: pos + s]))
        pos += s
    free = perm[pos:]
    arrivals = []
    for w in (order if order is not None else range(n_workers)):
        if w in strangers:
            boundary = set(int(x) for x in rng.choice(free, size=7, replace=False)) | {NODES + 5, NODES + 4000}
        else:
            foreign = np.concatenate([owned[v] for v in range(n_workers) if v != w])
            take = rng.choice(foreign, size=min(len(foreign), int(rng.integers(3, 40))), replace=False)
            boundary = set(int(x) for x in take) | set(int(x) for x in rng.choice(free, size=3, replace=False))
            boundary |= {NODES + 17 + w}
        if w in silent or everybody_silent:
            arrivals.append((w, None, None, boundary))
            continue
        ids = rng.permutation(owned[w])  # node indices need no order
        feature = torch.randn((len(ids),) + tuple(row_shape), generator=gen, dtype=torch.float32).to(dtype)
        arrivals.append((w, feature, [int(x) for x in ids], boundary))
    return arrivals


def build_cases():
    f32, f16, bf16, f64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
    cases = []

    def emb(name, *args, **kw):
        cases.append({"name": name, "rounds": [("embedding", embedding_round(*args, **kw))]})

    emb("f32_row64_n4", 1, 4, f32, (64,))
    emb("f16_row3_n2", 2, 2, f16, (3,))
    emb("bf16_row257_n3", 3, 3, bf16, (257,))
    emb("f64_row1_n5", 4, 5, f64, (1,))
    emb("f32_row257_n9", 5, 9, f32, (257,), order=[8, 3, 0, 5, 1, 7, 2, 6, 4])
    emb("f16_row64_n6", 6, 6, f16, (64,), order=[5, 4, 3, 2, 1, 0])
    emb("bf16_row1_n7", 7, 7, bf16, (1,))
    emb("f64_row3_n8", 8, 8, f64, (3,), order=[2, 0, 1, 7, 6, 5, 4, 3])
    emb("f32_scalar_rows", 9, 3, f32, ())
    emb("f32_matrix_rows", 10, 4, f32, (3, 5))
    emb("silent_worker", 11, 5, f32, (64,), silent=(2,), order=[4, 2, 0, 3, 1])
    emb("stranger", 12, 4, f16, (3,), strangers=(1,))
    emb("silent_and_stranger", 13, 6, bf16, (64,), silent=(0, 3), strangers=(5,), order=[3, 5, 1, 0, 4, 2])
    emb("nobody_sends", 14, 3, f32, (64,), everybody_silent=True)
    # two rounds on one object, the second with other workers and another row length
    cases.append({"name": "two_rounds", "rounds": [("embedding", embedding_round(15, 4, f32, (64,))),
                                                    ("embedding", embedding_round(16, 6, f32, (3,), order=[1, 0, 5, 4, 3, 2]))]})

    # the composite: a topology round, two embedding rounds, then a FedAvg round
    rng = np.random.default_rng(20)
    topology = [(w, set(int(x) for x in rng.choice(NODES, size=12, replace=False))) for w in (2, 0, 1)]
    shapes = {"conv.weight": (4, 3), "conv.bias": (4,), "lin.weight": (33,)}
    fedavg = [(w, gen_golden._model(shapes, f32, 200 + w), weight) for w, weight in ((1, 120), (0, 4000), (2, 33))]
    cases.append({"name": "graph_sequence", "composite": True,
                  "rounds": [("topology", topology),
                             ("embedding", embedding_round(21, 3, f32, (64,), order=[2, 0, 1])),
                             ("embedding", embedding_round(22, 3, f32, (64,), silent=(1,), order=[1, 2, 0])),
                             ("fedavg", fedavg)]})
    return cases


def main() -> int:
    if not gen_golden.REF.exists():
        print("reference not present: nothing to generate")
        return 0
    message, _agg, _fed = gen_golden._load_reference()
    emb_mod = importlib.import_module("simulation_lib.algorithm.graph_embedding_algorithm")
    importlib.import_module("simulation_lib.algorithm.composite_aggregation_algorithm")
    importlib.import_module("simulation_lib.algorithm.graph_topology_algorithm")
    graph_mod = importlib.import_module("simulation_lib.algorithm.graph_algorithm")

    arrays: dict[str, np.ndarray] = {}
    manifest = {"generator": "tests/golden/gen_graph_golden.py",
                "reference_files": ["simulation_lib/message.py", "simulation_lib/algorithm/aggregation_algorithm.py",
                                    "simulation_lib/algorithm/fed_avg_algorithm.py",
                                    "simulation_lib/algorithm/composite_aggregation_algorithm.py",
                                    "simulation_lib/algorithm/graph_topology_algorithm.py",
                                    "simulation_lib/algorithm/graph_embedding_algorithm.py",
                                    "simulation_lib/algorithm/graph_algorithm.py"],
                "cases": []}
    for case in build_cases():
        name = case["name"]
        algo = graph_mod.GraphAlgorithm() if case.get("composite") else emb_mod.GraphNodeEmbeddingPassingAlgorithm()
        entry = {"name": name, "composite": bool(case.get("composite")), "rounds": []}
        for r, (kind, arrivals) in enumerate(case["rounds"]):
            key = f"{name}/{r}"
            rec = {"kind": kind, "arrivals": [], "out": []}
            if kind == "topology":
                for w, nodes in arrivals:
                    rec["arrivals"].append({"worker_id": w, "training_node_indices": sorted(nodes)})
                    assert algo.process_worker_data(
                        worker_id=w, worker_data=message.Message(other_data={"training_node_indices": set(nodes)},
                                                                 in_round=True))
                res = algo.aggregate_worker_data()
                assert type(res) is message.Message and res.in_round
                rec["out"] = [{"worker_id": w, "training_node_indices": sorted(v)}
                              for w, v in res.other_data["training_node_indices"].items()]
            elif kind == "embedding":
                for j, (w, feature, ids, boundary) in enumerate(arrivals):
                    a = {"worker_id": w, "boundary": sorted(boundary), "feature": feature is not None}
                    other = {"boundary": set(boundary)}
                    if feature is not None:
                        a["dtype"] = str(feature.dtype).replace("torch.", "")
                        a["shape"] = list(feature.shape)
                        arrays[f"{key}/in/{j}/feature"] = gen_golden._np(feature)
                        arrays[f"{key}/in/{j}/node_indices"] = np.asarray(ids, dtype=np.int64)
                        other["node_indices"] = list(ids)
                    rec["arrivals"].append(a)
                    assert algo.process_worker_data(
                        worker_id=w, worker_data=message.FeatureMessage(
                            feature=None if feature is None else feature.clone(), other_data=other, in_round=True))
                res = algo.aggregate_worker_data()
                assert type(res) is message.MultipleWorkerMessage and res.in_round
                for j, (w, m) in enumerate(res.worker_data.items()):
                    assert type(m) is message.FeatureMessage and m.in_round and list(m.other_data) == ["node_indices"]
                    o = {"worker_id": w, "feature": m.feature is not None}
                    arrays[f"{key}/out/{j}/node_indices"] = np.asarray(m.other_data["node_indices"], dtype=np.int64)
                    if m.feature is not None:
                        o["dtype"] = str(m.feature.dtype).replace("torch.", "")
                        o["shape"] = list(m.feature.shape)
                        arrays[f"{key}/out/{j}/feature"] = gen_golden._np(m.feature)
                    rec["out"].append(o)
            else:
                for j, (w, params, weight) in enumerate(arrivals):
                    rec["arrivals"].append({"worker_id": w, "weight": weight, "names": list(params),
                                            "shapes": [list(v.shape) for v in params.values()]})
                    for k, v in params.items():
                        arrays[f"{key}/in/{j}/{k}"] = gen_golden._np(v)
                    assert algo.process_worker_data(
                        worker_id=w, worker_data=message.ParameterMessage(
                            parameter={k: v.clone() for k, v in params.items()}, aggregation_weight=weight))
                res = algo.aggregate_worker_data()
                assert type(res) is message.ParameterMessage
                rec["out"] = {"names": list(res.parameter), "shapes": [list(v.shape) for v in res.parameter.values()]}
                for k, v in res.parameter.items():
                    assert v.dtype == torch.float64
                    arrays[f"{key}/out/{k}"] = v.numpy()
            algo.clear_worker_data()
            entry["rounds"].append(rec)
        manifest["cases"].append(entry)
        print(f"{name}: ok")
    np.savez_compressed(OUT_DIR / "graph_golden.npz", **arrays)
    (OUT_DIR / "graph_manifest.json").write_text(json.dumps(manifest, separators=(",", ":")) + "\n")
    print(f"wrote {len(manifest['cases'])} cases, {(OUT_DIR / 'graph_golden.npz').stat().st_size / 1e3:.1f} kB")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
