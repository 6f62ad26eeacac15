"""Generate the golden fixtures of the sparse delta fold from the REFERENCE's own code.

A sparse delta is a ``DeltaParameterMessage`` whose missing entries are +0.0, so the expected result
of every case is what the reference's ``DeltaParameterMessage.restore`` (message.py:40-61) followed by
its ``FedAVGAlgorithm`` (fed_avg_algorithm.py:43-99) gives on the densified deltas. The reference is
loaded through ``gen_golden._load_reference`` (the same three unmodified files behind the same
stubs); nothing of it is copied. A no-op where the reference is absent.

Output: tests/golden/sparse_golden.npz (inputs as indices and values, expected float64 outputs) and
tests/golden/sparse_manifest.json. The file holds one pool per number format ("f64": bases, expected
outputs and float64 values; "i32": indices; "f32"; "u16": the bits of float16 / bfloat16 values),
each the concatenation of its arrays in a fixed order: case by case the bases in name order, then
arrival by arrival and name by name the indices and the values, then the expected outputs. The
manifest holds the shapes and, per arrival and name, the number of entries (null: a dense tensor),
which is all a reader needs to cut the pools up again (tests/sparse_cases.py does).
Re-run: `python tests/golden/gen_sparse_golden.py`.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

OUT_DIR = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT_DIR))
import gen_golden  # noqa: E402  (the loader of the reference and its stubs)

SHAPES = {"a": (11,), "b": (3, 5), "s": (), "c": (13,)}
POOL_OF = {torch.float32: "f32", torch.float16: "u16", torch.bfloat16: "u16", torch.float64: "f64"}


def _values(gen, n, dtype):
    return (torch.randn(n, generator=gen, dtype=torch.float32) * 0.05).to(dtype)


def _sparse(gen, shape, dtype, density):
    numel = int(np.prod(shape, dtype=np.int64))
    k = min(numel, max(1, round(density * numel)))
    idx = torch.sort(torch.randperm(numel, generator=gen)[:k]).values
    return {"kind": "sparse", "indices": idx, "values": _values(gen, k, dtype)}


def build_cases():
    """Each case: name, dtype, old (float64 base), arrivals = [(worker id, weight, {name: entry} or
    None)], entry = {"kind": "sparse", indices, values} or {"kind": "dense", tensor}."""
    cases = []

    def add(name, dtype, weights, seed, density=0.2, shapes=SHAPES):
        gen = torch.Generator().manual_seed(seed)
        old = {n: torch.randn(s, generator=gen, dtype=torch.float64) for n, s in shapes.items()}
        arrivals = [(wid, w, {n: _sparse(gen, s, dtype, density) for n, s in shapes.items()})
                    for wid, w in enumerate(weights)]
        cases.append(dict(name=name, dtype=dtype, shapes=shapes, old=old, arrivals=arrivals))
        return cases[-1]

    add("f32_int", torch.float32, [120, 4000, 33], 1)
    add("f16_frac", torch.float16, [0.1, 0.7, 1 / 3, 2.2], 2)
    add("bf16_int", torch.bfloat16, [7, 2, 9, 4, 11], 3)
    add("f64_frac", torch.float64, [2.5, 1e-3, 3.25], 4)
    add("one_client", torch.float32, [250], 5)
    add("nine_clients", torch.float32, [float(x) for x in np.random.default_rng(6).uniform(0.1, 10.0, 9)], 6, 0.05)

    c = add("skipped", torch.float32, [1, 3, 2, 5], 7)
    c["arrivals"][1] = (1, None, None)

    c = add("empty_client", torch.float32, [3, 5, 7], 8)
    for entry in c["arrivals"][1][2].values():
        entry["indices"], entry["values"] = entry["indices"][:0], entry["values"][:0]

    # -0.0 in the base without an entry (+0.0 comes out), under a -0.0 entry of every client (-0.0
    # comes out) and under a -0.0 entry of one client only
    c = add("signed_zero", torch.float32, [2, 3], 9, shapes={"z": (16,)})
    c["old"]["z"][:6] = -0.0
    for j, (_, _, entries) in enumerate(c["arrivals"]):
        idx = [2, 3, 9] if j == 0 else [2, 4, 9]
        entries["z"]["indices"] = torch.tensor(idx)
        entries["z"]["values"] = torch.tensor([-0.0, -0.0, 0.25 * (j + 1)], dtype=torch.float32)

    # a dense tensor among sparse ones: it counts as all-present
    c = add("dense_among_sparse", torch.float32, [5, 1, 4], 10)
    gen = torch.Generator().manual_seed(100)
    for _, _, entries in c["arrivals"][:2]:
        entries["b"] = {"kind": "dense", "tensor": _values(gen, 15, torch.float32).view(SHAPES["b"])}
    return cases


def densify(entry, shape, dtype):
    if entry["kind"] == "dense":
        return entry["tensor"].clone()
    flat = torch.zeros(int(np.prod(shape, dtype=np.int64)), dtype=dtype)
    flat[entry["indices"]] = entry["values"]
    return flat.view(shape)


def run_reference(case, message, fed):
    algo = fed.FedAVGAlgorithm()
    for wid, weight, entries in case["arrivals"]:
        if entries is None:
            algo.process_worker_data(worker_id=wid, worker_data=None)
            continue
        delta = {n: densify(e, case["shapes"][n], case["dtype"]) for n, e in entries.items()}
        msg = message.DeltaParameterMessage(delta_parameter=delta, aggregation_weight=weight)
        # AggregationServer._process_worker_data: data = data.restore(old_parameter)
        algo.process_worker_data(worker_id=wid, worker_data=msg.restore({k: v.clone() for k, v in case["old"].items()}))
    return algo.aggregate_worker_data()


def main() -> int:
    if not gen_golden.REF.exists():
        print("reference not present: nothing to generate")
        return 0
    message, _agg, fed = gen_golden._load_reference()
    pools: dict[str, list[np.ndarray]] = {"f64": [], "i32": [], "f32": [], "u16": []}

    def put(pool: str, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a).reshape(-1)
        if pool == "u16":
            a = a.view(np.uint16)
        assert a.dtype == {"f64": np.float64, "i32": np.int32, "f32": np.float32, "u16": np.uint16}[pool]
        pools[pool].append(a)

    manifest = {"generator": "tests/golden/gen_sparse_golden.py",
                "reference_files": ["simulation_lib/message.py", "simulation_lib/algorithm/aggregation_algorithm.py",
                                    "simulation_lib/algorithm/fed_avg_algorithm.py"],
                "cases": []}
    for case in build_cases():
        name, vpool, names = case["name"], POOL_OF[case["dtype"]], list(case["shapes"])
        entry = {"name": name, "dtype": str(case["dtype"]).replace("torch.", ""), "names": names,
                 "shapes": [list(s) for s in case["shapes"].values()], "arrivals": []}
        for k in names:
            put("f64", case["old"][k].numpy())
        for wid, weight, entries in case["arrivals"]:
            a = {"worker_id": wid, "weight": weight, "nnz": None}
            if entries is not None:
                assert list(entries) == names
                a["nnz"] = []
                for e in entries.values():
                    if e["kind"] == "dense":
                        a["nnz"].append(None)
                        put(vpool, gen_golden._np(e["tensor"]))
                    else:
                        a["nnz"].append(int(e["indices"].numel()))
                        put("i32", e["indices"].numpy().astype(np.int32))
                        put(vpool, gen_golden._np(e["values"]))
            entry["arrivals"].append(a)
        res = run_reference(case, message, fed)
        assert list(res.parameter) == names
        for v in res.parameter.values():
            assert v.dtype == torch.float64
            put("f64", v.numpy())
        manifest["cases"].append(entry)
        print(f"{name}: ok")
    np.savez_compressed(OUT_DIR / "sparse_golden.npz", **{k: np.concatenate(v) for k, v in pools.items()})
    (OUT_DIR / "sparse_manifest.json").write_text(json.dumps(manifest, separators=(",", ":")) + "\n")
    print(f"wrote {len(manifest['cases'])} cases, {(OUT_DIR / 'sparse_golden.npz').stat().st_size / 1e3:.1f} kB")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
