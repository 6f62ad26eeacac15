"""Time the graph embedding exchange on the GPU and write profiles/graph_lines.jsonl.

Per shape (workers x sent rows per worker x row length x dtype, every worker wanting `want` ids of
which about half hit), in one process on one GPU:

* ``aggregate``: the whole ``GraphNodeEmbeddingPassingAlgorithm.aggregate_worker_data`` with the
  round staged (features on the GPU), boundaries as sorted device tensors (the fast path) and as
  host sets (what the reference sends; the sorted host arrays are uploaded inside the call);
* ``route_rows``: the ``fedavg_route_rows`` call alone on prebuilt device arrays — host clock around
  the call and a synchronise, and device events around the call's work on the stream;
* ``torch_composition``: what a user would write in torch: ``cat`` of the features, a dense lookup
  table by ``index_put_``, per worker a lookup, a mask and ``index_select``;
* ``reference_loop``: the reference's rule restated with its per-row Python loop (a dict, per worker
  a set intersection, ``torch.stack`` of one ``.cpu()`` row at a time).

Every timing is a host clock around work that ends in a device synchronise (or device events where
it says so), after warm-up of the same shape; the line holds the median, the 10th and 90th
percentile and the repetitions. The outputs of the four ways are compared once per shape.

    python scripts/graph_bench.py [--out profiles/graph_lines.jsonl] [--quick]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distributed_learning_simulation_lib_amd import FeatureMessage, GraphNodeEmbeddingPassingAlgorithm  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import RowRouter  # noqa: E402

SHAPES = [  # (name, workers, rows per worker, row length, dtype, wanted ids per worker)
    ("w64_r2048_d64_f32", 64, 2048, 64, torch.float32, 8192),
    ("w64_r2048_d64_f16", 64, 2048, 64, torch.float16, 8192),
    ("w64_r2048_d256_f32", 64, 2048, 256, torch.float32, 8192),
    ("w64_r2048_d256_f16", 64, 2048, 256, torch.float16, 8192),
    ("w8_r256_d64_f32", 8, 256, 64, torch.float32, 1024),  # one in-round exchange of a small graph
]


def make_round(seed, workers, rows, dim, dtype, want, device):
    rng = np.random.default_rng(seed)
    owned = rng.permutation(workers * rows).reshape(workers, rows)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    features = [torch.randn(rows, dim, generator=gen).to(dtype).to(device) for _ in range(workers)]
    # ids from twice the owned range: about half of a boundary hits
    boundaries = [np.sort(rng.choice(2 * workers * rows, size=want, replace=False)) for _ in range(workers)]
    return owned, features, boundaries


def timed(fn, reps, warmup, device):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(device)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(device)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "reps": len(ms)}


def stage(algo, owned, features, boundaries, device, on_device):
    algo.clear_worker_data()
    for w, f in enumerate(features):
        b = torch.from_numpy(boundaries[w]).to(device) if on_device else set(boundaries[w].tolist())
        algo.process_worker_data(w, FeatureMessage(feature=f, other_data={"node_indices": owned[w], "boundary": b},
                                                   in_round=True))


def torch_composition(features, src_ids, dev_boundaries, node_space, device):
    cat = torch.cat(features)
    table = torch.full((node_space,), -1, dtype=torch.int64, device=device)
    table.index_put_((src_ids,), torch.arange(src_ids.numel(), device=device))
    out = []
    for b in dev_boundaries:
        r = table[b]
        hit = r >= 0
        out.append((b[hit], cat.index_select(0, r[hit])))
    return out


def reference_loop(features, owned, boundaries):
    where = {}
    for s, ids in enumerate(owned):
        for i, node in enumerate(ids.tolist()):
            assert node not in where
            where[node] = (s, i)
    keys = set(where)
    out = []
    for b in boundaries:
        ids = tuple(sorted(set(b.tolist()) & keys))
        rows = torch.stack([features[where[n][0]][where[n][1]].cpu() for n in ids]) if ids else None
        out.append((ids, rows))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "graph_lines.jsonl"))
    ap.add_argument("--quick", action="store_true", help="the small shape only, few repetitions (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_bench.py measures on a GPU: none is visible")
    device = torch.device("cuda", 0)
    lines = []
    for seed, (name, workers, rows, dim, dtype, want) in enumerate(SHAPES[-1:] if args.quick else SHAPES):
        owned, features, boundaries = make_round(seed, workers, rows, dim, dtype, want, device)
        big = workers * rows > 10000
        reps, warm = (10, 2) if args.quick else (30, 5) if big else (200, 20)
        node_space = 2 * workers * rows  # the torch table covers every wanted id
        src_ids = torch.from_numpy(owned.reshape(-1)).to(device)
        dev_boundaries = [torch.from_numpy(b).to(device) for b in boundaries]
        base = {"shape": name, "workers": workers, "rows_per_worker": rows, "row_len": dim,
                "dtype": str(dtype).replace("torch.", ""), "want_per_worker": want,
                "device": torch.cuda.get_device_name(device)}

        algo = GraphNodeEmbeddingPassingAlgorithm(device=device)
        results = {}
        for label, on_device in (("aggregate_device_boundaries", True), ("aggregate_host_boundaries", False)):
            stage(algo, owned, features, boundaries, device, on_device)
            results[label] = algo.aggregate_worker_data()
            lines.append({**base, "what": label, **stats(timed(algo.aggregate_worker_data, reps, warm, device))})
        algo.exit()

        # the ABI call alone
        router = RowRouter(device)
        want_ids = torch.cat(dev_boundaries)
        want_off = np.arange(workers + 1, dtype=np.int64) * want
        B = workers * want
        out_rows = torch.empty(B, dim, dtype=dtype, device=device)
        out_ids = torch.empty(B, dtype=torch.int64, device=device)
        out_count = torch.empty(workers, dtype=torch.int32, device=device)
        row_bytes = dim * features[0].element_size()

        def call():
            router.route_rows(features, src_ids, want_ids, want_off, workers * rows, out_rows, out_ids, out_count,
                              row_bytes, features[0].element_size())

        lines.append({**base, "what": "route_rows_call", **stats(timed(call, reps, warm, device))})
        ev = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize(device)
            ev.append(e0.elapsed_time(e1))
        assert router.errors() == 0
        hit_rows = int(out_count.sum())
        lines.append({**base, "what": "route_rows_device_events", **stats(ev), "hit_rows": hit_rows,
                      "bytes_moved": 2 * hit_rows * row_bytes})
        router.close()

        lines.append({**base, "what": "torch_composition", **stats(timed(
            lambda: torch_composition(features, src_ids, dev_boundaries, node_space, device), reps, warm, device))})
        ref_reps, ref_warm = (2, 0) if big else (20, 2)
        lines.append({**base, "what": "reference_loop", **stats(timed(
            lambda: reference_loop(features, owned, boundaries), ref_reps, ref_warm, device))})

        # the four ways give the same answer
        comp = torch_composition(features, src_ids, dev_boundaries, node_space, device)
        loop = reference_loop(features, owned, boundaries) if not big else None
        for label, res in results.items():
            for w, (ids, rws) in enumerate(comp):
                m = res.worker_data[w]
                assert m.other_data["node_indices"] == tuple(ids.tolist()), (name, label, w)
                assert torch.equal(m.feature, rws), (name, label, w)
                if loop is not None:
                    assert loop[w][0] == m.other_data["node_indices"] and torch.equal(loop[w][1], m.feature.cpu())
        for line in lines[-6:]:
            print(json.dumps(line), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(line) + "\n" for line in lines))
    print(f"wrote {len(lines)} lines to {out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
