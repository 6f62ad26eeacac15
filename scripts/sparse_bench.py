"""Time the sparse delta fold against the dense delta fold and against what a user does today.

For N clients (default 64) of a model (default the ResNet-18 layout) that each send, per tensor,
uniformly random strictly increasing indices at a given density with fp32 values, each density
times, in one process on one GPU, with HIP events, after warm-up, as the median over interleaved
repeats:

  (s) ``FedAvgContext.sparse_aggregate_delta`` on the (index, value) pairs (the index check kernel
      and the fold; the host wait for the index report is outside the timed region);
  (a) ``FedAvgContext.aggregate_delta`` on pre-densified tensors: the dense fold alone;
  (b) densify on the GPU — one ``zeros`` and one ``index_put`` per client and tensor — then (a):
      what a user of the package does today.

Events around one asynchronous call on an idle stream span the call's host work as well (the first
event is reached at once, the second only after everything the call enqueued), so (s) and (a) are
each measured in two more ways that take the two apart: the host time until the call returns
(``perf_counter``, no wait), and --chain calls back to back between one pair of events, divided by
their number, where the host work of one call hides behind the device work of the one before
(whichever of host and device is slower per call shows).

One JSON line per density goes to --out (default profiles/sparse_lines.jsonl): each time with its
spread, (s)/(a) and (s)/(b) for the single calls and (s)/(a) back to back, the bytes the sparse fold
reads, and after the last density a summary line with the lowest measured density at which (s) no
longer beats (a), single call and back to back. The three results are compared bit for bit before
anything is timed. There is no CPU fallback: no GPU, no number.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from bench import resnet18_layout  # noqa: E402
from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext, SparseDelta  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import SparseTable  # noqa: E402


def timed(fn, stream, calls: int = 1) -> tuple[float, float]:
    """(event ms per call, host ms per call until the call returned) of ``calls`` calls back to back."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / calls, host / calls


def spread(ts: list[float]) -> dict:
    m = statistics.median(ts)
    return {"median_ms": round(m, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "spread_over_median": round((max(ts) - min(ts)) / m, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--densify-repeats", type=int, default=3, help="repeats of the (host-bound) densify path")
    ap.add_argument("--chain", type=int, default=8, help="calls back to back between one pair of events")
    ap.add_argument("--densities", default="0.001,0.01,0.1,0.5")
    ap.add_argument("--out", default=str(REPO / "profiles" / "sparse_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("sparse_bench.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    N, P, T = args.clients, layout.total_numel, layout.num_segments
    stream = torch.cuda.current_stream(device)
    gen = torch.Generator(device=device).manual_seed(1)
    base = [torch.randn(n, dtype=torch.float64, device=device, generator=gen) for n in layout.numels]
    weights = [float(100 + 37 * (k % 11)) for k in range(N)]
    W = 0.0
    for w in weights:
        W = W + w
    ctx = FedAvgContext(layout, device)
    lines = []
    for density in (float(d) for d in args.densities.split(",")):
        rows, wide = [], []
        for _ in range(N):
            row, wrow = [], []
            for n in layout.numels:
                idx = torch.nonzero(torch.rand(n, device=device, generator=gen) < density).reshape(-1)
                val = torch.randn(idx.numel(), dtype=torch.float32, device=device, generator=gen) * 0.01
                row.append(SparseDelta(idx.to(torch.int32), val, (n,)))
                wrow.append(idx)                       # int64, as index_put takes them
            rows.append(row)
            wide.append(wrow)
        nnz = sum(d.nnz for row in rows for d in row)
        dense = [[d.to_dense() for d in row] for row in rows]
        table = ClientTable(T)
        for drow, w in zip(dense, weights):
            table.add_client(drow, [w] * T)
        out_s = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        out_a = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        out_b = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]

        staged = SparseTable(rows, layout, device)   # as the dense fold's ClientTable: built once

        def sparse_fold():
            ctx.sparse_aggregate_delta(staged, weights, W, base, out_s, torch.float64, check_indices=False)

        def dense_fold():
            ctx.aggregate_delta(table, torch.float32, base, out_a, torch.float64)

        def densify_then_fold():
            t = ClientTable(T)
            for row, wrow, w in zip(rows, wide, weights):
                drow = []
                for d, i in zip(row, wrow):
                    x = torch.zeros(d.numel, dtype=torch.float32, device=device)
                    x.index_put_((i,), d.values)
                    drow.append(x)
                t.add_client(drow, [w] * T)
            ctx.aggregate_delta(t, torch.float32, base, out_b, torch.float64)

        for _ in range(args.warmup):
            sparse_fold()
            dense_fold()
        densify_then_fold()
        assert not ctx.sparse_index_errors() and ctx.flags() == 0
        for s, a, b in zip(out_s, out_a, out_b):      # the same bits before anything is timed
            assert torch.equal(s.view(torch.int64), a.view(torch.int64))
            assert torch.equal(s.view(torch.int64), b.view(torch.int64))
        ts, ta, tb, hs, ha, cs, ca = [], [], [], [], [], [], []
        for r in range(args.repeats):                  # interleaved: all see the same machine state
            for fn, single, host, chain in ((sparse_fold, ts, hs, cs), (dense_fold, ta, ha, ca)):
                ms, host_ms = timed(fn, stream)
                single.append(ms)
                host.append(host_ms)
                chain.append(timed(fn, stream, args.chain)[0])
            if r < args.densify_repeats:
                tb.append(timed(densify_then_fold, stream)[0])
        assert not ctx.sparse_index_errors() and ctx.flags() == 0
        s, a, b = statistics.median(ts), statistics.median(ta), statistics.median(tb)
        read = nnz * (4 + 4) + nnz * 4 + 8 * P         # entries by the fold, indices again by the check, the base
        lines.append({
            "case": f"{N} x resnet18 fp32 values at density {density:g}, float64 base and output",
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P, "density": density,
            "entries": nnz, "measured_density": round(nnz / (N * P), 6),
            "sparse_fold": spread(ts), "dense_delta_fold": spread(ta), "densify_then_dense_fold": spread(tb),
            "sparse_over_dense": round(s / a, 3), "sparse_over_densify_then_dense": round(s / b, 4),
            "sparse_host_call": spread(hs), "dense_host_call": spread(ha),
            "sparse_back_to_back": spread(cs), "dense_back_to_back": spread(ca), "chain": args.chain,
            "sparse_over_dense_back_to_back": round(statistics.median(cs) / statistics.median(ca), 3),
            "sparse_bytes_read": read, "sparse_bytes_written": 8 * P,
            "dense_bytes_read": N * P * 4 + 8 * P, "densify_bytes_written_and_read_back": 2 * N * P * 4,
            "sparse_read_GBps": round(read / s / 1e6, 1), "dense_read_GBps": round((N * P * 4 + 8 * P) / a / 1e6, 1),
            "bit_identical_to_dense": True,
            "repeats": args.repeats, "densify_repeats": len(tb),
            "timing": "HIP events around one call and around `chain` calls back to back (per call); perf_counter "
                      "until the call returns; medians of interleaved repeats",
        })
        print(json.dumps(lines[-1]), flush=True)
        del rows, wide, dense, table, staged, out_s, out_a, out_b
        torch.cuda.empty_cache()
    ctx.close()
    losing = [x["density"] for x in lines if x["sparse_over_dense"] >= 1.0]
    losing_chain = [x["density"] for x in lines if x["sparse_over_dense_back_to_back"] >= 1.0]
    lines.append({"summary": "lowest measured density at which the sparse fold no longer beats the dense delta fold",
                  "density": min(losing) if losing else None,
                  "density_back_to_back": min(losing_chain) if losing_chain else None,
                  "densities_measured": [x["density"] for x in lines]})
    print(json.dumps(lines[-1]), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
