"""Time the mean-around-median kernel against the median kernel it shares its network with, against
its HBM floor, and a whole Bulyan round.

For N device-resident client updates of a model (default 64 x ResNet-18) each case times, in one
process, after warm-up, as the median over --repeats interleaved repeats:

  (a) ``FedAvgContext.mean_around_median`` with ``keep = N // 2`` — the new kernel, one launch;
  (b) ``FedAvgContext.robust_aggregate`` median on the same table — the same network, the same bytes;
  (c) ``FedAvgContext.aggregate`` on the same table — the weighted mean moves the same bytes: the floor;
  (d) a whole ``BulyanFedAVGAlgorithm`` round (n = N, f = N // 8: distances, read-back, selection,
      coordinate step), wall clock around a call that ends in a device synchronise.

(a)-(c) are timed with HIP events around each call. One JSON line per input dtype goes to --out
(default profiles/bulyan_lines.jsonl): the times, the ratios (a)/(b) and (a)/(c), and the spread of
(b) — (max - min) / median over its repeats — which is what a difference between (a) and (b) has
to exceed to mean anything. There is no CPU fallback: no GPU, no number.
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
from distributed_learning_simulation_lib_amd import (  # noqa: E402
    BulyanFedAVGAlgorithm,
    ClientTable,
    FedAvgContext,
    ParameterMessage,
)


def timed(fn, stream) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--round-repeats", type=int, default=5, help="repeats of the whole Bulyan round")
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--out", default=str(REPO / "profiles" / "bulyan_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bulyan_bench.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    N, P = args.clients, layout.total_numel
    keep, f = N // 2, N // 8
    stream = torch.cuda.current_stream(device)
    lines = []
    for dtype in (getattr(torch, d) for d in args.dtypes.split(",")):
        offs, total = layout.padded_offsets(dtype.itemsize)
        gen = torch.Generator(device=device).manual_seed(1)
        flats = [torch.randn(total, dtype=dtype, device=device, generator=gen) for _ in range(N)]
        rows = [[x[o:o + n] for o, n in zip(offs, layout.numels)] for x in flats]
        table = ClientTable(layout.num_segments)
        for r in rows:
            table.add_client(r, [1.0] * layout.num_segments)
        ctx = FedAvgContext(layout, device)
        outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]

        def mam():
            ctx.mean_around_median(table, dtype, keep, outs, torch.float64)

        def median():
            ctx.robust_aggregate(table, dtype, "median", 0.0, outs, torch.float64)

        def mean():
            ctx.aggregate(table, dtype, outs, torch.float64)

        def bulyan_round() -> float:
            algo = BulyanFedAVGAlgorithm(num_byzantine=f, device=device)
            for wid, r in enumerate(rows):
                algo.process_worker_data(wid, ParameterMessage(
                    parameter={name: t.view(shape) for name, shape, t in zip(layout.names, layout.shapes, r)},
                    aggregation_weight=1))
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            algo.aggregate_worker_data()
            torch.cuda.synchronize(device)
            return (time.perf_counter() - t0) * 1e3

        for _ in range(args.warmup):
            mam()
            median()
            mean()
        bulyan_round()
        torch.cuda.synchronize(device)
        ta, tb, tc = [], [], []
        for _ in range(args.repeats):  # interleaved: all three see the same machine state
            ta.append(timed(mam, stream))
            tb.append(timed(median, stream))
            tc.append(timed(mean, stream))
        td = [bulyan_round() for _ in range(args.round_repeats)]
        assert ctx.flags() == 0
        a, b, c, d = (statistics.median(t) for t in (ta, tb, tc, td))
        in_bytes = N * P * dtype.itemsize
        lines.append({
            "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} keep {keep}",
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P, "keep": keep,
            "mean_around_median_ms": round(a, 4), "robust_median_ms": round(b, 4), "fedavg_aggregate_ms": round(c, 4),
            "mam_over_median": round(a / b, 3), "mam_over_fedavg": round(a / c, 3),
            "median_spread": round((max(tb) - min(tb)) / b, 3),
            "mam_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "median_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
            "mam_input_GBps": round(in_bytes / a / 1e6, 1),
            "bulyan_round_ms": round(d, 3), "bulyan_round_ms_min_max": [round(min(td), 3), round(max(td), 3)],
            "bulyan_f": f, "repeats": args.repeats, "round_repeats": args.round_repeats,
            "timing": "HIP events around each call, median of interleaved repeats; the round: host clock "
                      "around aggregate_worker_data ending in a device synchronise",
        })
        print(json.dumps(lines[-1]), flush=True)
        ctx.close()
        del flats, rows, table, outs
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
