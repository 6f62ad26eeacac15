"""Time the pairwise-distance kernel against its HBM floor and against what a user has today.

For N device-resident client updates of a model (default 64 x ResNet-18) each case times, in one
process, with HIP events, after warm-up, as the median over --repeats interleaved repeats:

  (a) ``FedAvgContext.pairwise_sqdist`` — the chunk kernel and its reduce;
  (b) ``FedAvgContext.aggregate`` on the same table — it reads the same bytes: the HBM floor;
  (c) the torch composition: ``torch.stack`` -> ``.to(float64)`` -> ``torch.cdist(...) ** 2``, on the GPU;
  and the whole ``KrumFedAVGAlgorithm`` round (staging, distances, read-back, selection, FedAvg of
  the chosen), wall clock around ``aggregate_worker_data`` with a device synchronisation.

One JSON line per case goes to --out (default profiles/krum_lines.jsonl): the times, the ratios
(a)/(b) and (a)/(c), and the kernel's fp64 lane-operation rate (two per pair and element: a
subtraction and an FMA). Cases: fp32 and fp64. There is no CPU fallback: no GPU, no number.
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
    ClientTable,
    FedAvgContext,
    KrumFedAVGAlgorithm,
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3, help="repeats of the (slow) torch composition")
    ap.add_argument("--round-repeats", type=int, default=5, help="repeats of the whole algorithm round")
    ap.add_argument("--out", default=str(REPO / "profiles" / "krum_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("krum_bench.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    N, P = args.clients, layout.total_numel
    f = (N - 3) // 2
    stream = torch.cuda.current_stream(device)
    lines = []
    for dtype in (torch.float32, torch.float64):
        offs, total = layout.padded_offsets(dtype.itemsize)
        gen = torch.Generator(device=device).manual_seed(1)
        base = torch.randn(total, dtype=dtype, device=device, generator=gen)
        flats = [base + 0.01 * torch.randn(total, dtype=dtype, device=device, generator=gen) for _ in range(N)]
        table = ClientTable(layout.num_segments)
        for x in flats:
            table.add_client([x[o:o + n] for o, n in zip(offs, layout.numels)], [1.0] * layout.num_segments)
        ctx = FedAvgContext(layout, device)
        outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]

        def distances():
            return ctx.pairwise_sqdist(table, dtype)

        def mean():
            ctx.aggregate(table, dtype, outs, torch.float64)

        def composition():
            x = torch.stack(flats).to(torch.float64)
            return torch.cdist(x, x) ** 2

        for _ in range(args.warmup):
            distances()
            mean()
        tc = []
        torch_error = None
        try:
            composition()
            torch.cuda.synchronize(device)
            for _ in range(args.torch_repeats):
                tc.append(timed(composition, stream))
        except RuntimeError as e:  # e.g. out of memory for the fp64 stack
            torch_error = str(e).splitlines()[0]
            torch.cuda.empty_cache()
        torch.cuda.synchronize(device)
        ta, tb = [], []
        for _ in range(args.repeats):  # interleaved: both see the same machine state
            ta.append(timed(distances, stream))
            tb.append(timed(mean, stream))
        assert ctx.flags() == 0
        ctx.close()

        # the whole round through the plugin class, updates already on the device
        msgs = [{name: x[o:o + n].view(shape) for name, shape, o, n in zip(layout.names, layout.shapes, offs, layout.numels)}
                for x in flats]
        tr = []
        for r in range(args.round_repeats + 1):
            algo = KrumFedAVGAlgorithm(f, 1, device=device)
            for wid, p in enumerate(msgs):
                algo.process_worker_data(wid, ParameterMessage(parameter=p, aggregation_weight=1.0))
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            algo.aggregate_worker_data()
            torch.cuda.synchronize(device)
            if r:  # the first round builds the context and the workspace
                tr.append((time.perf_counter() - t0) * 1e3)

        a, b = statistics.median(ta), statistics.median(tb)
        c = statistics.median(tc) if tc else None
        lane_ops = 2.0 * (N * (N - 1) / 2) * P
        lines.append({
            "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} pairwise squared distances",
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P, "pairs": N * (N - 1) // 2,
            "pairwise_sqdist_ms": round(a, 4), "fedavg_aggregate_ms": round(b, 4),
            "torch_cdist_composition_ms": None if c is None else round(c, 3), "torch_cdist_error": torch_error,
            "sqdist_over_fedavg": round(a / b, 3), "sqdist_over_composition": None if c is None else round(a / c, 4),
            "sqdist_fp64_Tlaneops_per_s": round(lane_ops / a / 1e9, 2),
            "sqdist_input_GBps": round(N * P * dtype.itemsize / a / 1e6, 1),
            "sqdist_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "krum_round_ms": round(statistics.median(tr), 3), "krum_round_f": f, "repeats": args.repeats,
            "torch_repeats": args.torch_repeats, "round_repeats": args.round_repeats,
            "timing": "HIP events around each call, median of interleaved repeats; the round is wall clock",
        })
        print(json.dumps(lines[-1]), flush=True)
        del flats, table, outs, msgs, base
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
