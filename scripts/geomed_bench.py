"""Time the point-distance kernel against its HBM floor and against what a user has today.

For N device-resident client updates of a model (default 64 x ResNet-18: a common model plus 1 %
noise) each case times, in one process, with HIP events, after warm-up, as the median over --repeats
interleaved repeats:

  (a) ``FedAvgContext.sqdist_to_point`` with a float64 point — the chunk kernel and its reduce;
  (b) ``FedAvgContext.aggregate`` on the same table — it reads the same client bytes: the HBM floor;
  (c) the torch composition: ``torch.stack`` -> ``.to(float64)`` -> ``(X - z).square().sum(1)``, on the GPU;
  (d) the whole ``GeometricMedianFedAVGAlgorithm`` round at its default 3 iterations (staging, norms,
      4 folds, 3 distance calls and read-backs), wall clock around ``aggregate_worker_data`` with a
      device synchronisation;
  (e) the whole ``KrumFedAVGAlgorithm`` round on the same data, for scale.

One JSON line per case goes to --out (default profiles/geomed_lines.jsonl): the times, the figure of
merit (a)/(b) with the run-to-run spread of (b), (a)/(c), and the kernel's input rate. Cases: fp32
and fp64, then bf16 and fp16 (four fp64 operations and a conversion per element on a quarter of the
fp64 bytes). There is no CPU fallback: no GPU, no number.
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
    GeometricMedianFedAVGAlgorithm,
    KrumFedAVGAlgorithm,
    ParameterMessage,
)

DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}


def timed(fn, stream) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def round_ms(make, msgs, device, repeats) -> float:
    """Median wall clock of ``aggregate_worker_data`` over ``repeats`` rounds after one untimed round."""
    times = []
    for r in range(repeats + 1):
        algo = make()
        for wid, p in enumerate(msgs):
            algo.process_worker_data(wid, ParameterMessage(parameter=p, aggregation_weight=1.0))
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        algo.aggregate_worker_data()
        torch.cuda.synchronize(device)
        if r:  # the first round builds the context and the workspace
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3, help="repeats of the (slow) torch composition")
    ap.add_argument("--round-repeats", type=int, default=5, help="repeats of the whole algorithm rounds")
    ap.add_argument("--dtypes", default="f32,f64,bf16,f16")
    ap.add_argument("--out", default=str(REPO / "profiles" / "geomed_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("geomed_bench.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    N, P = args.clients, layout.total_numel
    stream = torch.cuda.current_stream(device)
    lines = []
    for code in args.dtypes.split(","):
        dtype = DTYPES[code]
        offs, total = layout.padded_offsets(dtype.itemsize)
        gen = torch.Generator(device=device).manual_seed(1)
        base = torch.randn(total, dtype=torch.float32, device=device, generator=gen)
        flats = [(base + 0.01 * torch.randn(total, dtype=torch.float32, device=device, generator=gen)).to(dtype)
                 for _ in range(N)]
        table = ClientTable(layout.num_segments)
        for x in flats:
            table.add_client([x[o:o + n] for o, n in zip(offs, layout.numels)], [1.0] * layout.num_segments)
        ctx = FedAvgContext(layout, device)
        outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        ctx.aggregate(table, dtype, outs, torch.float64)   # the point: the clients' mean
        zflat = torch.zeros(total, dtype=torch.float64, device=device)
        for o, n, z in zip(offs, layout.numels, outs):
            zflat[o:o + n] = z
        point = [z.clone() for z in outs]

        def distances():
            return ctx.sqdist_to_point(table, dtype, point)

        def mean():
            ctx.aggregate(table, dtype, outs, torch.float64)

        def composition():
            x = torch.stack(flats).to(torch.float64)
            return (x - zflat).square().sum(1)

        for _ in range(args.warmup):
            distances()
            mean()
        tc, torch_error = [], None
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

        # the whole rounds through the plugin classes, updates already on the device
        msgs = [{name: x[o:o + n].view(shape) for name, shape, o, n in zip(layout.names, layout.shapes, offs, layout.numels)}
                for x in flats]
        geomed = round_ms(lambda: GeometricMedianFedAVGAlgorithm(device=device), msgs, device, args.round_repeats)
        krum = round_ms(lambda: KrumFedAVGAlgorithm((N - 3) // 2, 1, device=device), msgs, device, args.round_repeats)

        a, b = statistics.median(ta), statistics.median(tb)
        c = statistics.median(tc) if tc else None
        lines.append({
            "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} squared distances to a float64 point",
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P,
            "sqdist_to_point_ms": round(a, 4), "fedavg_aggregate_ms": round(b, 4),
            "torch_composition_ms": None if c is None else round(c, 3), "torch_composition_error": torch_error,
            "sqdist_over_fedavg": round(a / b, 3),
            "fedavg_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
            "fedavg_spread_over_median": round((max(tb) - min(tb)) / b, 3),
            "sqdist_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "sqdist_over_composition": None if c is None else round(a / c, 4),
            "sqdist_input_GBps": round((N * P * dtype.itemsize + 8 * P) / a / 1e6, 1),
            "fedavg_input_GBps": round(N * P * dtype.itemsize / b / 1e6, 1),
            "sqdist_fp64_Tlaneops_per_s": round(3.0 * N * P / a / 1e9, 3),
            "geometric_median_round_ms": round(geomed, 3), "geometric_median_iterations": 3,
            "krum_round_ms": round(krum, 3), "krum_round_f": (N - 3) // 2,
            "repeats": args.repeats, "torch_repeats": args.torch_repeats, "round_repeats": args.round_repeats,
            "timing": "HIP events around each call, median of interleaved repeats; the rounds are wall clock",
        })
        print(json.dumps(lines[-1]), flush=True)
        del flats, table, outs, msgs, base, point, zflat
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
