"""Time the fold about a point against the FedAvg fold and against what a user has today.

For N device-resident client updates of a model (default 64 x ResNet-18: a common model plus 1 %
noise) each case times, in one process, with HIP events, after warm-up, as the median over --repeats
interleaved repeats:

  (a) ``FedAvgContext.fold_about_point`` with a float64 point and float64 output;
  (b) ``FedAvgContext.aggregate`` on the same table — it reads the same client bytes; (a) reads
      8 P more (the point);
  (c) the torch composition ``z + ((X.to(f64) - z) * c[:, None]).sum(0) / W`` on the same GPU;
  (d) the whole ``ClippedFedAVGAlgorithm`` round at its defaults (one iteration about the previous
      model: staging, norms, one distance call and read-back, one step), wall clock around
      ``aggregate_worker_data`` with a device synchronisation.

One JSON line per case goes to --out (default profiles/clip_lines.jsonl): the times, (a)/(b) with
the run-to-run spread of (b), (a)/(c), and the kernel's rates. Cases: fp32, fp64, bf16, fp16. There
is no CPU fallback: no GPU, no number.
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
    ClippedFedAVGAlgorithm,
    FedAvgContext,
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


def round_ms(make, msgs, previous, device, repeats) -> float:
    """Median wall clock of ``aggregate_worker_data`` over ``repeats`` rounds after one untimed round."""
    times = []
    for r in range(repeats + 1):
        algo = make()
        for wid, p in enumerate(msgs):
            algo.process_worker_data(wid, ParameterMessage(parameter=p, aggregation_weight=1.0))
        algo.set_old_parameter(previous)
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
    ap.add_argument("--round-repeats", type=int, default=5, help="repeats of the whole algorithm round")
    ap.add_argument("--dtypes", default="f32,f64,bf16,f16")
    ap.add_argument("--out", default=str(REPO / "profiles" / "clip_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("clip_bench.py needs a GPU", file=sys.stderr)
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
        zflat = base.to(torch.float64)                       # the point: the common model
        point = [zflat[o:o + n] for o, n in zip(offs, layout.numels)]
        outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        means = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        coef = [1.0 if k % 4 else 0.37 for k in range(N)]   # a quarter of the clients clipped
        cdev = torch.tensor(coef, dtype=torch.float64, device=device)
        W = float(N)

        def step():
            ctx.fold_about_point(table, dtype, coef, W, point, outs, torch.float64)

        def mean():
            ctx.aggregate(table, dtype, means, torch.float64)

        def composition():
            x = torch.stack(flats).to(torch.float64)
            return zflat + ((x - zflat) * cdev[:, None]).sum(0) / W

        for _ in range(args.warmup):
            step()
            mean()
        tc, torch_error, max_diff = [], None, None
        try:
            got = composition()
            torch.cuda.synchronize(device)
            max_diff = max(float((got[o:o + n] - out).abs().max()) for o, n, out in zip(offs, layout.numels, outs))
            del got
            for _ in range(args.torch_repeats):
                tc.append(timed(composition, stream))
        except RuntimeError as e:  # e.g. out of memory for the fp64 stack
            torch_error = str(e).splitlines()[0]
        torch.cuda.empty_cache()
        torch.cuda.synchronize(device)
        ta, tb = [], []
        for _ in range(args.repeats):  # interleaved: both see the same machine state
            ta.append(timed(step, stream))
            tb.append(timed(mean, stream))
        assert ctx.flags() == 0
        ctx.close()

        # the whole round through the plugin class, updates and previous model already on the device
        msgs = [{name: x[o:o + n].view(shape) for name, shape, o, n in zip(layout.names, layout.shapes, offs, layout.numels)}
                for x in flats]
        previous = {name: zflat[o:o + n].view(shape)
                    for name, shape, o, n in zip(layout.names, layout.shapes, offs, layout.numels)}
        whole = round_ms(lambda: ClippedFedAVGAlgorithm(1.0, device=device), msgs, previous, device, args.round_repeats)

        a, b = statistics.median(ta), statistics.median(tb)
        c = statistics.median(tc) if tc else None
        s = dtype.itemsize
        lines.append({
            "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} fold about a float64 point, float64 out",
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P,
            "fold_about_point_ms": round(a, 4), "fedavg_aggregate_ms": round(b, 4),
            "torch_composition_ms": None if c is None else round(c, 3), "torch_composition_error": torch_error,
            "torch_composition_max_abs_diff": max_diff,
            "fold_over_fedavg": round(a / b, 3),
            "fedavg_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
            "fedavg_spread_over_median": round((max(tb) - min(tb)) / b, 3),
            "fold_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "fold_spread_over_median": round((max(ta) - min(ta)) / a, 3),
            "fold_over_composition": None if c is None else round(a / c, 4),
            "fold_traffic_GBps": round((N * P * s + 8 * P + 8 * P) / a / 1e6, 1),
            "fedavg_traffic_GBps": round((N * P * s + 8 * P) / b / 1e6, 1),
            "fold_fp64_Tlaneops_per_s": round(3.0 * N * P / a / 1e9, 3),
            "clipped_round_ms": round(whole, 3), "clipped_round_iterations": 1,
            "repeats": args.repeats, "torch_repeats": args.torch_repeats, "round_repeats": args.round_repeats,
            "timing": "HIP events around each call, median of interleaved repeats; the round is wall clock",
        })
        print(json.dumps(lines[-1]), flush=True)
        del flats, table, outs, means, msgs, base, point, zflat, previous
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
