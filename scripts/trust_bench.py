"""Time the moments about a point against the distances to a point and against what a user has today.

For N device-resident client updates of a model (default 64 x ResNet-18: a common model plus a
common step plus 1 % noise) each case times, in one process, with HIP events, after warm-up, as the
median over --repeats interleaved repeats:

  (a) ``FedAvgContext.moments_about_point`` with a float64 centre and a float64 direction;
  (b) ``FedAvgContext.sqdist_to_point`` on the same table and centre — the yardstick: it reads the
      same client bytes and the centre; (a) reads 8 P more (the direction) and does one more multiply
      and add per element;
  (c) the torch composition ``X = stack(...).to(f64); ((X - v) * g).sum(1); ((X - v) ** 2).sum(1)`` on
      the same GPU;
  (d) the whole ``FLTrustFedAVGAlgorithm`` round (staging, norms and read-back, the direction, one
      moments call and read-back, one step), wall clock around ``aggregate_worker_data`` with a
      device synchronisation.

One JSON line per case goes to --out (default profiles/trust_lines.jsonl): the times with their
min / max and spread, (a)/(b) and (a)/(c), and the kernel's rates. Cases: fp32, fp64, bf16, fp16.
There is no CPU fallback: no GPU, no number.
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
    FLTrustFedAVGAlgorithm,
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


def round_ms(make, msgs, previous, device, repeats) -> list[float]:
    """Wall clock of ``aggregate_worker_data`` over ``repeats`` rounds after one untimed round."""
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
    return times


def spread(ts: list[float]) -> dict:
    m = statistics.median(ts)
    return {"median": round(m, 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "spread_over_median": round((max(ts) - min(ts)) / m, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3, help="repeats of the (slow) torch composition")
    ap.add_argument("--round-repeats", type=int, default=5, help="repeats of the whole algorithm round")
    ap.add_argument("--dtypes", default="f32,f64,bf16,f16")
    ap.add_argument("--out", default=str(REPO / "profiles" / "trust_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("trust_bench.py needs a GPU", file=sys.stderr)
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
        move = 0.05 * torch.randn(total, dtype=torch.float32, device=device, generator=gen)
        flats = [(base + (move if k % 4 else -move)      # a quarter of the clients step the other way
                  + 0.01 * torch.randn(total, dtype=torch.float32, device=device, generator=gen)).to(dtype)
                 for k in range(N)]
        table = ClientTable(layout.num_segments)
        for x in flats:
            table.add_client([x[o:o + n] for o, n in zip(offs, layout.numels)], [1.0] * layout.num_segments)
        ctx = FedAvgContext(layout, device)
        vflat = base.to(torch.float64)                       # the centre: the common model
        gflat = flats[1].to(torch.float64) - vflat           # the direction: client 1's update
        centre = [vflat[o:o + n] for o, n in zip(offs, layout.numels)]
        direction = [gflat[o:o + n] for o, n in zip(offs, layout.numels)]
        got = {}

        def moments():
            got["T"], got["S"] = ctx.moments_about_point(table, dtype, centre, direction)

        def sqdist():
            got["D"] = ctx.sqdist_to_point(table, dtype, centre)

        def composition():
            x = torch.stack(flats).to(torch.float64)
            d = x - vflat
            return (d * gflat).sum(1), (d ** 2).sum(1)

        for _ in range(args.warmup):
            moments()
            sqdist()
        torch.cuda.synchronize(device)
        same_bits = bool(torch.equal(got["S"].view(torch.int64), got["D"].view(torch.int64)))
        tc, torch_error, rel_dot, rel_sq = [], None, None, None
        try:
            cT, cS = composition()
            torch.cuda.synchronize(device)
            rel_dot = float(((cT - got["T"]).abs() / got["T"].abs().clamp_min(1e-300)).max())
            rel_sq = float(((cS - got["S"]).abs() / got["S"]).max())
            del cT, cS
            for _ in range(args.torch_repeats):
                tc.append(timed(composition, stream))
        except RuntimeError as e:  # e.g. out of memory for the fp64 stack
            torch_error = str(e).splitlines()[0]
        torch.cuda.empty_cache()
        torch.cuda.synchronize(device)
        ta, tb = [], []
        for _ in range(args.repeats):  # interleaved: both see the same machine state
            ta.append(timed(moments, stream))
            tb.append(timed(sqdist, stream))
        assert ctx.flags() == 0
        ctx.close()

        # the whole round through the plugin class, updates and previous model already on the device
        msgs = [{name: x[o:o + n].view(shape) for name, shape, o, n in zip(layout.names, layout.shapes, offs, layout.numels)}
                for x in flats]
        previous = {name: vflat[o:o + n].view(shape)
                    for name, shape, o, n in zip(layout.names, layout.shapes, offs, layout.numels)}
        whole = round_ms(lambda: FLTrustFedAVGAlgorithm(1, device=device), msgs, previous, device, args.round_repeats)

        a, b = statistics.median(ta), statistics.median(tb)
        c = statistics.median(tc) if tc else None
        s = dtype.itemsize
        lines.append({
            "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} moments about a float64 centre with a float64 direction",
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P,
            "moments_about_point_ms": spread(ta), "sqdist_to_point_ms": spread(tb),
            "torch_composition_ms": None if not tc else spread(tc), "torch_composition_error": torch_error,
            "torch_composition_max_rel_diff": {"dots": rel_dot, "sqnorms": rel_sq},
            "sqnorms_bit_identical_to_sqdist": same_bits,
            "moments_over_sqdist": round(a / b, 3),
            "moments_over_two_sqdist": round(a / (2 * b), 3),
            "moments_over_composition": None if c is None else round(a / c, 4),
            "moments_traffic_GBps": round((N * P * s + 16 * P) / a / 1e6, 1),
            "sqdist_traffic_GBps": round((N * P * s + 8 * P) / b / 1e6, 1),
            "moments_fp64_Tlaneops_per_s": round(5.0 * N * P / a / 1e9, 3),
            "fltrust_round_ms": spread(whole),
            "repeats": args.repeats, "torch_repeats": args.torch_repeats, "round_repeats": args.round_repeats,
            "timing": "HIP events around each call, median of interleaved repeats; the round is wall clock",
        })
        print(json.dumps(lines[-1]), flush=True)
        del flats, table, msgs, base, move, centre, direction, vflat, gflat, previous, got
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
