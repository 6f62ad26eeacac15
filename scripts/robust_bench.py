"""Time the robust aggregation kernel against its HBM floor and against what a user has today.

For N device-resident client updates of a model (default 64 x ResNet-18) each case times, in one
process, with HIP events, after warm-up, as the median over --repeats interleaved repeats:

  (a) ``FedAvgContext.robust_aggregate`` — the new kernel, one launch;
  (b) ``FedAvgContext.aggregate`` on the same table — the weighted mean moves the same bytes: the floor;
  (c) the torch composition: ``torch.stack`` -> ``.to(float64)`` -> ``torch.sort`` -> slice-sum, on the GPU.

One JSON line per case goes to --out (default profiles/robust_lines.jsonl): the three times, the
ratios (a)/(b) and (a)/(c), and the kernel's input bytes over its time. Cases: fp32 median, fp32
trimmed mean (trim 0.1), fp64 median (64-bit keys). There is no CPU fallback: no GPU, no number.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from bench import resnet18_layout  # noqa: E402
from distributed_learning_simulation_lib_amd import ClientTable, FedAvgContext  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import robust_trim  # noqa: E402


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
    ap.add_argument("--torch-repeats", type=int, default=5, help="repeats of the (slow) torch composition")
    ap.add_argument("--out", default=str(REPO / "profiles" / "robust_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("robust_bench.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    N, P = args.clients, layout.total_numel
    stream = torch.cuda.current_stream(device)
    lines = []
    for dtype, mode, trim in ((torch.float32, "median", 0.0), (torch.float32, "trimmed_mean", 0.1),
                              (torch.float64, "median", 0.0)):
        offs, total = layout.padded_offsets(dtype.itemsize)
        gen = torch.Generator(device=device).manual_seed(1)
        flats = [torch.randn(total, dtype=dtype, device=device, generator=gen) for _ in range(N)]
        table = ClientTable(layout.num_segments)
        for f in flats:
            table.add_client([f[o:o + n] for o, n in zip(offs, layout.numels)], [1.0] * layout.num_segments)
        ctx = FedAvgContext(layout, device)
        outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        k = robust_trim(mode, trim, N)

        def robust():
            ctx.robust_aggregate(table, dtype, mode, trim, outs, torch.float64)

        def mean():
            ctx.aggregate(table, dtype, outs, torch.float64)

        def composition():
            s = torch.sort(torch.stack(flats).to(torch.float64), dim=0).values
            return s[k:N - k].sum(dim=0) / float(N - 2 * k)

        for _ in range(args.warmup):
            robust()
            mean()
        composition()
        torch.cuda.synchronize(device)
        ta, tb, tc = [], [], []
        for _ in range(args.repeats):  # interleaved: both see the same machine state
            ta.append(timed(robust, stream))
            tb.append(timed(mean, stream))
        for _ in range(args.torch_repeats):
            tc.append(timed(composition, stream))
        assert ctx.flags() == 0
        a, b, c = (statistics.median(t) for t in (ta, tb, tc))
        in_bytes = N * P * dtype.itemsize
        lines.append({
            "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} {mode}" + (f" trim {trim}" if mode != "median" else ""),
            "device": torch.cuda.get_device_name(device), "clients": N, "elements": P, "k": k,
            "robust_ms": round(a, 4), "fedavg_aggregate_ms": round(b, 4), "torch_sort_composition_ms": round(c, 3),
            "robust_over_fedavg": round(a / b, 3), "robust_over_composition": round(a / c, 4),
            "robust_input_GBps": round(in_bytes / a / 1e6, 1), "fedavg_input_GBps": round(in_bytes / b / 1e6, 1),
            "robust_ms_min_max": [round(min(ta), 4), round(max(ta), 4)], "repeats": args.repeats,
            "torch_repeats": args.torch_repeats, "timing": "HIP events around each call, median of interleaved repeats",
        })
        print(json.dumps(lines[-1]), flush=True)
        ctx.close()
        del flats, table, outs
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
