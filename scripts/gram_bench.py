"""Time the Gram kernel against what a user has today and against its neighbours.

For N device-resident client updates of a model (default 64 x ResNet-18) each case times, in one
process, with HIP events, after warm-up, as the median (with min and max) over --repeats
interleaved repeats:

  (a) ``FedAvgContext.gram_about_point`` — the chunk kernel and its reduce, with a point and, in the
      history cases, with the history tables;
  (b) the torch composition on the same device tensors: ``D = stack.to(float64) - v; D @ D.T``, plus
      ``H += D`` (and ``H @ H.T``) in the history cases;
  (c) ``FedAvgContext.pairwise_sqdist`` on the same table — another quantity of the same shape, for scale;
  (d) ``FedAvgContext.aggregate`` on the same table — the FedAvg fold of the same client bytes.

One JSON line per case goes to --out (default profiles/gram_lines.jsonl) with the byte model
(N * P * s_in + P * 8, plus 2 * N * P * 8 with history) and the operation model (the multiply-adds of
the 16 x 16 tiles actually computed). Cases: the four client dtypes, without and with history. There
is no CPU fallback: no GPU, no number.
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


def timed(fn, stream) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts: list[float]) -> dict:
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def tiles_computed(n: int, block: int = 64, edge: int = 16) -> int:
    """The 16 x 16 tiles the kernel multiplies for n clients: per block pair the strips that hold a
    client, the diagonal pairs only on or above the diagonal."""
    nb = (n + block - 1) // block
    strips = [(min(block, n - b * block) + edge - 1) // edge for b in range(nb)]
    return sum(strips[i] * (strips[i] + 1) // 2 if i == j else strips[i] * strips[j]
               for i in range(nb) for j in range(i, nb))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=str(REPO / "profiles" / "gram_lines.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("gram_bench.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    N, P, T = args.clients, layout.total_numel, layout.num_segments
    stream = torch.cuda.current_stream(device)
    lines = []
    for dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        offs, total = layout.padded_offsets(dtype.itemsize)
        gen = torch.Generator(device=device).manual_seed(1)
        base = torch.randn(total, dtype=torch.float64, device=device, generator=gen)
        flats = [(base + 0.01 * torch.randn(total, dtype=torch.float64, device=device, generator=gen)).to(dtype)
                 for _ in range(N)]
        split = lambda x: [x[o:o + n] for o, n in zip(offs, layout.numels)]  # noqa: E731
        table = ClientTable(T)
        for x in flats:
            table.add_client(split(x), [1.0] * T)
        point = split(base)
        ctx = FedAvgContext(layout, device)
        outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
        for history in (False, True):
            hin = hout = H = None
            if history:
                H = 0.01 * torch.randn((N, total), dtype=torch.float64, device=device, generator=gen)
                hin = [split(H[i]) for i in range(N)]
                hout = [split(torch.empty(total, dtype=torch.float64, device=device)) for _ in range(N)]

            def gram():
                return ctx.gram_about_point(table, dtype, point, hin, hout)

            def composition():
                D = torch.stack(flats).to(torch.float64) - base
                if history:
                    H.add_(D)
                    return H @ H.T
                return D @ D.T

            def distances():
                return ctx.pairwise_sqdist(table, dtype)

            def mean():
                ctx.aggregate(table, dtype, outs, torch.float64)

            calls = (gram, composition, distances, mean)
            for _ in range(args.warmup):
                for fn in calls:
                    fn()
            torch.cuda.synchronize(device)
            times: list[list[float]] = [[] for _ in calls]
            for _ in range(args.repeats):  # interleaved: every call sees the same machine state
                for ts, fn in zip(times, calls):
                    ts.append(timed(fn, stream))
            assert ctx.flags() == 0
            a = statistics.median(times[0])
            model_bytes = N * P * dtype.itemsize + P * 8 + (2 * N * P * 8 if history else 0)
            macs = tiles_computed(N) * 256 * P
            lines.append({
                "case": f"{N} x resnet18 {str(dtype).removeprefix('torch.')} Gram about a point"
                        + (" with history" if history else ""),
                "device": torch.cuda.get_device_name(device), "clients": N, "elements": P, "history": history,
                "gram_about_point_ms": spread(times[0]), "torch_composition_ms": spread(times[1]),
                "pairwise_sqdist_ms": spread(times[2]), "fedavg_aggregate_ms": spread(times[3]),
                "gram_over_composition": round(a / statistics.median(times[1]), 4),
                "gram_over_sqdist": round(a / statistics.median(times[2]), 4),
                "gram_over_fedavg": round(a / statistics.median(times[3]), 4),
                "model_bytes": model_bytes, "model_GBps": round(model_bytes / a / 1e6, 1),
                "tile_multiply_adds": macs, "fp64_matrix_TFLOPs": round(2 * macs / a / 1e9, 2),
                "repeats": args.repeats, "warmup": args.warmup,
                "timing": "HIP events around each call, median (min, max) of interleaved repeats; not traced",
            })
            print(json.dumps(lines[-1]), flush=True)
            del hin, hout, H
            torch.cuda.empty_cache()
        ctx.close()
        del flats, table, outs, point, base
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
