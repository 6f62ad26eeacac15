"""Time the broadcast encoder against the torch compositions a user calls today.

On one ResNet-18 result (62 tensors, 11,689,512 elements; the tensors are views into one flat
buffer, as the fold's result is), fp64 and fp32, QSGD and NNADQ, in one process on one GPU, after
warm-up, as the median over interleaved repeats:

  (k) the GPU call alone: ``FedAvgContext.quant_encode`` into a resident blob (HIP events around
      the asynchronous call, so its host work is inside);
  (q) the whole ``BroadcastQuantizer.encode_to_host``: encode, the flag check, one D2H copy of the
      blob and the per-record host copies (wall clock);
  (b) the baseline: the existing ``stochastic_quantization()`` / ``NNADQ()`` composition on the same
      device tensors, then ``.to("cpu")`` per record (wall clock); and (bk) that composition alone,
      synchronised, without the copies;
  (d) the dense broadcast's device-to-host leg: ``.to("cpu", torch.float64)`` per tensor.

One JSON line per (scheme, dtype) goes to --out (default profiles/quant_encode_lines.jsonl): each
time with its spread, the ratios (bk)/(k) and (b)/(q), and the bytes that cross to the host against
the dense fp64 copy. The records of (k) are compared with the CPU path's bytes before anything is
timed. There is no CPU fallback: no GPU, no number.
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
from distributed_learning_simulation_lib_amd import BroadcastQuantizer  # noqa: E402
from distributed_learning_simulation_lib_amd.quantized import NNADQ, codec_for, stochastic_quantization  # noqa: E402


def spread(ts: list[float]) -> dict:
    s = sorted(ts)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "p10_ms": s[len(s) // 10], "p90_ms": s[-1 - len(s) // 10], "runs": len(s)}


def wall(fn, device) -> float:
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3


def events(fn, device) -> float:
    stream = torch.cuda.current_stream(device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "quant_encode_lines.jsonl")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("at least 20 runs")
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    lines = []
    for dtype in (torch.float64, torch.float32):
        g = torch.Generator(device="cpu").manual_seed(0)
        flat = (torch.randn(layout.total_numel, generator=g, dtype=torch.float64) * 0.05).to(dtype).to(device)
        param, off = {}, 0
        for name, shape, n in zip(layout.names, layout.shapes, layout.numels):
            param[name] = flat[off : off + n].view(shape)  # element-aligned views, as the fold's result
            off += n
        dense_bytes = layout.total_numel * 8
        for scheme in ("qsgd", "nnadq"):
            q = BroadcastQuantizer(scheme, seed=1)
            codec = codec_for(dtype, scheme)
            # correctness first: the device records are the CPU path's bytes
            small = {k: v for k, v in list(param.items())[:8]}
            dev = q(small, 3)
            cpu = q({k: v.cpu() for k, v in small.items()}, 3)
            assert all(torch.equal(dev[k].record.cpu(), cpu[k].record) for k in small), "device and CPU records differ"

            ctx = q._context(device)
            tensors = [v.reshape(-1) for v in param.values()]
            sizes = [codec.record_bytes(t.numel()) for t in tensors]
            blob = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
            recs, o = [], 0
            for s in sizes:
                recs.append(blob[o : o + s])
                o += s
            if scheme == "qsgd":
                compose = stochastic_quantization(255)[0]
            else:
                compose = NNADQ(0.01)[0]

            def k_call():
                ctx.quant_encode(codec.code, tensors, recs, 255, 0.01, 1, 5)

            def q_call():
                q.encode_to_host(param, 5)

            def bk_call():
                compose(param)

            def b_call():
                {k: v.to("cpu") for k, v in compose(param).items()}

            def d_call():
                {k: v.to("cpu", torch.float64) for k, v in param.items()}

            legs = {"k": (events, k_call), "q": (wall, q_call), "bk": (wall, bk_call), "b": (wall, b_call),
                    "d": (wall, d_call)}
            for _ in range(args.warmup):
                for timer, fn in legs.values():
                    timer(fn, device)
            ts: dict[str, list[float]] = {k: [] for k in legs}
            for _ in range(args.runs):  # interleaved: drift hits every leg alike
                for key, (timer, fn) in legs.items():
                    ts[key].append(timer(fn, device))
            assert ctx.flags() == 0
            sp = {k: spread(v) for k, v in ts.items()}
            line = {
                "what": "quant_encode", "scheme": scheme, "dtype": str(dtype).replace("torch.", ""),
                "tensors": len(tensors), "elements": layout.total_numel, "device": torch.cuda.get_device_name(device),
                "kernel_call": sp["k"], "quantizer_to_host": sp["q"], "composition_device_only": sp["bk"],
                "composition_to_host": sp["b"], "dense_fp64_to_host": sp["d"],
                "ratio_composition_over_kernel_call": sp["bk"]["median_ms"] / sp["k"]["median_ms"],
                "ratio_composition_to_host_over_quantizer": sp["b"]["median_ms"] / sp["q"]["median_ms"],
                "ratio_dense_to_host_over_quantizer": sp["d"]["median_ms"] / sp["q"]["median_ms"],
                "record_bytes": sum(sizes), "dense_fp64_bytes": dense_bytes,
                "bytes_per_element": sum(sizes) / layout.total_numel,
                "d2h_bytes_saved": dense_bytes - sum(sizes),
                "kernel_call_input_gbps": 2 * layout.total_numel * flat.element_size() / sp["k"]["median_ms"] / 1e6,
            }
            lines.append(line)
            print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
