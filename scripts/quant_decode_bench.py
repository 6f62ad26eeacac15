"""Time the record decoder against the torch composition it replaces.

On one ResNet-18 broadcast (62 records, 11,689,512 elements), fp64 and fp32 codecs, QSGD and NNADQ, in
one process on one GPU, after warm-up, as the median over interleaved repeats:

  (k)  the GPU call alone: ``FedAvgContext.quant_decode`` of device records into resident tensors (HIP
       events around the asynchronous call, so its host work is inside); (k64) the same with the fp64
       copy (fp32 codecs);
  (dq) the whole ``BroadcastDequantizer`` call on the same device records with ``out=``: the launch
       and the flag check, which waits for the stream (wall clock);
  (b)  the composition a caller had before: the eager torch chain of ``dequantize_tensor`` per tensor
       on the same device records (the host path's code, which is what ran on device records too),
       synchronised (wall clock);
  (c)  host records to device tensors, both ways: (cu) ``BroadcastDequantizer(records, device=,
       out=)``: one pinned blob, one upload, the kernel; (ch) the eager chain on the host, then
       ``.to(device)`` per tensor (wall clock; timed in a loop of its own after the others).

One JSON line per (scheme, dtype) goes to --out (default profiles/quant_decode_lines.jsonl): each time
with its spread, the ratio (b)/(k) and (ch)/(cu), and the byte model (input 1.125 or 1 byte per
element, output 4, 8 or 12). The kernel's output is compared with the composition's, bit for bit, on
the whole layout before anything is timed. There is no CPU fallback: no GPU, no number.
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
from distributed_learning_simulation_lib_amd import BroadcastDequantizer, BroadcastQuantizer  # noqa: E402
from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor, _dequantize_host  # noqa: E402


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
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "quant_decode_lines.jsonl")
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
            param[name] = flat[off : off + n].view(shape)
            off += n
        for scheme in ("qsgd", "nnadq"):
            host = BroadcastQuantizer(scheme, seed=1).encode_to_host(param, 5)  # the records a worker receives
            dev = {k: QuantizedTensor(q.record.to(device), q.shape, q.codec) for k, q in host.items()}
            record_bytes = sum(q.record.numel() for q in host.values())
            code = next(iter(host.values())).codec.code
            # element-aligned views into one flat buffer, as a model's parameters can be
            out_flat = torch.empty(layout.total_numel, dtype=dtype, device=device)
            wide_flat = torch.empty(layout.total_numel, dtype=torch.float64, device=device)
            out, wide, off = {}, {}, 0
            for name, shape, n in zip(layout.names, layout.shapes, layout.numels):
                out[name] = out_flat[off : off + n].view(shape)
                wide[name] = wide_flat[off : off + n].view(shape)
                off += n
            deq = BroadcastDequantizer()
            ctx = deq._context(device)
            recs = [q.record for q in dev.values()]
            outs = [o.reshape(-1) for o in out.values()]
            wides = [w.reshape(-1) for w in wide.values()]
            fp32 = dtype == torch.float32

            # correctness first: the kernel's bits are the composition's, on the whole layout
            ctx.quant_decode(code, recs, outs, wides if fp32 else None)
            assert ctx.flags() == 0
            for name, q in dev.items():
                ref = _dequantize_host(q)
                assert torch.equal(out[name].reshape(-1).view(torch.uint8), ref.reshape(-1).view(torch.uint8)), name
                assert not fp32 or torch.equal(wide[name], ref.to(torch.float64)), name

            def k_call():
                ctx.quant_decode(code, recs, outs)

            def k64_call():
                ctx.quant_decode(code, recs, outs, wides)

            def dq_call():
                deq(dev, out=out)

            def b_call():
                {k: _dequantize_host(q) for k, q in dev.items()}

            def cu_call():
                deq(host, device=device, out=out)

            def ch_call():
                {k: _dequantize_host(q).to(device) for k, q in host.items()}

            legs = {"k": (events, k_call), "dq": (wall, dq_call), "b": (wall, b_call), "cu": (wall, cu_call),
                    "ch": (wall, ch_call)}
            if fp32:
                legs["k64"] = (events, k64_call)
            # (ch) keeps every core of the host busy for up to 0.1 s a run: it is timed after the
            # others, not between them, so that it does not disturb the legs that take a millisecond
            apart = {"ch": legs.pop("ch")}
            ts: dict[str, list[float]] = {}
            for group in (legs, apart):
                for _ in range(args.warmup):
                    for timer, fn in group.values():
                        timer(fn, device)
                ts.update({k: [] for k in group})
                for _ in range(args.runs):  # interleaved: drift hits every leg of a group alike
                    for key, (timer, fn) in group.items():
                        ts[key].append(timer(fn, device))
            assert ctx.flags() == 0
            sp = {k: spread(v) for k, v in ts.items()}
            n = layout.total_numel
            out_bytes = n * flat.element_size()
            line = {
                "what": "quant_decode", "scheme": scheme, "dtype": str(dtype).replace("torch.", ""),
                "tensors": len(recs), "elements": n, "device": torch.cuda.get_device_name(device),
                "kernel_call": sp["k"], "kernel_call_with_fp64_copy": sp.get("k64"), "dequantizer_out": sp["dq"],
                "composition_device": sp["b"], "host_records_upload_then_kernel": sp["cu"],
                "host_decode_then_upload": sp["ch"],
                "ratio_composition_over_kernel_call": sp["b"]["median_ms"] / sp["k"]["median_ms"],
                "ratio_composition_over_dequantizer": sp["b"]["median_ms"] / sp["dq"]["median_ms"],
                "ratio_host_decode_over_upload_then_kernel": sp["ch"]["median_ms"] / sp["cu"]["median_ms"],
                "record_bytes": record_bytes, "input_bytes_per_element": record_bytes / n,
                "output_bytes_per_element": flat.element_size(), "dense_upload_bytes": out_bytes,
                "kernel_call_gbps": (record_bytes + out_bytes) / sp["k"]["median_ms"] / 1e6,
                "kernel_call_with_fp64_copy_gbps":
                    (record_bytes + out_bytes + 8 * n) / sp["k64"]["median_ms"] / 1e6 if fp32 else None,
            }
            lines.append(line)
            print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
