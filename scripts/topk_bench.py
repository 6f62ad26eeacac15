"""Time the top-k step with error feedback against the torch composition it replaces.

One client's ResNet-18 layout (62 tensors, 11,689,512 elements) in fp32 and fp16, N(0, 0.1^2) deltas
with a residual, at ratios 0.1 %, 1 % and 10 %, in one process on one GPU, after warm-up, as the
median over interleaved repeats:

  (k)  the GPU call alone: ``FedAvgContext.topk_sparsify`` into resident outputs (HIP events around
       the asynchronous call, so its host work is inside);
  (k') eight calls back to back between one pair of events, per call: the host work of a call
       overlaps the kernels of the one before;
  (b)  the baseline: the per-tensor torch composition (``sparse._topk_sparsify_torch``: add, a stable
       sort of all magnitudes, a sort of the kept positions, a clone, a gather, a scatter) on the
       same device tensors, wall clock, synchronised;
  (p)  the package's ``topk_sparsify_parameter``: the call plus the output allocation, wall clock,
       synchronised.

One JSON line per case goes to --out (default profiles/topk_lines.jsonl): each time with its spread,
the ratios (b)/(k) and (b)/(p), and the byte model of the call with the rate it gives over (k') and
its share of the 8.0 TB/s HBM peak. The model counts what the passes read and write of the tensors
themselves: the first pass reads the delta and the residual and writes the total, every later pass
(one per further digit, the count and the write pass) reads the total, and the write pass stores an
index, a value and a zero per sent entry; the histograms and counts are left out. The outputs of (k)
are compared bit for bit with the composition's before anything is timed. No GPU, no number.
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
from distributed_learning_simulation_lib_amd import sparse  # noqa: E402

HBM_PEAK_GBPS = 8000.0
DIGIT_PASSES = {torch.float32: 3, torch.float16: 2}
BURST = 8


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
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "topk_lines.jsonl")
    args = ap.parse_args()
    if args.runs < 15:
        ap.error("at least 15 runs")
    device = torch.device("cuda", 0)
    ctx = sparse._context(device)
    layout = resnet18_layout()
    lines = []
    for dtype in (torch.float32, torch.float16):
        g = torch.Generator(device="cpu").manual_seed(0)
        delta = {n: (torch.randn(s, generator=g) * 0.1).to(dtype).to(device) for n, s in zip(layout.names, layout.shapes)}
        error = {n: (torch.randn(s, generator=g) * 0.03).to(dtype).to(device)
                 for n, s in zip(layout.names, layout.shapes)}
        flat = [v.reshape(-1) for v in delta.values()]
        err = [v.reshape(-1) for v in error.values()]
        elements = sum(t.numel() for t in flat)
        size = flat[0].element_size()
        for ratio in (0.001, 0.01, 0.1):
            keeps = [sparse.topk_count(t.numel(), ratio=ratio) for t in flat]
            idx = [torch.empty(k, dtype=torch.int32, device=device) for k in keeps]
            val = [torch.empty(k, dtype=dtype, device=device) for k in keeps]
            res = [torch.empty_like(t) for t in flat]

            def k_call():
                ctx.topk_sparsify(flat, err, keeps, idx, val, res)

            def burst():
                for _ in range(BURST):
                    k_call()

            def b_call():
                for d, e in zip(flat, err):
                    sparse._topk_sparsify_torch(d, ratio=ratio, error=e)

            def p_call():
                sparse.topk_sparsify_parameter(delta, ratio=ratio, error=error)

            # correctness first: the kernel's bits are the composition's
            k_call()
            for d, e, i, v, r in zip(flat, err, idx, val, res):
                sent, residual = sparse._topk_sparsify_torch(d, ratio=ratio, error=e)
                as_int = torch.int32 if size == 4 else torch.int16
                assert torch.equal(i, sent.indices) and torch.equal(v.view(as_int), sent.values.view(as_int))
                assert torch.equal(r.view(as_int), residual.view(as_int)), "kernel and composition differ"

            legs = {"k": (events, k_call), "k8": (events, burst), "b": (wall, b_call), "p": (wall, p_call)}
            for _ in range(args.warmup):
                for timer, fn in legs.values():
                    timer(fn, device)
            ts: dict[str, list[float]] = {k: [] for k in legs}
            for _ in range(args.runs):  # interleaved: drift hits every leg alike
                for key, (timer, fn) in legs.items():
                    ts[key].append(timer(fn, device))
            ts["k8"] = [t / BURST for t in ts["k8"]]
            sp = {k: spread(v) for k, v in ts.items()}
            later = DIGIT_PASSES[dtype] - 1 + 2  # reads of the total after the first pass: digits - 1, count, write
            model_bytes = (3 + later) * elements * size + sum(keeps) * (4 + 2 * size)
            gbps = model_bytes / sp["k8"]["median_ms"] / 1e6
            line = {
                "what": "topk_sparsify", "case": f"resnet18_{str(dtype).replace('torch.', '')}", "ratio": ratio,
                "tensors": len(flat), "elements": elements, "kept": sum(keeps),
                "device": torch.cuda.get_device_name(device),
                "kernel_call": sp["k"], "kernel_call_in_burst_of_8": sp["k8"], "torch_composition": sp["b"],
                "package_call": sp["p"],
                "ratio_composition_over_kernel_call": sp["b"]["median_ms"] / sp["k"]["median_ms"],
                "ratio_composition_over_package_call": sp["b"]["median_ms"] / sp["p"]["median_ms"],
                "model_bytes": model_bytes, "burst_call_model_gbps": gbps,
                "burst_call_share_of_hbm_peak": gbps / HBM_PEAK_GBPS,
            }
            lines.append(line)
            print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
