"""Time the clip-and-noise pass against the torch composition a user of the reference runs today.

Three cases, in one process on one GPU, after warm-up, as the median over interleaved repeats:
one client's ResNet-18 layout (62 tensors, 11,689,512 elements) in fp64 and in fp32 through
``add_dp_noise_to_parameter`` (whole-list mode), and a 2048 x 64 fp32 embedding matrix through
``add_dp_noise`` (row mode).

  (k) the GPU call alone: ``FedAvgContext.dp_noise`` into resident outputs (HIP events around the
      asynchronous call, so its host work is inside);
  (p) the package's public function: the call, the output allocation and the flag check that turns
      a non-finite input into ``ValueError`` (wall clock, synchronised);
  (b) the baseline: the reference's composition restated in torch on the same device tensors, with
      ``torch.randn_like`` (cat, to(float64), vector_norm, clamp, div, randn_like, mul, add, and a
      slice, reshape and cast per tensor; per row for the matrix), wall clock, synchronised.

One JSON line per case goes to --out (default profiles/dp_lines.jsonl): each time with its spread,
the ratio (b)/(k), and the byte model of the call — two reads of the input plus one write — with the
rate it gives over (k) and its share of the 8.0 TB/s HBM peak. The outputs of (k) are compared with
the CPU path's bytes on a slice before anything is timed. There is no CPU fallback: no GPU, no number.
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
from distributed_learning_simulation_lib_amd import dp  # noqa: E402

HBM_PEAK_GBPS = 8000.0
C, SIGMA, SEED = 1.0, dp.compute_dp_sigma(), 1


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


@torch.no_grad()
def torch_rows(t: torch.Tensor) -> torch.Tensor:
    """The per-row composition in the tensor's own dtype, noise from torch's generator."""
    rows = t.reshape(1, -1) if t.dim() <= 1 else t.reshape(t.shape[0], -1)
    norms = torch.linalg.vector_norm(rows, dim=-1, keepdim=True)
    clipped = rows / torch.clamp(norms / C, min=1)
    return (clipped + torch.randn_like(clipped) * (SIGMA * C)).reshape(t.shape)


@torch.no_grad()
def torch_parameter(parameter: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
    """The whole-dict composition: one fp64 vector, one norm, the noise, and back per tensor."""
    flat = torch.cat([v.reshape(-1).to(torch.float64) for v in parameter.values()])
    noised = torch_rows(flat)
    out, off = {}, 0
    for k, v in parameter.items():
        out[k] = noised[off : off + v.numel()].reshape(v.shape).to(v.dtype)
        off += v.numel()
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "dp_lines.jsonl")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("at least 20 runs")
    device = torch.device("cuda", 0)
    ctx = dp._context(device)
    layout = resnet18_layout()
    cases = []
    for dtype in (torch.float64, torch.float32):
        g = torch.Generator(device="cpu").manual_seed(0)
        host = {name: (torch.randn(shape, generator=g, dtype=torch.float64) * 0.05).to(dtype)
                for name, shape in zip(layout.names, layout.shapes)}
        cases.append((f"resnet18_{str(dtype).replace('torch.', '')}", host, 0))
    g = torch.Generator(device="cpu").manual_seed(1)
    cases.append(("embedding_2048x64_float32", {"feature": torch.randn(2048, 64, generator=g)}, 64))

    lines = []
    for name, host, row_len in cases:
        param = {k: v.to(device) for k, v in host.items()}
        tensors = [v.reshape(-1) for v in param.values()]
        outs = [torch.empty_like(t) for t in tensors]
        elements = sum(t.numel() for t in tensors)
        model_bytes = 3 * elements * tensors[0].element_size()

        # correctness first: the device bytes are the CPU path's
        ctx.dp_noise(tensors, outs, C, SIGMA * C, SEED, 5, None, row_len)
        assert ctx.flags() == 0
        if row_len:
            want = [dp.add_dp_noise(host["feature"], C=C, sigma=SIGMA, seed=SEED, draw=5).reshape(-1)]
        else:
            want = [v.reshape(-1) for v in dp.add_dp_noise_to_parameter(host, C=C, sigma=SIGMA, seed=SEED,
                                                                        draw=5).values()]
        assert all(torch.equal(o.cpu(), w) for o, w in zip(outs, want)), "device and CPU outputs differ"

        def k_call():
            ctx.dp_noise(tensors, outs, C, SIGMA * C, SEED, 5, None, row_len)

        if row_len:
            def p_call():
                dp.add_dp_noise(param["feature"], C=C, sigma=SIGMA, seed=SEED, draw=5)

            def b_call():
                torch_rows(param["feature"])
        else:
            def p_call():
                dp.add_dp_noise_to_parameter(param, C=C, sigma=SIGMA, seed=SEED, draw=5)

            def b_call():
                torch_parameter(param)

        legs = {"k": (events, k_call), "p": (wall, p_call), "b": (wall, b_call)}
        for _ in range(args.warmup):
            for timer, fn in legs.values():
                timer(fn, device)
        ts: dict[str, list[float]] = {k: [] for k in legs}
        for _ in range(args.runs):  # interleaved: drift hits every leg alike
            for key, (timer, fn) in legs.items():
                ts[key].append(timer(fn, device))
        assert ctx.flags() == 0
        sp = {k: spread(v) for k, v in ts.items()}
        gbps = model_bytes / sp["k"]["median_ms"] / 1e6
        line = {
            "what": "dp_noise", "case": name, "tensors": len(tensors), "elements": elements, "row_len": row_len,
            "device": torch.cuda.get_device_name(device),
            "kernel_call": sp["k"], "package_call": sp["p"], "torch_composition": sp["b"],
            "ratio_composition_over_kernel_call": sp["b"]["median_ms"] / sp["k"]["median_ms"],
            "ratio_composition_over_package_call": sp["b"]["median_ms"] / sp["p"]["median_ms"],
            "composition_spread_ms": sp["b"]["p90_ms"] - sp["b"]["p10_ms"],
            "model_bytes": model_bytes, "kernel_call_model_gbps": gbps,
            "kernel_call_share_of_hbm_peak": gbps / HBM_PEAK_GBPS,
        }
        lines.append(line)
        print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
