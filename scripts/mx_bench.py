"""Time the MX fold and client step against the dense fp16 delta fold.

The ResNet-18 layout (62 tensors, 11,689,512 elements), 64 clients, fp64 out against the fp64 base, in
one process on one GPU, after warm-up, HIP events around every leg, the legs interleaved in one run,
the median with its spread (the helpers are ``sign_bench.py``'s):

  (f8, f4) ``FedAvgContext.mx_aggregate_delta`` over 64 MXFP8 / MXFP4 payloads;
  (d16)    ``FedAvgContext.aggregate_delta`` on the same deltas densified into fp16;
  (c8, c4) ``FedAvgContext.mx_compress`` of one client's fp32 diff with a residual, into MXFP8 / MXFP4.

One JSON line per leg goes to --out (default profiles/mx_lines.jsonl) with the payload bytes read
(codes and scale bytes of all clients; for d16 the fp16 tensors) and that figure over the call's time,
the byte model (payload + fp64 base + fp64 out; for the client step delta, error, residual, codes and
scales) over the 8.0 TB/s HBM peak, the operation model of the fold (five separately rounded fp64
operations per client and element: widen, scale, add, multiply, add) over the 39.3 T/s fp64 vector
rate, and which of the two bounds the call. The f8 fold is compared bit for bit with d16's inputs
densified exactly (fp64) on one tensor before anything is timed. Whole-call times from events, not
kernel times: not traced. No GPU, no number.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "scripts"))

from bench import resnet18_layout  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import ClientTable, FedAvgContext, ModelLayout, MXTable  # noqa: E402
from distributed_learning_simulation_lib_amd.mx import MXDelta, code_bytes  # noqa: E402
from sign_bench import CLIENTS, FP64_PEAK_GOPS, HBM_PEAK_GBPS, timed  # noqa: E402

FOLD_OPS = 5


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "mx_lines.jsonl")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    numels = list(layout.numels)
    P, T = sum(numels), len(numels)
    ctx, flat = FedAvgContext(layout, device), FedAvgContext(ModelLayout.flat(1, "mx"), device)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = [torch.randn(n, generator=g, dtype=torch.float64).to(device) for n in numels]
    outs = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    deltas = [[(torch.randn(n, generator=g) * 0.01).to(device) for n in numels] for _ in range(CLIENTS)]
    errors = [torch.zeros_like(d) for d in deltas[0]]
    weights = [1.0 + i for i in range(CLIENTS)]
    divisor = float(sum(weights))

    # the round's real payloads, from the client step itself
    rows, scratch = {}, {}
    for fmt in ("mxfp8", "mxfp4"):
        rows[fmt] = []
        for d in deltas:
            codes = [torch.empty(code_bytes(n, fmt), dtype=torch.uint8, device=device) for n in numels]
            scales = [torch.empty((n + 31) // 32, dtype=torch.uint8, device=device) for n in numels]
            flat.mx_compress(d, None, codes, scales, [torch.empty_like(x) for x in d], fmt)
            rows[fmt].append([MXDelta(c, s, (n,), fmt) for c, s, n in zip(codes, scales, numels)])
        scratch[fmt] = ([torch.empty_like(r.codes) for r in rows[fmt][0]], [torch.empty_like(r.scales) for r in rows[fmt][0]])
    assert flat.flags() == 0
    residual = [torch.empty_like(d) for d in deltas[0]]
    tables = {fmt: MXTable(rows[fmt], layout, device) for fmt in rows}
    half = ClientTable(T)
    for row, w in zip(rows["mxfp8"], weights):  # the same deltas, dense fp16 (values below the fp16 range flush)
        half.add_client([r.to_dense(torch.float16).reshape(-1) for r in row], [w] * T)

    # before anything is timed: the f8 fold against the dense fold of its exactly densified inputs
    exact = ClientTable(T)
    for row, w in zip(rows["mxfp8"], weights):
        exact.add_client([r.to_dense(torch.float64).reshape(-1) for r in row], [w] * T)
    want = [torch.empty_like(o) for o in outs]
    ctx.aggregate_delta(exact, torch.float64, base, want, torch.float64)
    ctx.mx_aggregate_delta(tables["mxfp8"], weights, divisor, base, outs)
    assert ctx.flags() == 0
    assert all(torch.equal(o.view(torch.int64), w.view(torch.int64)) for o, w in zip(outs, want)), "mx and dense folds differ"
    ctx.reset()
    del exact, want

    legs = {
        "f8": lambda: ctx.mx_aggregate_delta(tables["mxfp8"], weights, divisor, base, outs),
        "f4": lambda: ctx.mx_aggregate_delta(tables["mxfp4"], weights, divisor, base, outs),
        "d16": lambda: ctx.aggregate_delta(half, torch.float16, base, outs, torch.float64),
        "c8": lambda: flat.mx_compress(deltas[0], errors, *scratch["mxfp8"], residual, "mxfp8"),
        "c4": lambda: flat.mx_compress(deltas[0], errors, *scratch["mxfp4"], residual, "mxfp4"),
    }
    sp = timed(legs, device, args.warmup, args.runs)
    blocks = sum((n + 31) // 32 for n in numels)
    payload = {"f8": CLIENTS * (32 * blocks + blocks), "f4": CLIENTS * (16 * blocks + blocks), "d16": CLIENTS * P * 2}
    lines = []
    for key in ("f8", "f4", "d16"):
        model_bytes = payload[key] + 2 * P * 8
        byte_ms = model_bytes / HBM_PEAK_GBPS / 1e6
        op_ms = FOLD_OPS * CLIENTS * P / FP64_PEAK_GOPS / 1e6
        ms = sp[key]["median_ms"]
        lines.append({"what": "mx_aggregate_delta" if key != "d16" else "aggregate_delta fp16", "case": key,
                      "clients": CLIENTS, "elements": P, "device": torch.cuda.get_device_name(device), "traced": False,
                      "time": sp[key], "payload_bytes": payload[key], "payload_gbps": payload[key] / ms / 1e6,
                      "model_bytes": model_bytes, "byte_bound_ms": byte_ms, "share_of_hbm_peak": byte_ms / ms,
                      **({} if key == "d16" else {"op_bound_ms": op_ms, "bound": "operations" if op_ms > byte_ms else "bytes",
                                                  "share_of_bound": max(op_ms, byte_ms) / ms})})
    for key, per in (("c8", 32), ("c4", 16)):
        model_bytes = 3 * P * 4 + per * blocks + blocks
        ms = sp[key]["median_ms"]
        lines.append({"what": "mx_compress fp32", "case": key, "elements": P,
                      "device": torch.cuda.get_device_name(device), "traced": False, "time": sp[key],
                      "model_bytes": model_bytes, "byte_bound_ms": model_bytes / HBM_PEAK_GBPS / 1e6,
                      "share_of_hbm_peak": model_bytes / HBM_PEAK_GBPS / 1e6 / ms})
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
