"""Time 1-bit sign compression and its fold against what they replace.

The ResNet-18 layout (62 tensors, 11,689,512 elements), 64 clients, scale dtypes fp32, fp16, bf16 and
fp64, in one process on one GPU, after warm-up, HIP events around every leg, the legs interleaved in
one run, the median with its spread:

  the fold, fp64 out against the fp64 base:
  (f)  ``FedAvgContext.sign_aggregate_delta`` over a ``SignTable`` built once;
  (f8) eight such calls back to back between one pair of events, per call: the host work of a call
       overlaps the kernel of the one before, so this is the kernel's time where the kernel is longer;
  (a)  ``FedAvgContext.aggregate_delta`` on the pre-densified tensors (the densification not timed);
  (u)  what a user does today: ``to_dense()`` per client and tensor, then the dense fold (a);

  the client step on one client's diff with a residual:
  (c)  ``FedAvgContext.sign_compress`` into resident outputs, and (c8) eight of them back to back, per call;
  (t)  the torch composition on the same device tensors, per tensor: add, ``abs().sum()``, a divide, a
       sign test, a select, a subtract and a bit-pack (torch's own summation order, not the pinned one);
  (k)  ``FedAvgContext.topk_sparsify`` at ratio 1 % on the same tensors, for scale.

One JSON line per dtype and part goes to --out (default profiles/sign_lines.jsonl) with the byte
model (what the kernels read and write of the tensors: bits, base and result for the fold; delta and
error twice, residual and bits for the client step) over the 8.0 TB/s HBM peak, the fp64 operation
model of the fold (3 per client and element) over the 39.3 T/s peak of separately rounded fp64
operations, the bound that applies and the share reached. The fold's result is compared bit for bit
with (a) before anything is timed. Not traced. No GPU, no number.
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
from distributed_learning_simulation_lib_amd import _native, sign  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import ClientTable, FedAvgContext, SignTable  # noqa: E402
from distributed_learning_simulation_lib_amd.sparse import topk_count  # noqa: E402

HBM_PEAK_GBPS = 8000.0
FP64_PEAK_GOPS = 39300.0  # 78.6 TFLOP/s of vector FMA = 39.3 T separately rounded operations per second
CLIENTS = 64
BURST = 8


def spread(ts: list[float]) -> dict:
    s = sorted(ts)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "p10_ms": s[len(s) // 10], "p90_ms": s[-1 - len(s) // 10], "runs": len(s)}


def events(fn, device) -> float:
    stream = torch.cuda.current_stream(device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def timed(legs: dict, device, warmup: int, runs: int) -> dict:
    for _ in range(warmup):
        for fn in legs.values():
            events(fn, device)
    ts: dict[str, list[float]] = {k: [] for k in legs}
    for _ in range(runs):  # interleaved: drift hits every leg alike
        for key, fn in legs.items():
            ts[key].append(events(fn, device))
    return {k: spread(v) for k, v in ts.items()}


def user_compress(d: torch.Tensor, e: torch.Tensor):
    total = d + e
    scale = total.abs().sum(dtype=torch.float64).div(total.numel()).to(d.dtype)
    neg = torch.signbit(total)
    residual = total - torch.where(neg, -scale, scale)
    return sign._pack(neg), scale, residual


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-user-leg", action="store_true", help="leave (u) out: a tuning build's run")
    ap.add_argument("--fold-only", action="store_true", help="leave the client step out: a tuning build's run")
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "sign_lines.jsonl")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    numels = list(layout.numels)
    P = sum(numels)
    ctx = FedAvgContext(layout, device)
    free = sign._context(device)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = [torch.randn(n, generator=g, dtype=torch.float64).to(device) for n in numels]
    outs = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    ref = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    weights = [1.0 + (i % 7) / 8 for i in range(CLIENTS)]
    divisor = float(sum(weights))
    lines = []
    name = torch.cuda.get_device_name(device)
    for dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        tag = str(dtype).replace("torch.", "")
        size = torch.empty(0, dtype=dtype).element_size()
        rows = [[sign.SignDelta(torch.randint(0, 256, (sign.bit_bytes(n),), generator=g, dtype=torch.uint8).to(device),
                                (torch.rand((), generator=g) * 0.01).to(dtype).to(device), (n,)) for n in numels]
                for _ in range(CLIENTS)]
        table = SignTable(rows, layout, device)
        dense = ClientTable(len(numels))
        for row, w in zip(rows, weights):
            dense.add_client([d.to_dense().contiguous() for d in row], [w] * len(numels))

        def f_call():
            ctx.sign_aggregate_delta(table, weights, divisor, base, outs)

        def a_call(t=dense):
            ctx.aggregate_delta(t, dtype, base, ref, torch.float64)
            ctx.reset()

        def u_call():
            t = ClientTable(len(numels))
            for row, w in zip(rows, weights):
                t.add_client([d.to_dense().contiguous() for d in row], [w] * len(numels))
            a_call(t)

        f_call()
        a_call()
        assert ctx.flags() == 0
        for o, r in zip(outs, ref):
            assert torch.equal(o.view(torch.int64), r.view(torch.int64)), "the sign fold and the dense delta fold differ"
        def f_burst():
            for _ in range(BURST):
                f_call()

        legs = {"f": f_call, "f8": f_burst, "a": a_call}
        if not args.skip_user_leg:
            legs["u"] = u_call
        sp = timed(legs, device, args.warmup, args.runs)
        sp["f8"] = {k: v / BURST if k != "runs" else v for k, v in sp["f8"].items()}
        sp.setdefault("u", None)
        fold_bytes = CLIENTS * sum(sign.bit_bytes(n) for n in numels) + 16 * P
        fold_ops = 3 * CLIENTS * P
        t_bytes, t_ops = fold_bytes / HBM_PEAK_GBPS / 1e6, fold_ops / FP64_PEAK_GOPS / 1e6
        line = {"what": "sign_aggregate_delta", "case": f"resnet18_{tag}", "clients": CLIENTS, "elements": P,
                "device": name, "traced": False, "sign_fold": sp["f"], "dense_delta_fold_predensified": sp["a"],
                "to_dense_then_dense_delta_fold": sp["u"],
                "ratio_dense_over_sign": sp["a"]["median_ms"] / sp["f"]["median_ms"],
                "sign_fold_in_burst_of_8": sp["f8"],
                "ratio_user_over_sign": sp["u"]["median_ms"] / sp["f"]["median_ms"] if sp["u"] else None,
                "model_bytes": fold_bytes, "model_fp64_ops": fold_ops, "bound_ms_bytes": t_bytes, "bound_ms_fp64": t_ops,
                "bound": "fp64" if t_ops > t_bytes else "bytes",
                "share_of_bound": max(t_bytes, t_ops) / sp["f"]["median_ms"],
                "burst_share_of_bound": max(t_bytes, t_ops) / sp["f8"]["median_ms"],
                "sign_words": _native.kernel_constant("sign_words"), "sign_batch": _native.kernel_constant("sign_batch"),
                "dense_model_bytes": CLIENTS * P * size + 16 * P}
        lines.append(line)
        print(json.dumps(line))
        del rows, table, dense

        if args.fold_only:
            continue
        # the client step
        delta = [(torch.randn(n, generator=g) * 0.1).to(dtype).to(device) for n in numels]
        error = [(torch.randn(n, generator=g) * 0.03).to(dtype).to(device) for n in numels]
        bits = [torch.empty(sign.bit_bytes(n), dtype=torch.uint8, device=device) for n in numels]
        scales = [torch.empty((), dtype=dtype, device=device) for _ in numels]
        res = [torch.empty_like(d) for d in delta]
        keeps = [topk_count(n, ratio=0.01) for n in numels]
        idx = [torch.empty(k, dtype=torch.int32, device=device) for k in keeps]
        val = [torch.empty(k, dtype=dtype, device=device) for k in keeps]

        def c_call():
            free.sign_compress(delta, error, bits, scales, res)

        def t_call():
            for d, e in zip(delta, error):
                user_compress(d, e)

        def k_call():
            free.topk_sparsify(delta, error, keeps, idx, val, res)

        def c_burst():
            for _ in range(BURST):
                c_call()

        sp = timed({"c": c_call, "c8": c_burst, "t": t_call, "k": k_call}, device, args.warmup, args.runs)
        sp["c8"] = {k: v / BURST if k != "runs" else v for k, v in sp["c8"].items()}
        c_bytes = P * size * 5 + sum(sign.bit_bytes(n) for n in numels)
        gbps = c_bytes / sp["c8"]["median_ms"] / 1e6
        line = {"what": "sign_compress", "case": f"resnet18_{tag}", "tensors": len(numels), "elements": P, "device": name,
                "traced": False, "sign_compress": sp["c"], "sign_compress_in_burst_of_8": sp["c8"], "torch_composition": sp["t"], "topk_sparsify_1pct": sp["k"],
                "ratio_composition_over_kernel_call": sp["t"]["median_ms"] / sp["c"]["median_ms"],
                "ratio_topk_over_kernel_call": sp["k"]["median_ms"] / sp["c"]["median_ms"],
                "model_bytes": c_bytes, "bound": "bytes", "burst_model_gbps": gbps,
                "burst_share_of_bound": gbps / HBM_PEAK_GBPS}
        lines.append(line)
        print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
