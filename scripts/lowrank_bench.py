"""Time a round of low-rank clients against what it replaces.

The ResNet-18 layout (62 tensors, 11,689,512 elements), 64 clients, rank 4: every tensor of two or more
dimensions travels as fp32 factors, the 1-D tensors (norms, biases) dense. One process on one GPU, after
warm-up, HIP events around every leg, the legs interleaved in one run, the median with its spread:

  (l)  the new round: ``FedAvgContext.lowrank_aggregate_delta`` over a ``LowRankTable`` built once for
       the matrices, then ``aggregate_delta`` for the 1-D tensors on their own context;
  (l8) eight low-rank folds back to back between one pair of events, per call: the kernel's time where
       the kernel is longer than a call's host work;
  (u)  what a user does today: ``to_dense()`` per client and matrix, then ``aggregate_delta`` on the
       whole layout;
  (a)  ``aggregate_delta`` alone on the pre-densified tensors (the densification not timed).

One JSON line goes to --out (default profiles/lowrank_lines.jsonl) with each ratio as measured, the
operation model (N r m n fp64 multiply-adds per matrix) over the 78.6 TFLOP/s fp64 matrix peak and the
byte model (the factors once, base and result) over the 8.0 TB/s HBM peak, and the share of the bound
that applies. Not traced. No GPU, no number.

``--leg compress`` times the client step instead (``compress_lines``) and appends its lines to --out.
"""

from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from bench import resnet18_layout  # noqa: E402
from distributed_learning_simulation_lib_amd import LowRankDelta, _native  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import ClientTable, FedAvgContext, LowRankTable, ModelLayout  # noqa: E402

HBM_PEAK_GBPS = 8000.0
FP64_MATRIX_PEAK_GFLOPS = 78600.0
CLIENTS = 64
RANK = 4
BURST = 8


def spread(ts: list[float]) -> dict:
    s = sorted(ts)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "runs": len(s)}


def events(fn, device) -> float:
    stream = torch.cuda.current_stream(device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def compress_lines(args, device) -> None:
    """The client step: one client's ResNet-18 diff at rank 4, fp32 and fp64, with and without
    residuals. (k) ``FedAvgContext.lowrank_compress`` over all compressible tensors into
    preallocated outputs; (t) ``_lowrank_compress_torch`` per tensor on the same device tensors. The
    byte model is delta (+ error) read three times and the residual written once. One JSON line
    per case is appended to --out."""
    from distributed_learning_simulation_lib_amd.lowrank import _lowrank_compress_torch, _shape
    from distributed_learning_simulation_lib_amd.sign import _context

    layout = resnet18_layout()
    g = torch.Generator(device="cpu").manual_seed(1)
    shapes = [s for s in layout.shapes if len(s) >= 2 and _shape(torch.empty(s, device="meta"), RANK) is not None]
    ctx = _context(device)
    for dtype in (torch.float32, torch.float64):
        deltas = [(torch.randn(*s, generator=g) * 0.01).to(dtype).to(device) for s in shapes]
        errors = [(torch.randn(*s, generator=g) * 0.001).to(dtype).to(device) for s in shapes]
        starts = [torch.randn(RANK, d.numel() // d.shape[0], generator=g).to(dtype).to(device) for d in deltas]
        lefts = [torch.empty(d.shape[0], RANK, dtype=dtype, device=device) for d in deltas]
        rights = [torch.empty_like(q) for q in starts]
        res = [torch.empty_like(d) for d in deltas]
        for with_error in (False, True):
            errs = errors if with_error else None

            def k_call():
                ctx.lowrank_compress(deltas, errs, starts, lefts, rights, res)

            def t_call():
                for i, d in enumerate(deltas):
                    _lowrank_compress_torch(d, RANK, starts[i], errs[i] if errs else None)

            legs = {"k": k_call, "t": t_call}
            for _ in range(args.warmup):
                for fn in legs.values():
                    events(fn, device)
            assert ctx.flags() == 0
            ts: dict[str, list[float]] = {k: [] for k in legs}
            for _ in range(args.runs):  # interleaved: drift hits every leg alike
                for key, fn in legs.items():
                    ts[key].append(events(fn, device))
            sp = {k: spread(v) for k, v in ts.items()}
            p = sum(d.numel() for d in deltas)
            model_bytes = deltas[0].element_size() * p * (3 * (2 if with_error else 1) + 1)
            line = {"what": "lowrank_compress", "case": f"resnet18_{str(dtype).split('.')[-1]}", "rank": RANK,
                    "with_residuals": with_error, "tensors": len(deltas), "elements": p,
                    "device": torch.cuda.get_device_name(device), "traced": False, "kernel_call": sp["k"],
                    "torch_per_tensor": sp["t"], "ratio_torch_over_kernel": sp["t"]["median_ms"] / sp["k"]["median_ms"],
                    "model_bytes": model_bytes, "bound_ms_bytes": model_bytes / HBM_PEAK_GBPS / 1e6,
                    "share_of_byte_bound": model_bytes / HBM_PEAK_GBPS / 1e6 / sp["k"]["median_ms"],
                    "launches": 5, **{k: _native.kernel_constant(k) for k in
                                      ("lowrank_chunk_cols", "lowrank_chunk_rows", "lowrank_ortho_lds_rows")}}
            print(json.dumps(line))
            args.out.parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "lowrank_lines.jsonl")
    ap.add_argument("--leg", choices=("fold", "compress"), default="fold",
                    help="fold: the server round (rewrites --out); compress: the client step (appends to --out)")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    if args.leg == "compress":
        compress_lines(args, device)
        return
    layout = resnet18_layout()
    T = layout.num_segments
    low = [i for i, s in enumerate(layout.shapes) if len(s) >= 2]
    flat = [i for i in range(T) if i not in low]
    sub = {k: ModelLayout(names=tuple(layout.names[i] for i in idx), shapes=tuple(layout.shapes[i] for i in idx))
           for k, idx in (("low", low), ("flat", flat))}
    ctx = {"all": FedAvgContext(layout, device), "low": FedAvgContext(sub["low"], device),
           "flat": FedAvgContext(sub["flat"], device)}
    g = torch.Generator(device="cpu").manual_seed(0)
    base = [torch.randn(n, generator=g, dtype=torch.float64).to(device) for n in layout.numels]
    outs = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
    ref = [torch.empty(n, dtype=torch.float64, device=device) for n in layout.numels]
    weights = [1.0 + (i % 7) / 8 for i in range(CLIENTS)]
    divisor = float(sum(weights))

    def factors(shape):
        m, n = shape[0], math.prod(shape[1:])
        return LowRankDelta((torch.randn(m, RANK, generator=g) * 0.1).to(device), (torch.randn(RANK, n, generator=g) * 0.1).to(device), shape)

    rows = [[factors(layout.shapes[i]) for i in low] for _ in range(CLIENTS)]
    small = [[(torch.randn(layout.numels[i], generator=g) * 0.01).to(device) for i in flat] for _ in range(CLIENTS)]
    table = LowRankTable(rows, sub["low"], device)
    flat_table = ClientTable(len(flat))
    for row, w in zip(small, weights):
        flat_table.add_client(row, [w] * len(flat))

    def whole_table() -> ClientTable:
        t = ClientTable(T)
        for lr, sm, w in zip(rows, small, weights):
            row: list = [None] * T
            for j, i in enumerate(low):
                row[i] = lr[j].to_dense().reshape(-1).contiguous()
            for j, i in enumerate(flat):
                row[i] = sm[j]
            t.add_client(row, [w] * T)
        return t

    dense = whole_table()
    pick = lambda xs, idx: [xs[i] for i in idx]  # noqa: E731

    def fold():
        ctx["low"].lowrank_aggregate_delta(table, weights, divisor, pick(base, low), pick(outs, low))

    def l_call():
        fold()
        ctx["flat"].aggregate_delta(flat_table, torch.float32, pick(base, flat), pick(outs, flat), torch.float64)
        ctx["flat"].reset()

    def l_burst():
        for _ in range(BURST):
            fold()

    def a_call(t=dense):
        ctx["all"].aggregate_delta(t, torch.float32, base, ref, torch.float64)
        ctx["all"].reset()

    def u_call():
        a_call(whole_table())

    l_call()
    a_call()
    assert ctx["low"].flags() == 0 and ctx["flat"].flags() == 0 and ctx["all"].flags() == 0
    worst = max(float((o - r).abs().max()) for o, r in zip(outs, ref))  # two contracts: close, not the same bits
    legs = {"l": l_call, "l8": l_burst, "u": u_call, "a": a_call}
    for _ in range(args.warmup):
        for fn in legs.values():
            events(fn, device)
    ts: dict[str, list[float]] = {k: [] for k in legs}
    for _ in range(args.runs):  # interleaved: drift hits every leg alike
        for key, fn in legs.items():
            ts[key].append(events(fn, device))
    sp = {k: spread(v) for k, v in ts.items()}
    sp["l8"] = {k: v / BURST if k != "runs" else v for k, v in sp["l8"].items()}
    macs = sum(CLIENTS * RANK * layout.numels[i] for i in low)
    p_low = sum(layout.numels[i] for i in low)
    factor_bytes = 4 * CLIENTS * sum(RANK * (layout.shapes[i][0] + layout.numels[i] // layout.shapes[i][0]) for i in low)
    model_bytes = factor_bytes + 16 * p_low
    t_ops, t_bytes = 2 * macs / FP64_MATRIX_PEAK_GFLOPS / 1e6, model_bytes / HBM_PEAK_GBPS / 1e6
    line = {"what": "lowrank_aggregate_delta", "case": "resnet18_float32", "clients": CLIENTS, "rank": RANK,
            "elements": layout.total_numel, "lowrank_elements": p_low, "device": torch.cuda.get_device_name(device),
            "traced": False, "lowrank_round": sp["l"], "lowrank_fold_in_burst_of_8": sp["l8"],
            "to_dense_then_dense_delta_fold": sp["u"], "dense_delta_fold_predensified": sp["a"],
            "ratio_user_over_lowrank_round": sp["u"]["median_ms"] / sp["l"]["median_ms"],
            "ratio_predensified_over_lowrank_round": sp["a"]["median_ms"] / sp["l"]["median_ms"],
            "max_abs_difference_to_dense_fold": worst,
            "model_multiply_adds": macs, "model_bytes": model_bytes, "factor_bytes": factor_bytes,
            "dense_model_bytes": 4 * CLIENTS * layout.total_numel + 16 * layout.total_numel,
            "bound_ms_fp64_matrix": t_ops, "bound_ms_bytes": t_bytes, "bound": "fp64 matrix" if t_ops > t_bytes else "bytes",
            "burst_share_of_bound": max(t_ops, t_bytes) / sp["l8"]["median_ms"],
            "burst_share_of_fp64_matrix_peak": t_ops / sp["l8"]["median_ms"],
            "lowrank_tm": _native.kernel_constant("lowrank_tm"), "lowrank_tn": _native.kernel_constant("lowrank_tn"),
            "lowrank_kstep": _native.kernel_constant("lowrank_kstep")}
    print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
