"""Time the rotated 1-bit fold and client step against the plain sign kernels and against what a user
would do without them.

The ResNet-18 layout (62 tensors, 11,689,512 elements), 64 clients, fp64 out against the fp64 base, in
one process on one GPU, after warm-up, HIP events around every leg, the legs interleaved in one run,
the median with its spread (the helpers are ``sign_bench.py``'s):

  (rf) ``FedAvgContext.rsign_aggregate_delta`` over 64 rotated payloads;
  (sf) ``FedAvgContext.sign_aggregate_delta`` over 64 plain sign payloads of the same diffs;
  (df) the rotated payloads densified per client and tensor by a torch composition on the GPU (sign
       select, a Walsh-Hadamard transform level by level, the diagonal), then ``aggregate_delta``;
  (rc) ``FedAvgContext.rsign_compress`` of one client's fp32 diff with a residual;
  (sc) ``FedAvgContext.sign_compress`` of the same diff;
  (tc) the client step as a torch composition on the device tensors (its sums are torch's, not the
       contract's tree: a time, not an oracle).

One JSON line per leg goes to --out (default profiles/rsign_lines.jsonl) with the byte model of the
folds (N payloads + fp64 base in, fp64 result out) over the 8.0 TB/s HBM peak. Whole-call times from
events, not kernel times: not traced. No GPU, no number.
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
from distributed_learning_simulation_lib_amd.fedavg import (  # noqa: E402
    ClientTable, FedAvgContext, ModelLayout, RotatedSignTable, SignTable)
from distributed_learning_simulation_lib_amd.rotated import RotatedSignDelta, diagonal, geometry  # noqa: E402
from distributed_learning_simulation_lib_amd.sign import SignDelta, bit_bytes  # noqa: E402
from sign_bench import CLIENTS, HBM_PEAK_GBPS, timed  # noqa: E402

SEED, DRAW = 0x5EED, 0


def hadamard(x: torch.Tensor) -> torch.Tensor:
    """H_B of every row of x ([nb, B]) on its device, level by level."""
    nb, B = x.shape
    h = 1
    while h < B:
        v = x.view(nb, B // (2 * h), 2, h)
        x = torch.stack((v[:, :, 0] + v[:, :, 1], v[:, :, 0] - v[:, :, 1]), dim=2).view(nb, B)
        h *= 2
    return x


def unpack(bits: torch.Tensor, nb: int, B: int) -> torch.Tensor:
    e = torch.arange(nb * B, device=bits.device)
    return (((bits.to(torch.int32)[e >> 3] >> (e & 7).to(torch.int32)) & 1).bool()).view(nb, B)


def user_dense(d: RotatedSignDelta, D: torch.Tensor) -> torch.Tensor:
    B, nb, _ = geometry(d.numel)
    s = d.scales.to(torch.float64)[:, None].expand(nb, B)
    z = hadamard(torch.where(unpack(d.bits, nb, B), -s, s)).view(-1)
    return torch.where(D, -z, z)[: d.numel].to(torch.float32)


def user_compress(x: torch.Tensor, e: torch.Tensor, D: torch.Tensor):
    total = x + e
    n = total.numel()
    B, nb, n_pad = geometry(n)
    u = torch.zeros(n_pad, dtype=torch.float64, device=x.device)
    u[:n] = torch.where(D[:n], -total, total)
    y = hadamard(u.view(nb, B))
    scale = (y.abs().sum(dim=1) / (B * B)).to(torch.float32).to(torch.float64)[:, None].expand(nb, B)
    z = hadamard(torch.where(torch.signbit(y), -scale, scale)).view(-1)
    return torch.signbit(y), total - torch.where(D, -z, z)[:n].to(x.dtype)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "rsign_lines.jsonl")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    numels = list(layout.numels)
    P, T = sum(numels), len(numels)
    geo = [geometry(n) for n in numels]
    ctx, flat = FedAvgContext(layout, device), FedAvgContext(ModelLayout.flat(1, "rsign"), device)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = [torch.randn(n, generator=g, dtype=torch.float64).to(device) for n in numels]
    outs = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    deltas = [[(torch.randn(n, generator=g) * 0.01).to(device) for n in numels] for _ in range(CLIENTS)]
    errors = [torch.zeros_like(d) for d in deltas[0]]
    residual = [torch.empty_like(d) for d in deltas[0]]
    weights = [1.0 + i for i in range(CLIENTS)]
    divisor = float(sum(weights))
    diag = [torch.from_numpy(diagonal(SEED, DRAW, t, n_pad)).to(device) for t, (_, _, n_pad) in enumerate(geo)]

    def rotated_buffers():
        return ([torch.empty(n_pad // 8, dtype=torch.uint8, device=device) for _, _, n_pad in geo],
                [torch.empty(nb, dtype=torch.float32, device=device) for _, nb, _ in geo])

    def sign_buffers():
        return ([torch.empty(bit_bytes(n), dtype=torch.uint8, device=device) for n in numels],
                [torch.empty((), dtype=torch.float32, device=device) for _ in numels])

    # the round's real payloads, from the client steps themselves
    rrows, srows = [], []
    for d in deltas:
        bits, scales = rotated_buffers()
        flat.rsign_compress(d, None, bits, scales, residual, seed=SEED, draw=DRAW, mode="unbiased")
        rrows.append([RotatedSignDelta(b, s, (n,), SEED, DRAW, t) for t, (b, s, n) in enumerate(zip(bits, scales, numels))])
        bits, scales = sign_buffers()
        flat.sign_compress(d, None, bits, scales, residual)
        srows.append([SignDelta(b, s, (n,)) for b, s, n in zip(bits, scales, numels)])
    assert flat.flags() == 0
    rtable, stable = RotatedSignTable(rrows, layout, device), SignTable(srows, layout, device)
    rscratch, sscratch = rotated_buffers(), sign_buffers()

    def densify_then_fold():
        table = ClientTable(T)
        keep = []
        for row, w in zip(rrows, weights):
            keep.append([user_dense(d, D) for d, D in zip(row, diag)])
            table.add_client(keep[-1], [w] * T)
        ctx.aggregate_delta(table, torch.float32, base, outs, torch.float64)

    legs = {
        "rf": lambda: ctx.rsign_aggregate_delta(rtable, weights, divisor, base, outs),
        "sf": lambda: ctx.sign_aggregate_delta(stable, weights, divisor, base, outs),
        "df": densify_then_fold,
        "rc": lambda: flat.rsign_compress(deltas[0], errors, *rscratch, residual, seed=SEED, draw=DRAW, mode="mse"),
        "sc": lambda: flat.sign_compress(deltas[0], errors, *sscratch, residual),
        "tc": lambda: [user_compress(x, e, D) for x, e, D in zip(deltas[0], errors, diag)],
    }
    sp = timed(legs, device, args.warmup, args.runs)
    assert ctx.flags() == 0 and flat.flags() == 0
    payload = {"rf": CLIENTS * sum(n_pad // 8 + 4 * nb for _, nb, n_pad in geo),
               "sf": CLIENTS * sum(bit_bytes(n) + 4 for n in numels), "df": CLIENTS * sum(n_pad // 8 + 4 * nb for _, nb, n_pad in geo)}
    what = {"rf": "rsign_aggregate_delta", "sf": "sign_aggregate_delta", "df": "torch to_dense per client + aggregate_delta fp32",
            "rc": "rsign_compress fp32", "sc": "sign_compress fp32", "tc": "torch composition of the rotated client step"}
    lines = []
    for key in legs:
        line = {"what": what[key], "case": key, "clients": CLIENTS, "elements": P,
                "device": torch.cuda.get_device_name(device), "traced": False, "time": sp[key]}
        if key in payload:
            model_bytes = payload[key] + 2 * P * 8
            byte_ms = model_bytes / HBM_PEAK_GBPS / 1e6
            line.update({"payload_bytes": payload[key], "model_bytes": model_bytes, "byte_bound_ms": byte_ms,
                         "share_of_hbm_peak": byte_ms / sp[key]["median_ms"]})
        lines.append(line)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
