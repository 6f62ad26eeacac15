"""Time the secure-aggregation kernels against what a user does today and against the plain delta fold.

The ResNet-18 layout (62 tensors, 11,689,512 elements), 64 workers, fp64 out against the fp64 base, in
one process on one GPU, after warm-up, HIP events around every leg, the legs interleaved in one run,
the median with its spread (the helpers are ``sign_bench.py``'s):

  (m32, m64) ``FedAvgContext.secagg_mask`` for one client of 64 (64 seed entries), fp32 and fp64 tensors;
  (u0, u1, u8) ``FedAvgContext.secagg_unmask`` with 0, 1 and 8 of the 64 workers dropped
       (64, 126 and 504 seed entries);
  (a)  what a user does today for one client: per tensor and pair one ``torch.randint`` of int64 words,
       added or subtracted (no defined stream, so no other party could regenerate it);
  (b)  ``FedAvgContext.aggregate_delta`` on the 64 unmasked fp32 tensors: the fold without privacy.

One JSON line per kernel leg goes to --out (default profiles/secagg_lines.jsonl) with the two models:
bytes (``|A| * P * 8 + P * 8 + base`` for unmask, ``P * (esize + 8)`` for mask) over the 8.0 TB/s HBM
peak, and Philox blocks (``seed entries * P / 2``, 20 32 x 32 -> 64 products each) over an ASSUMED
product rate (one product per lane every fourth cycle: 256 CUs x 64 lanes x 2.4 GHz / 4), and which of
the two bounds the call. unmask with no dropout is compared bit for bit with the numpy composition on
one tensor before anything is timed. Not traced. No GPU, no number.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "scripts"))

from bench import resnet18_layout  # noqa: E402
from distributed_learning_simulation_lib_amd import _native  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import ClientTable, FedAvgContext, ModelLayout  # noqa: E402
from distributed_learning_simulation_lib_amd.secagg import SecAggSession, _masks  # noqa: E402
from sign_bench import CLIENTS, HBM_PEAK_GBPS, timed  # noqa: E402

PRODUCTS_PER_BLOCK = 20
ASSUMED_PRODUCTS_PER_S = 256 * 64 * 2.4e9 / 4
F, VB = 24, 40


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "secagg_lines.jsonl")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    numels = list(layout.numels)
    P = sum(numels)
    ctx, flat = FedAvgContext(layout, device), FedAvgContext(ModelLayout.flat(1, "secagg"), device)
    session = SecAggSession(7, CLIENTS)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = [torch.randn(n, generator=g, dtype=torch.float64).to(device) for n in numels]
    outs = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    plain = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    deltas = [[(torch.randn(n, generator=g) * 0.01).to(device) for n in numels] for _ in range(CLIENTS)]
    wide = [d.double() for d in deltas[0]]
    words = [[torch.empty(n, dtype=torch.int64, device=device) for n in numels] for _ in range(CLIENTS)]
    for i in range(CLIENTS):  # the round's real masked words
        flat.secagg_mask(deltas[i], words[i], 1, *session.client_table(i, 0), 0, F, VB)
    assert flat.flags() == 0
    scratch = [torch.empty(n, dtype=torch.int64, device=device) for n in numels]
    table = ClientTable(len(numels))
    for d in deltas:
        table.add_client(d, [1.0] * len(numels))
    seeds0, signs0 = session.client_table(0, 0)

    def rows_of(dropped):
        A = [i for i in range(CLIENTS) if i not in dropped]
        return A, [words[i] for i in A], session.server_table(A, dropped, 0)

    drops = {"u0": [], "u1": [63], "u8": list(range(56, 64))}
    cases = {k: rows_of(d) for k, d in drops.items()}

    def unmask(key):
        A, rows, (sd, sg) = cases[key]
        return lambda: ctx.secagg_unmask(rows, sd, sg, 0, F, float(len(A)), base, outs)

    def a_call():
        for t, (x, o) in enumerate(zip(deltas[0], scratch)):
            o.copy_((x.double() * 2.0 ** F).round().to(torch.int64))
            for sign in signs0:
                m = torch.randint(-(1 << 63), (1 << 63) - 1, o.shape, dtype=torch.int64, device=device)
                o.add_(m) if sign > 0 else o.sub_(m)

    def b_call():
        ctx.aggregate_delta(table, torch.float32, base, plain, torch.float64)

    unmask("u0")()
    assert ctx.flags() == 0
    t = 1  # a small tensor: the numpy composition on it (base + ((double)(int64)S * 2^-f) / W)
    S = _masks(*cases["u0"][2], 0, t, numels[t])
    for r in cases["u0"][1]:
        S = S + r[t].cpu().numpy().view(np.uint64)
    ref = base[t].cpu().numpy() + (S.view(np.int64).astype(np.float64) * 2.0 ** -F) / float(CLIENTS)
    assert np.array_equal(outs[t].cpu().numpy().view(np.uint64), ref.view(np.uint64)), "kernel and numpy differ"

    legs = {"m32": lambda: flat.secagg_mask(deltas[0], scratch, 1, seeds0, signs0, 0, F, VB),
            "m64": lambda: flat.secagg_mask(wide, scratch, 1, seeds0, signs0, 0, F, VB),
            "u0": unmask("u0"), "u1": unmask("u1"), "u8": unmask("u8"), "a": a_call, "b": b_call}
    sp = timed(legs, device, args.warmup, args.runs)
    lines = []
    for key in ("m32", "m64", "u0", "u1", "u8"):
        if key[0] == "m":
            entries, model_bytes = len(seeds0), P * ((4 if key == "m32" else 8) + 8)
        else:
            A, _, (sd, _) = cases[key]
            entries, model_bytes = len(sd), len(A) * P * 8 + P * 8 + P * 8
        blocks = entries * (P // 2)
        byte_ms = model_bytes / HBM_PEAK_GBPS / 1e6
        gen_ms = blocks * PRODUCTS_PER_BLOCK / ASSUMED_PRODUCTS_PER_S * 1e3
        lines.append({"what": "secagg_mask" if key[0] == "m" else "secagg_unmask", "case": key, "workers": CLIENTS,
                      "elements": P, "seed_entries": entries, "device": torch.cuda.get_device_name(device),
                      "traced": False, "time": sp[key], "model_bytes": model_bytes, "byte_bound_ms": byte_ms,
                      "philox_blocks": blocks, "generator_bound_ms_assumed_rate": gen_ms,
                      "bound": "generator" if gen_ms > byte_ms else "bytes",
                      "share_of_bound": max(gen_ms, byte_ms) / sp[key]["median_ms"],
                      "torch_randint_one_client": sp["a"], "plain_delta_fold_fp32": sp["b"],
                      "shared_tile": entries >= _native.kernel_constant("secagg_split")})
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
