"""Time signSGD's majority vote against the existing sign fold and against torch.

The ResNet-18 layout (62 tensors, 11,689,512 elements), 64 clients, fp64 out against the fp64 base,
in one process on one GPU, after warm-up, HIP events around every leg, the legs interleaved in one
run, the median with its spread (the helpers are ``sign_bench.py``'s):

  (v)  ``FedAvgContext.sign_majority_vote`` over a ``SignBitTable`` built once;
  (v8) eight such calls back to back between one pair of events, per call: the host work of a call
       overlaps the kernel of the one before, so this is the kernel's time where the kernel is longer;
  (m)  the same with both packed masks asked for, in a burst of eight, per call;
  (f)  ``FedAvgContext.sign_aggregate_delta`` on the same bits: the existing kernel with the same input
       bytes, and (f8) its burst of eight, per call;
  (t)  what a user does today on the device: per tensor, unpack every client's bits, an integer sum,
       two compares, one add.

One JSON line goes to --out (default profiles/sign_vote_lines.jsonl) with the byte model (the bits, 8
bytes of base and 8 bytes of result per element; the masks add a quarter byte) over the 8.0 TB/s HBM
peak and the share reached. The vote's result is compared bit for bit with (t) before anything is
timed. Not traced. No GPU, no number.
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
from distributed_learning_simulation_lib_amd import _native, sign  # noqa: E402
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, SignBitTable, SignTable  # noqa: E402
from sign_bench import BURST, CLIENTS, HBM_PEAK_GBPS, timed  # noqa: E402

STEP = 0.01


def torch_vote(bits: torch.Tensor, base: torch.Tensor, shifts: torch.Tensor) -> torch.Tensor:
    """``bits`` is uint8 [n, bytes]: unpack, sum over the clients, compare, add."""
    n = bits.shape[0]
    unpacked = (bits.unsqueeze(-1) >> shifts) & 1           # [n, bytes, 8]
    c = unpacked.sum(dim=0, dtype=torch.int32).reshape(-1)[: base.numel()]
    return torch.where(2 * c > n, base - STEP, torch.where(2 * c < n, base + STEP, base))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "sign_vote_lines.jsonl")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    layout = resnet18_layout()
    numels = list(layout.numels)
    P, T = sum(numels), len(numels)
    ctx = FedAvgContext(layout, device)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = [torch.randn(n, generator=g, dtype=torch.float64).to(device) for n in numels]
    outs = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    fold = [torch.empty(n, dtype=torch.float64, device=device) for n in numels]
    negs = [torch.empty(sign.bit_bytes(n), dtype=torch.uint8, device=device) for n in numels]
    ties = [torch.empty(sign.bit_bytes(n), dtype=torch.uint8, device=device) for n in numels]
    # a tensor's clients are the rows of one upload, so the torch leg has them stacked for free
    stacked = [torch.randint(0, 256, (CLIENTS, sign.bit_bytes(n)), generator=g, dtype=torch.uint8).to(device) for n in numels]
    scale = torch.tensor(STEP, dtype=torch.float32, device=device)
    rows = [[sign.SignDelta(stacked[t][i], scale, (n,)) for t, n in enumerate(numels)] for i in range(CLIENTS)]
    table, both = SignBitTable(rows, layout, device), SignTable(rows, layout, device)
    steps, weights = [STEP] * T, [1.0] * CLIENTS
    shifts = torch.arange(8, dtype=torch.uint8, device=device)

    def v_call():
        ctx.sign_majority_vote(table, steps, base, outs)

    def m_call():
        ctx.sign_majority_vote(table, steps, base, outs, neg_bits=negs, tie_bits=ties)

    def f_call():
        ctx.sign_aggregate_delta(both, weights, float(CLIENTS), base, fold)

    def t_call():
        return [torch_vote(b, z, shifts) for b, z in zip(stacked, base)]

    def burst(fn):
        def run():
            for _ in range(BURST):
                fn()
        return run

    v_call()
    assert ctx.flags() == 0
    for o, r in zip(outs, t_call()):
        assert torch.equal(o.view(torch.int64), r.view(torch.int64)), "the vote kernel and the torch composition differ"
    sp = timed({"v": v_call, "v8": burst(v_call), "m8": burst(m_call), "f": f_call, "f8": burst(f_call), "t": t_call},
               device, args.warmup, args.runs)
    for k in ("v8", "m8", "f8"):
        sp[k] = {key: v / BURST if key != "runs" else v for key, v in sp[k].items()}
    bit_total = sum(sign.bit_bytes(n) for n in numels)
    model = CLIENTS * bit_total + 16 * P
    bound = model / HBM_PEAK_GBPS / 1e6
    line = {"what": "sign_majority_vote", "case": "resnet18_out64", "clients": CLIENTS, "elements": P,
            "device": torch.cuda.get_device_name(device), "traced": False,
            "vote": sp["v"], "vote_in_burst_of_8": sp["v8"], "vote_with_masks_in_burst_of_8": sp["m8"],
            "sign_fold_same_bits": sp["f"], "sign_fold_in_burst_of_8": sp["f8"], "torch_composition": sp["t"],
            "ratio_fold_over_vote_burst": sp["f8"]["median_ms"] / sp["v8"]["median_ms"],
            "ratio_torch_over_vote": sp["t"]["median_ms"] / sp["v"]["median_ms"],
            "model_bytes": model, "model_bytes_with_masks": model + 2 * bit_total, "bound": "bytes", "bound_ms": bound,
            "share_of_bound": bound / sp["v"]["median_ms"], "burst_share_of_bound": bound / sp["v8"]["median_ms"],
            "burst_model_gbps": model / sp["v8"]["median_ms"] / 1e6,
            "vote_tile": _native.kernel_constant("vote_tile"), "vote_group": _native.kernel_constant("vote_group"),
            "vote_loads": _native.kernel_constant("vote_loads")}
    print(json.dumps(line))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
