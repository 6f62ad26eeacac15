#!/usr/bin/env python3
"""Host cost of ``FedAvgContext``'s side-kernel wrappers, without a GPU: the real methods on a CPU
context over a library stand-in that answers every call with 0, so what is timed is the argument
checks and the marshalling alone.

    python scripts/context_checks_host.py --tree . --label new --repeats 5 >> profiles/context_checks_host.jsonl

A ResNet-18-sized layout (62 tensors, 64 elements each: the checks do not depend on the sizes) and
10 clients. One JSON line per wrapper and repeat: microseconds per call, the mean over ``--calls``
calls. ``--tree`` names the checkout whose package is measured, so two trees can be alternated.
``--device cuda`` runs the same calls on a real context with device tensors instead (each batch of
calls ends with a synchronisation): with tensors this small the time is the host's.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time

T, N, NUMEL = 62, 10, 64


class NullLib:
    def __getattr__(self, name):
        if not name.startswith("fedavg_"):
            raise AttributeError(name)
        return lambda *args: 0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=".")
    ap.add_argument("--label", default="new")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import torch

    from distributed_learning_simulation_lib_amd import _native, fedavg
    from distributed_learning_simulation_lib_amd.quantized import record_bytes
    from distributed_learning_simulation_lib_amd.sparse import SparseDelta

    f32, f64 = torch.float32, torch.float64
    layout = fedavg.ModelLayout(names=tuple(f"t{i}" for i in range(T)), shapes=((NUMEL,),) * T)
    table = fedavg.ClientTable(T)
    if args.device == "cpu":
        device = torch.device("cpu")
        fedavg._stream_handle = lambda device: ctypes.c_void_p(0)
        torch.cuda.current_device = lambda: 0
        ctx = fedavg.FedAvgContext.borrowed(NullLib(), 1, layout, device, torch.zeros(T * NUMEL, dtype=f64))
        for k in range(N):
            table.add_resident_client([0x1000 * (k + 1) + 0x10 * t for t in range(T)], [1.0] * T, [NUMEL] * T, 4, 0, [])
    else:
        device = torch.device("cuda", 0)
        ctx = fedavg.FedAvgContext(layout, device)
        for k in range(N):
            table.add_client([torch.full((NUMEL,), float(k), dtype=f32, device=device) for _ in range(T)], [1.0] * T)

    def segs(dtype=torch.float64, numel=NUMEL):
        return [torch.zeros(numel, dtype=dtype, device=device) for _ in range(T)]

    point, direction, outs, base = segs(), segs(), segs(), segs()
    m_in, v_in, m_out, v_out = segs(), segs(), segs(), segs()
    coef = [1.0] * N
    rows = [[SparseDelta(torch.arange(4, dtype=torch.int32, device=device), torch.ones(4, device=device), (NUMEL,))
             for _ in range(T)] for _ in range(N)]
    x, y = segs(f32), segs(f32)
    records = [torch.zeros(record_bytes(NUMEL), dtype=torch.uint8, device=device) for _ in range(T)]
    keeps = [4] * T
    idx, val = segs(torch.int32, 4), segs(f32, 4)
    wrappers = {
        "pairwise_sqdist": lambda: ctx.pairwise_sqdist(table, f32),
        "sqdist_to_point": lambda: ctx.sqdist_to_point(table, f32, point),
        "moments_about_point": lambda: ctx.moments_about_point(table, f32, point, direction),
        "fold_about_point": lambda: ctx.fold_about_point(table, f32, coef, 10.0, point, outs),
        "server_opt_step": lambda: ctx.server_opt_step(table, f32, coef, 10.0, point, m_in, v_in, m_out, v_out, outs,
                                                       mode="adam", lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3),
        "sparse_aggregate_delta": lambda: ctx.sparse_aggregate_delta(rows, coef, 10.0, base, outs),
        "quant_encode": lambda: ctx.quant_encode(_native.QSGD_F32, x, records),
        "quant_decode": lambda: ctx.quant_decode(_native.QSGD_F32, records, y),
        "dp_noise": lambda: ctx.dp_noise(x, y, 1.0, 0.5),
        "topk_sparsify": lambda: ctx.topk_sparsify(x, None, keeps, idx, val, y),
    }
    def sync():
        if args.device == "cuda":
            assert ctx.flags() == 0

    for call in wrappers.values():  # quant_encode fills the records before quant_decode reads them
        call()
    sync()
    for repeat in range(args.repeats):
        for name, call in wrappers.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            sync()
            us = (time.perf_counter() - t0) / args.calls * 1e6
            print(json.dumps({"build": args.label, "repeat": repeat, "wrapper": name, "us_per_call": round(us, 2),
                              "calls": args.calls, "tensors": T, "clients": N, "device": args.device}), flush=True)


if __name__ == "__main__":
    main()
