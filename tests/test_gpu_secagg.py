"""Secure aggregation on the GPU (fedavg_secagg_mask / fedavg_secagg_unmask), bit for
bit against tests/secagg_reference.py. The masked words are uniformly random, so every partial sum
wraps: a dropped seed, a wrong sign, the wrong half of a block or a lost carry cannot pass."""

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import AlgorithmRepository, _native
from distributed_learning_simulation_lib_amd._native import kernel_constant as K
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout
from tests import secagg_reference as ref
from tests.test_secagg_host import SEED, secagg_rounds

pytestmark = pytest.mark.gpu

TILE, SPLIT, LOADS = K("secagg_tile"), K("secagg_split"), K("secagg_loads")
NUMELS = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)
F, VB = 4, 20  # (2^20 - 1) / 16 is an fp32 value; with the largest weight 20 + 31 bits stay below 63
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
# signed zeros, ties of both parities, the largest magnitudes in range, subnormals
PLANTED = [0.0, -0.0, 0.5 / 16, 1.5 / 16, -2.5 / 16, -3.5 / 16, (2 ** VB - 1) / 16, -(2 ** VB - 1) / 16, 5e-324, -1e-310, 1e-40]


def device():
    return torch.device("cuda", torch.cuda.current_device())


def context(numels, dev):
    ctx = FedAvgContext(ModelLayout(names=tuple(f"t{t}" for t in range(len(numels))), shapes=tuple((m,) for m in numels)), dev)
    ctx.accumulator.fill_(3.0)
    return ctx


def framed(numel, dtype, lead, dev, fill=77):  # a buffer of sentinels and the view `lead` elements into it
    whole = torch.full((numel + 2 * lead,), fill, dtype=dtype, device=dev)
    return whole, whole[lead:lead + numel]


def table(rng, count):
    return [(int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.choice((-1, 1)))) for _ in range(count)]


def inputs(numels, dtype, rng, dev):
    xs = []
    for k, m in enumerate(numels):
        x = torch.from_numpy(rng.standard_normal(m) * 100.0)
        x[:len(PLANTED)] = torch.tensor(PLANTED, dtype=torch.float64)[:m]
        x = x.to(dtype)
        x[(x.double() * 2.0 ** F).round().abs() >= 2.0 ** VB] = 0  # a planted value the dtype rounded out of range
        whole = torch.zeros(m + 1, dtype=dtype, device=dev)  # the last segment: aligned to its element only
        lead = int(k == len(numels) - 1)
        whole[lead:lead + m] = x.to(dev)
        xs.append(whole[lead:lead + m])
    return xs


@pytest.mark.parametrize("tag,seeds", [(d, 3) for d in DTYPES] + [("f32", s) for s in (
    1, 2, 64, 65, SPLIT - 1, SPLIT, SPLIT + 1)] + [("f64", 1024)], ids=str)
def test_mask_matches_the_restatement(tag, seeds):
    dev, rng, dtype = device(), np.random.default_rng(seeds), DTYPES[tag]
    numels = (5,) if seeds == 1024 else NUMELS
    ctx, xs, tab = context((1,), dev), inputs(numels, dtype, rng, dev), table(rng, seeds)
    for call, (weight, lead) in enumerate(((2 ** 31 - 1, 1), (1, 2), (0, 1))):  # lead 1: 8- but not 16-byte aligned
        outs = [framed(m, torch.int64, lead, dev) for m in numels]
        ctx.secagg_mask(xs, [o[1] for o in outs], weight, [s for s, _ in tab], [g for _, g in tab], 7 + call, F, VB)
        assert ctx.flags() == 0
        for t, (x, (whole, out)) in enumerate(zip(xs, outs)):
            want, ok = ref.masked(x.double().cpu().numpy(), weight, tab, 7 + call, t, F, VB)
            assert ok.all() and np.array_equal(out.cpu().numpy().view(np.uint64), want), (call, t)
            assert (whole[:lead] == 77).all() and (whole[lead + x.numel():] == 77).all(), (call, t)
    assert (ctx.accumulator == 3.0).all()


@pytest.mark.parametrize("bad", [2.0 ** (VB - F), float("inf"), float("nan")], ids=["range", "inf", "nan"])
@pytest.mark.parametrize("seeds", [2, SPLIT], ids=["wave", "shared"])
def test_mask_latches_the_input_flag_alone(bad, seeds):
    dev, rng = device(), np.random.default_rng(1)
    ctx, tab = context((1,), dev), table(rng, seeds)
    x = torch.zeros(TILE + 3, device=dev)
    x[TILE + 1] = -bad
    ctx.secagg_mask([x], [torch.empty(TILE + 3, dtype=torch.int64, device=dev)], 1, [s for s, _ in tab],
                    [g for _, g in tab], 0, F, VB)
    assert ctx.flags() == _native.FLAG_INPUT_NAN
    ctx.reset()


DROPS = {"none": lambda n: [], "first": lambda n: [0], "last": lambda n: [n - 1],
         "second": lambda n: list(range(1, n, 2)), "all-but-one": lambda n: list(range(1, n))}
MODES = [(b, o) for b in (True, False) for o in (torch.float64, torch.float32)]
UNMASK = ([(5, d, m) for d in DROPS for m in range(4)] + [(65, d, k % 4) for k, d in enumerate(DROPS)]
          + [(n, list(DROPS)[k % 5], k % 4) for k, n in enumerate((1, 2, 3, LOADS - 1, LOADS + 1, 64))])


@pytest.mark.parametrize("workers,drop,mode", UNMASK, ids=str)
def test_unmask_matches_the_restatement(workers, drop, mode):
    dev, rng = device(), np.random.default_rng(workers)
    with_base, out_dtype = MODES[mode]
    D = DROPS[drop](workers) if workers > 1 else []
    A = [i for i in range(workers) if i not in D]
    tab, W = ref.server_table(SEED, A, D, 3), float(sum(1 + i for i in A))
    ctx = context(NUMELS, dev)
    words = [[rng.integers(0, 1 << 64, m, dtype=np.uint64) for m in NUMELS] for _ in A]
    # every second client one element into its buffer: 8-byte but not 16-byte aligned storage
    rows = [[framed(m, torch.int64, 1 + i % 2, dev)[1].copy_(torch.from_numpy(w.view(np.int64))) for m, w in zip(NUMELS, row)]
            for i, row in enumerate(words)]
    base = [torch.from_numpy(rng.standard_normal(m)).to(dev) for m in NUMELS] if with_base else None
    kept = [t.clone() for t in (base or [])] + [t.clone() for row in rows for t in row]
    both = []
    for _ in range(2):  # the ring's two slots
        outs = [framed(m, out_dtype, 1, dev) for m in NUMELS]
        ctx.secagg_unmask(rows, [s for s, _ in tab], [g for _, g in tab], 3, F, W, base, [o[1] for o in outs], out_dtype)
        assert ctx.flags() == 0
        both.append(outs)
    for t, m in enumerate(NUMELS):
        want = ref.unmasked([row[t] for row in words], tab, 3, t, F, W, base[t].cpu().numpy() if with_base else None,
                            out_dtype == torch.float32)
        for whole, out in (both[0][t], both[1][t]):
            assert np.array_equal(out.cpu().numpy().view(want.dtype.str.replace("f", "u")),
                                  want.view(want.dtype.str.replace("f", "u"))), t
            assert (whole[:1] == 77).all() and (whole[1 + m:] == 77).all(), t
    assert all(torch.equal(a, b) for a, b in zip(kept, (base or []) + [t for row in rows for t in row]))
    assert (ctx.accumulator == 3.0).all()


def test_unmask_flags_and_wrapper_refusals():
    dev = device()
    ctx = context((3,), dev)
    rows, out = [[torch.ones(3, dtype=torch.int64, device=dev)]], torch.full((3,), 77.0, dtype=torch.float64, device=dev)
    base = torch.tensor([0.0, float("nan"), 1.0], dtype=torch.float64, device=dev)
    ctx.secagg_unmask(rows, [], [], 0, F, 1.0, [base], [out])
    assert ctx.flags() == _native.FLAG_INPUT_NAN
    ctx.reset()
    ctx.secagg_unmask([[torch.zeros(3, dtype=torch.int64, device=dev)]], [], [], 0, F, 0.0, None, [out])  # 0 / 0
    assert ctx.flags() == _native.FLAG_RESULT_NAN and torch.isnan(out).all()
    ctx.reset()
    out.fill_(77.0)
    x = torch.ones(3, device=dev)
    refused = [
        lambda: ctx.secagg_unmask(rows * 1025, [], [], 0, F, 1.0, None, [out]),
        lambda: ctx.secagg_unmask(rows, [], [], 0, 53, 1.0, None, [out]),
        lambda: ctx.secagg_unmask(rows, [], [], 0, F, 1.0, [out], [out]),
        lambda: ctx.secagg_unmask(rows, [], [], 0, F, 1.0, None, [rows[0][0].view(torch.float64)]),
        lambda: ctx.secagg_unmask([[rows[0][0].int()]], [], [], 0, F, 1.0, None, [out]),
        lambda: ctx.secagg_unmask(rows, [5], [0], 0, F, 1.0, None, [out]),
        lambda: ctx.secagg_mask([x], [rows[0][0]], 1, [5], [1], 0, F, 0),
        lambda: ctx.secagg_mask([x], [rows[0][0]], 1.5, [5], [1], 0, F, VB),
        lambda: ctx.secagg_mask([x], [rows[0][0]], 1, [], [], 0, F, VB),
        lambda: ctx.secagg_mask([x], [rows[0][0][:2]], 1, [5], [1], 0, F, VB),
    ]
    for k, call in enumerate(refused):
        with pytest.raises((ValueError, TypeError, NotImplementedError)):
            call()
        assert ctx.flags() == 0 and (out == 77.0).all() and (rows[0][0] == 1).all(), k


@pytest.mark.parametrize("out_dtype", [torch.float64, torch.float32], ids=["out64", "out32"])
def test_the_class_on_the_gpu_equals_the_class_on_the_cpu_and_the_restatement(out_dtype):
    entry = AlgorithmRepository.config["fed_avg_secagg"]
    assert entry["algorithm_cls"].accepts_masked_messages and entry["client_endpoint_cls"].__name__ == "SecAggEndpoint"
    present = [[0, 1, 2, 3, 4], [0, 2, 3], [2, 0]]
    gpu = secagg_rounds(device(), present, out_dtype, client_device=device(), algorithm_cls=entry["algorithm_cls"],
                        endpoint_cls=entry["client_endpoint_cls"])
    cpu = secagg_rounds(torch.device("cpu"), present, out_dtype)
    for g, c in zip(gpu, cpu):
        assert all(torch.equal(g.parameter[k].cpu().view(torch.int64), c.parameter[k].view(torch.int64)) for k in c.parameter)
