"""The Gram kernel (csrc/gram_kernels.hip) and ``FoolsGoldFedAVGAlgorithm`` on the MI355X against the
numpy restatement (tests/foolsgold_reference.py; NOT a reference algorithm). Sizes come from the
build's geometry. Integer inputs in [-32, 32] (point and histories too) make every product and partial
sum an exact integer below 2^53, so ``G`` and ``history_out`` are compared bit for bit. For N(0, 1)
inputs kernel and restatement are each within (P + 2) * 2^-53 * sum_e |r_i r_j| of the exact value, so
they differ by at most twice that; ``history_out`` is two IEEE operations and stays bit for bit."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    ClientTable,
    FedAvgContext,
    FoolsGoldFedAVGAlgorithm,
    ModelLayout,
    ParameterMessage,
    _native,
)
from tests import foolsgold_reference as ref

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
COUNTS = [1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 130]


def edge_sizes(code: str) -> list[int]:
    """The last segment is the one stored misaligned."""
    k = _native.kernel_constant
    tile, chunk, ae = k("gram_tile"), k("gram_chunk"), k(f"gram_ae_{code}")
    return [1, ae - 1, 3, 4, 5, tile - 1, tile, tile + 1, chunk + 1, 2 * ae + 1]


def place(t: torch.Tensor, device, misalign: bool) -> torch.Tensor:
    """``t`` on the device; ``misalign``: a contiguous view one element into a larger buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    v = buf[1:] if misalign else buf[:-1]
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == misalign
    return v


def draw(gen, numel, dtype, integer):
    x = torch.randint(-32, 33, (numel,), generator=gen) if integer else torch.randn(numel, generator=gen)
    return x.to(dtype)


class Case:
    """n clients of a layout on the device with a point and histories, and their float64 numpy images."""

    def __init__(self, device, sizes, n, dtype, integer, seed):
        gen = torch.Generator().manual_seed(seed)
        last = len(sizes) - 1
        put = lambda t, i: place(t, device, i == last and len(sizes) > 1)  # noqa: E731
        host = [[draw(gen, s, dtype, integer) for s in sizes] for _ in range(n)]
        point = [draw(gen, s, torch.float64, integer) for s in sizes]
        hist = [[draw(gen, s, torch.float64, integer) for s in sizes] for _ in range(n)]
        self.n, self.dtype = n, dtype
        self.rows = [[t.to(torch.float64).numpy() for t in r] for r in host]
        self.point, self.hist = [t.numpy() for t in point], [[t.numpy() for t in r] for r in hist]
        self.ctx = FedAvgContext(ModelLayout(names=tuple(f"t{i}" for i in range(len(sizes))),
                                             shapes=tuple((s,) for s in sizes)), device)
        self.table = ClientTable(len(sizes))
        for r in host:
            self.table.add_client([put(t, i) for i, t in enumerate(r)], [1.0] * len(sizes))
        self.d_point = [put(t, i) for i, t in enumerate(point)]
        self.d_hin = [[put(t, i) for i, t in enumerate(r)] for r in hist]
        self.d_hout = [[put(torch.full_like(t, 7.0), i) for i, t in enumerate(r)] for r in hist]

    def gram(self, full: bool):
        """(G, history_out) from the GPU and (G, history_out, A) from the restatement."""
        args = (self.d_point, self.d_hin, self.d_hout) if full else (None, None, None)
        G = self.ctx.gram_about_point(self.table, self.dtype, *args).cpu().numpy()
        assert self.ctx.flags() == 0
        hout = [[t.cpu().numpy() for t in r] for r in self.d_hout] if full else None
        return (G, hout), ref.gram(self.rows, *((self.point, self.hist) if full else (None, None)))


def same_bits(a, b) -> bool:
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def check_exact(case: Case):
    for full in (False, True):
        (G, hout), (G_ref, h_ref, _) = case.gram(full)
        assert G.shape == (case.n, case.n) and np.array_equal(G, G_ref), full
        if full:
            assert all(same_bits(a, b) for ra, rb in zip(hout, h_ref) for a, b in zip(ra, rb))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("code", list(DTYPES))
def test_integer_inputs_are_bit_exact(hip_device, code, n):
    check_exact(Case(hip_device, edge_sizes(code), n, DTYPES[code], True, 1000 * n + len(code)))


def test_256_clients_one_tiny_segment(hip_device):
    check_exact(Case(hip_device, [5], 256, torch.float32, True, 256))


@pytest.mark.parametrize("n", [17, 130])
@pytest.mark.parametrize("code", list(DTYPES))
def test_gaussian_inputs_within_the_bound_symmetric_and_repeatable(hip_device, code, n):
    sizes = edge_sizes(code)
    case = Case(hip_device, sizes, n, DTYPES[code], False, 77 * n + len(code))
    (G, hout), (G_ref, h_ref, A) = case.gram(True)
    err, bound = np.abs(G - G_ref), 2 * (sum(sizes) + 2) * 2.0 ** -53 * A
    print(f"max |G - G_ref| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert all(same_bits(a, b) for ra, rb in zip(hout, h_ref) for a, b in zip(ra, rb))
    assert same_bits(G, G.T)
    assert same_bits(case.gram(True)[0][0], G)


def test_flags_and_refusals(hip_device):
    case = Case(hip_device, [5, 40], 3, torch.float32, True, 9)
    ctx, table = case.ctx, case.table
    x = table.arrays()  # keep the table's arrays alive
    client0 = torch.zeros(5, dtype=torch.float32, device=hip_device)
    t2 = ClientTable(2)
    t2.add_client([client0, torch.zeros(40, device=hip_device)], [1.0, 1.0])
    inf_client = torch.zeros(5, device=hip_device)
    inf_client[2] = float("inf")
    t2.add_client([inf_client, torch.zeros(40, device=hip_device)], [1.0, 1.0])
    ctx.gram_about_point(t2, torch.float32)                    # 0 * inf in G[0][1]
    assert ctx.flags() == _native.FLAG_ACC_NAN
    ctx.reset()
    inf_client[2] = float("nan")
    ctx.gram_about_point(t2, torch.float32)
    assert ctx.flags() & _native.FLAG_INPUT_NAN
    ctx.reset()
    before = [[t.clone() for t in r] for r in case.d_hout]
    for kwargs in ({"history_in": case.d_hin}, {"history_out": case.d_hout},
                   {"history_in": case.d_hin, "history_out": case.d_hin},
                   {"history_in": case.d_hin, "history_out": [case.d_hout[0], case.d_hout[0], case.d_hout[2]]},
                   {"point": case.d_point[:1]}, {"point": [t.float() for t in case.d_point]}):
        with pytest.raises(ValueError):
            ctx.gram_about_point(table, torch.float32, **kwargs)
    many = ClientTable(2)
    for _ in range(_native.GRAM_MAX_CLIENTS + 1):
        many.add_client([client0, torch.zeros(40, device=hip_device)], [1.0, 1.0])
    with pytest.raises(NotImplementedError, match=str(_native.GRAM_MAX_CLIENTS)):
        ctx.gram_about_point(many, torch.float32)
    assert ctx.flags() == 0 and x is not None
    assert all(torch.equal(a, b) for ra, rb in zip(case.d_hout, before) for a, b in zip(ra, rb))


def run_round(algo, updates, previous):
    for wid, c in enumerate(updates):
        algo.process_worker_data(10 + wid, None if c is None else ParameterMessage(parameter=dict(c), aggregation_weight=1))
    algo.set_old_parameter(previous)
    try:
        return algo.aggregate_worker_data().parameter
    finally:
        algo.clear_worker_data()


@pytest.mark.parametrize("integer", [True, False])
def test_class_two_rounds_with_a_skipped_worker(hip_device, integer):
    """Integer inputs: the GPU class, the CPU class and the restatement give the same bits. Gaussian
    inputs: the GPU class gives the bits of the restatement fed the GPU's own ``G``."""
    shapes = {"a": (33,), "b": (4, 5)}
    gen = torch.Generator().manual_seed(5)
    previous = {k: draw(gen, int(np.prod(s)), torch.float64, integer).reshape(s) for k, s in shapes.items()}
    rounds = [[{k: draw(gen, int(np.prod(s)), torch.float32, integer).reshape(s) for k, s in shapes.items()}
               for _ in range(5)] for _ in range(2)]
    rounds[0][3] = {k: t.clone() for k, t in rounds[0][0].items()}   # a look-alike in round 1
    rounds[1][1] = None                                               # worker 11 skips round 2
    gpu, cpu = FoolsGoldFedAVGAlgorithm(device=hip_device), FoolsGoldFedAVGAlgorithm(device="cpu")
    ctx = FedAvgContext(ModelLayout(names=tuple(shapes), shapes=tuple(shapes.values())), hip_device)
    point = [t.numpy().reshape(-1) for t in previous.values()]
    hist = {10 + w: [np.zeros(int(np.prod(s))) for s in shapes.values()] for w in range(5)}
    for updates in rounds:
        ids = [10 + w for w, c in enumerate(updates) if c is not None]
        rows = [[t.to(torch.float64).numpy().reshape(-1) for t in c.values()] for c in updates if c is not None]
        table = ClientTable(len(shapes))
        for c in updates:
            if c is not None:
                table.add_client([t.reshape(-1).to(hip_device) for t in c.values()], [1.0] * len(shapes))
        to_dev = lambda rows_: [[torch.from_numpy(a).to(hip_device) for a in r] for r in rows_]  # noqa: E731
        hin = to_dev([hist[w] for w in ids])
        G = ctx.gram_about_point(table, torch.float32, [torch.from_numpy(z).to(hip_device) for z in point], hin,
                                 [[torch.empty_like(t) for t in r] for r in hin]).cpu().numpy()
        want, new, alphas, _ = ref.foolsgold_round(rows, point, [hist[w] for w in ids], G=None if integer else G)
        hist.update(zip(ids, new))
        got = run_round(gpu, updates, previous)
        assert same_bits(gpu.last_foolsgold.alphas, alphas) and gpu.last_foolsgold.worker_ids == ids
        assert all(same_bits(g.cpu().numpy().reshape(-1), w) for g, w in zip(got.values(), want))
        if integer:
            on_cpu = run_round(cpu, updates, previous)
            assert all(same_bits(g.cpu().numpy(), c.numpy()) for g, c in zip(got.values(), on_cpu.values()))
    state = gpu.state_dict()["history"]
    assert all(same_bits(t.numpy().reshape(-1), h) for w in hist for t, h in zip(state[w].values(), hist[w]))
