"""``SparseFedAVGAlgorithm`` on the GPU: the golden cases (expected results from the reference's own
``restore()`` + ``FedAVGAlgorithm`` on the densified deltas) bit for bit, the GPU class against the
CPU class, a round through the server, the NaN stages and the refusals that need the device."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    DeltaParameterMessage,
    NaNAggregationError,
    ParameterMessage,
    SparseDelta,
    SparseFedAVGAlgorithm,
    _native,
    topk_sparsify,
)
from distributed_learning_simulation_lib_amd.server import AggregationServer
from tests.sparse_cases import CASES, assert_same_bits, golden_cases, random_sparse, run_round

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_on_the_gpu(hip_device, name):
    case = golden_cases()[name]
    for out_dtype, npd in ((torch.float64, np.float64), (torch.float32, np.float32)):
        gpu = run_round(SparseFedAVGAlgorithm(device=hip_device, out_dtype=out_dtype), case)
        cpu = run_round(SparseFedAVGAlgorithm(device=CPU, out_dtype=out_dtype), case)
        assert list(gpu.parameter) == case["names"]
        for n in case["names"]:
            got = gpu.parameter[n]
            assert got.device == hip_device and got.dtype == out_dtype and tuple(got.shape) == case["shapes"][n]
            assert_same_bits(got, case["out"][n].astype(npd), f"{name} {n} {out_dtype}: the reference")
            assert_same_bits(got, cpu.parameter[n], f"{name} {n} {out_dtype}: the CPU class")


def make_round(gen, shapes, n, dtype, ratio):
    old = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    msgs = []
    for wid in range(n):
        delta = {k: topk_sparsify((torch.randn(s, generator=gen) * 0.1).to(dtype), ratio=ratio)[0]
                 for k, s in shapes.items()}
        msgs.append((wid, DeltaParameterMessage(delta_parameter=delta, aggregation_weight=10 + 3 * wid)))
    return dict(old=old, names=list(shapes)), msgs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gpu_class_equals_cpu_class_over_several_tiles(hip_device, dtype):
    """Top-k deltas of a layout with an empty tensor, a 0-dim tensor and tensors of several tiles."""
    T, B = _native.kernel_constant("sparse_tile"), _native.kernel_constant("sparse_batch")
    shapes = {"w": (3, T + 1), "e": (0,), "s": (), "b": (T - 1,), "v": (2 * T + 3,)}
    case, msgs = make_round(torch.Generator().manual_seed(41), shapes, 2 * B + 1, dtype, 0.02)

    def run(device, out_dtype):
        algo = SparseFedAVGAlgorithm(device=device, out_dtype=out_dtype)
        algo.set_old_parameter(case["old"])
        for wid, m in msgs:
            algo.process_worker_data(wid, m)
        return algo, algo.aggregate_worker_data()

    for out_dtype in (torch.float64, torch.float32):
        ga, g = run(hip_device, out_dtype)
        ca, c = run(CPU, out_dtype)
        assert ga.last_round == ca.last_round and ga.last_round.worker_ids == list(range(2 * B + 1))
        assert list(g.parameter) == list(shapes) and g.parameter["e"].shape == (0,)
        for n in shapes:
            assert_same_bits(g.parameter[n], c.parameter[n], f"{n} {dtype} {out_dtype}")


def test_round_through_the_server(hip_device):
    gen = torch.Generator().manual_seed(42)
    init = {"w": torch.randn(50, 60, generator=gen, dtype=torch.float64), "b": torch.randn(7, generator=gen,
                                                                                          dtype=torch.float64)}
    rounds = [[{n: topk_sparsify(torch.randn(t.shape, generator=gen) * 0.1, ratio=0.05)[0] for n, t in init.items()}
               for _ in range(3)] for _ in range(2)]

    def run(device):
        server = AggregationServer(SparseFedAVGAlgorithm(device=device), worker_number=3, round_number=2)
        server._send_result(ParameterMessage(parameter=init, in_round=True, is_initial=True))
        for deltas in rounds:
            for wid, delta in enumerate(deltas):
                server._process_worker_data(wid, DeltaParameterMessage(delta_parameter=dict(delta),
                                                                       aggregation_weight=wid + 1))
        return server.results

    for a, b in zip(run(hip_device), run(CPU)):
        for n in init:
            assert_same_bits(a.parameter[n], b.parameter[n], f"server round: {n}")


def faulty_round(hip_device, edit):
    gen = torch.Generator().manual_seed(43)
    numel = _native.kernel_constant("sparse_tile") + 5
    old = {"a": torch.randn(numel, generator=gen, dtype=torch.float64)}
    deltas = [random_sparse(gen, numel, 40, torch.float32) for _ in range(3)]
    edit(deltas)
    algo = SparseFedAVGAlgorithm(device=hip_device)
    algo.set_old_parameter(old)
    for wid, d in enumerate(deltas):
        algo.process_worker_data(wid, DeltaParameterMessage(delta_parameter={"a": d}, aggregation_weight=1 + wid))
    return algo


def test_nan_stages(hip_device):
    def nan_value(deltas):
        deltas[1].values[3] = float("nan")

    def opposite_infinities(deltas):
        at = int(deltas[0].indices[5])
        for k, v in ((0, float("inf")), (2, float("-inf"))):
            keep = deltas[k].indices != at
            idx = torch.cat([deltas[k].indices[keep], torch.tensor([at], dtype=torch.int32)])
            val = torch.cat([deltas[k].values[keep], torch.tensor([v])])
            order = torch.argsort(idx)
            deltas[k] = SparseDelta(idx[order], val[order], deltas[k].shape)

    for edit, stage in ((nan_value, "input"), (opposite_infinities, "accumulator")):
        with pytest.raises(NaNAggregationError) as e:
            faulty_round(hip_device, edit).aggregate_worker_data()
        assert e.value.stage == stage
    # the flags were cleared: the cached context folds the next round
    assert faulty_round(hip_device, lambda deltas: None).aggregate_worker_data().parameter["a"].isfinite().all()


def test_zero_total_weight_is_refused_before_any_launch(hip_device):
    algo = faulty_round(hip_device, lambda deltas: None)
    for msg in algo._all_worker_data.values():
        msg.aggregation_weight = 0
    with pytest.raises(ValueError, match="add up to 0"):
        algo.aggregate_worker_data()


@pytest.mark.parametrize("what", ["duplicate", "descending", "negative", "numel"])
def test_index_violations_are_a_value_error(hip_device, what):
    def edit(deltas):
        i = deltas[1].indices
        if what == "duplicate":
            i[7] = i[6]
        elif what == "descending":
            i[6], i[7] = i[7].item(), i[6].item()
        elif what == "negative":
            i[0] = -1
        else:
            i[-1] = deltas[1].numel

    with pytest.raises(ValueError, match="strictly increasing"):
        faulty_round(hip_device, edit).aggregate_worker_data()
    assert faulty_round(hip_device, lambda deltas: None).aggregate_worker_data().parameter["a"].isfinite().all()


def test_a_nan_beside_a_bad_index_does_not_outlive_its_round(hip_device):
    """The fold that meets the bad index also latches the input flag; the context is cached per
    layout, so the next, clean round on it must not raise for the round before."""
    def edit(deltas):
        deltas[1].indices[7] = deltas[1].indices[6]
        deltas[0].values[3] = float("nan")

    with pytest.raises(ValueError, match="strictly increasing"):
        faulty_round(hip_device, edit).aggregate_worker_data()
    assert faulty_round(hip_device, lambda deltas: None).aggregate_worker_data().parameter["a"].isfinite().all()


def test_the_input_stage_wins_over_the_accumulator_stage_on_both_devices(hip_device):
    numel = _native.kernel_constant("sparse_tile") + 5
    old = {"a": torch.zeros(numel, dtype=torch.float64), "b": torch.zeros(7, dtype=torch.float64)}
    idx = torch.tensor([2], dtype=torch.int32)

    def run(device, b_value):
        algo = SparseFedAVGAlgorithm(device=device)
        algo.set_old_parameter(old)
        for wid, (a, b) in enumerate(((float("inf"), 1.0), (float("-inf"), b_value))):
            algo.process_worker_data(wid, DeltaParameterMessage(aggregation_weight=1, delta_parameter={
                "a": SparseDelta(idx, torch.tensor([a]), (numel,)), "b": SparseDelta(idx, torch.tensor([b]), (7,))}))
        return algo.aggregate_worker_data()

    for device in (hip_device, CPU):
        for b_value, stage in ((1.0, "accumulator"), (float("nan"), "input")):
            with pytest.raises(NaNAggregationError) as e:
                run(device, b_value)
            assert e.value.stage == stage, (device, stage)
