"""The graph algorithms on the GPU: the golden cases (answers of the reference's own classes)
through the GPU class byte for byte — features arriving on the device and on the host, boundaries
as sets and as sorted tensors —, the whole ``GraphAlgorithm`` sequence, random rounds against the
numpy restatement and against the CPU class, the duplicate assertion, and foreign wire classes."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    FeatureMessage,
    GraphAlgorithm,
    GraphNodeEmbeddingPassingAlgorithm,
    MultipleWorkerMessage,
    _native,
)
from tests import graph_foreign_messages as foreign
from tests import graph_reference as ref
from tests.graph_cases import (
    EMBEDDING_CASES,
    assert_same_bytes,
    check_embedding_result,
    feature_message,
    golden_cases,
    parameter_message,
    random_round,
    run_embedding_round,
    topology_message,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_algo(hip_device):
    algo = GraphNodeEmbeddingPassingAlgorithm(device=hip_device)
    yield algo
    algo.exit()


@pytest.mark.parametrize("name", EMBEDDING_CASES)
@pytest.mark.parametrize("where", ["features_on_gpu", "features_on_host", "tensor_boundaries_on_gpu"])
def test_embedding_golden_on_gpu(gpu_algo, hip_device, name, where):
    kw = {"features_on_gpu": dict(device=hip_device), "features_on_host": {},
          "tensor_boundaries_on_gpu": dict(device=hip_device, tensor_boundary=True)}[where]
    for r, rnd in enumerate(golden_cases()[name]["rounds"]):
        res = run_embedding_round(gpu_algo, rnd["arrivals"], **kw)
        check_embedding_result(res, rnd["out"], MultipleWorkerMessage, FeatureMessage, device_type="cuda",
                               what=f"{name}/{r}")


def test_output_device_cpu_returns_what_the_reference_returns(hip_device):
    algo = GraphNodeEmbeddingPassingAlgorithm(device=hip_device, output_device="cpu")
    rnd = golden_cases()["silent_and_stranger"]["rounds"][0]
    res = run_embedding_round(algo, rnd["arrivals"])
    check_embedding_result(res, rnd["out"], MultipleWorkerMessage, FeatureMessage, device_type="cpu")
    algo.exit()


def test_graph_algorithm_golden_sequence(hip_device):
    algo = GraphAlgorithm(device=hip_device)
    rounds = golden_cases()["graph_sequence"]["rounds"]
    for w, nodes in rounds[0]["arrivals"]:
        assert algo.process_worker_data(worker_id=w, worker_data=topology_message(nodes))
    res = algo.aggregate_worker_data()
    assert res.in_round and [(w, sorted(v)) for w, v in res.other_data["training_node_indices"].items()] == rounds[0]["out"]
    algo.clear_worker_data()
    for r in (1, 2):
        res = run_embedding_round(algo, rounds[r]["arrivals"])
        check_embedding_result(res, rounds[r]["out"], MultipleWorkerMessage, FeatureMessage, device_type="cuda")
    for w, params, weight in rounds[3]["arrivals"]:
        assert algo.process_worker_data(worker_id=w, worker_data=parameter_message(params, weight))
    res = algo.aggregate_worker_data()
    assert list(res.parameter) == list(rounds[3]["out"])
    for name, want in rounds[3]["out"].items():
        assert_same_bytes(res.parameter[name].to(torch.float64), want, name)
    algo.clear_worker_data()
    algo.exit()


@pytest.mark.parametrize("dtype, row_shape, n_workers, owned, wanted", [
    (torch.float32, (64,), 8, 256, 700),     # several chunks per list, 16-byte rows
    (torch.float16, (3,), 5, 40, 90),        # 6-byte rows: the element path
    (torch.float64, (2, 5), 3, 600, 1300),   # trailing shape, more than two chunks
    (torch.bfloat16, (257,), 9, 17, 33),
])
def test_random_rounds_against_the_restatement_and_the_cpu_class(gpu_algo, hip_device, dtype, row_shape, n_workers,
                                                                 owned, wanted):
    arrivals = random_round(17 + n_workers, n_workers, dtype, row_shape, 2 * n_workers * owned, owned, wanted)
    want = ref.route_round(arrivals)
    got = run_embedding_round(gpu_algo, arrivals, device=hip_device)
    cpu = run_embedding_round(GraphNodeEmbeddingPassingAlgorithm(device="cpu"), arrivals)
    assert list(got.worker_data) == list(cpu.worker_data) == list(want)
    for w, (ids, rows) in want.items():
        g, c = got.worker_data[w], cpu.worker_data[w]
        assert g.other_data["node_indices"] == c.other_data["node_indices"] == ids and len(ids) > 0
        assert np.array_equal(ref.as_bytes(g.feature), rows) and np.array_equal(ref.as_bytes(c.feature), rows)
        assert g.feature.dtype == dtype and tuple(g.feature.shape[1:]) == row_shape


def test_a_node_sent_twice_is_an_assertion_error_and_the_object_recovers(gpu_algo, hip_device):
    gpu_algo.process_worker_data(0, feature_message(torch.zeros(2, 4), [5, 9], {1}, device=hip_device))
    gpu_algo.process_worker_data(1, feature_message(torch.ones(2, 4), [9, 11], {5}, device=hip_device))
    with pytest.raises(AssertionError, match="sent twice"):
        gpu_algo.aggregate_worker_data()
    gpu_algo.clear_worker_data()
    # a tensor boundary on the device that is not strictly increasing: found by the kernel
    gpu_algo.process_worker_data(0, FeatureMessage(feature=None, other_data={
        "boundary": torch.tensor([4, 4, 6], device=hip_device)}))
    with pytest.raises(ValueError, match="strictly increasing"):
        gpu_algo.aggregate_worker_data()
    gpu_algo.clear_worker_data()
    rnd = golden_cases()["f32_row64_n4"]["rounds"][0]  # wants 5, 9, 11 among others: the table is empty again
    check_embedding_result(run_embedding_round(gpu_algo, rnd["arrivals"]), rnd["out"], device_type="cuda")


def test_foreign_wire_classes_in_the_same_modules_classes_out(gpu_algo):
    rnd = golden_cases()["stranger"]["rounds"][0]
    res = run_embedding_round(gpu_algo, rnd["arrivals"], feature_cls=foreign.FeatureMessage)
    check_embedding_result(res, rnd["out"], foreign.MultipleWorkerMessage, foreign.FeatureMessage, device_type="cuda")


def test_the_binding_names_the_kernel_limits():
    assert _native.kernel_constant("route_max_sources") == _native.ROUTE_MAX_SOURCES
    assert _native.kernel_constant("route_max_node_space") == _native.ROUTE_MAX_NODE_SPACE
    assert _native.kernel_constant("route_chunk") % _native.kernel_constant("route_threads") == 0
