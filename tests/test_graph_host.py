"""The graph algorithms without a GPU: the golden cases (answers of the reference's own classes)
through the four classes on ``device="cpu"`` and through the numpy restatement, the composite's
dispatch, every assertion and refusal of the embedding exchange, and foreign wire classes."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import (
    AggregationAlgorithm,
    AlgorithmRepository,
    CompositeAggregationAlgorithm,
    FeatureMessage,
    GraphAlgorithm,
    GraphNodeEmbeddingPassingAlgorithm,
    GraphTopologyAlgorithm,
    Message,
    MultipleWorkerMessage,
    ParameterMessage,
)
from distributed_learning_simulation_lib_amd.message import is_feature_message
from tests import graph_foreign_messages as foreign
from tests import graph_reference as ref
from tests.graph_cases import (
    EMBEDDING_CASES,
    check_embedding_result,
    feature_message,
    golden_cases,
    run_embedding_round,
    topology_message,
)


def embedding(**kw):
    return GraphNodeEmbeddingPassingAlgorithm(device="cpu", **kw)


def test_the_golden_file_holds_the_cases_the_contract_names():
    cases = golden_cases()
    assert list(cases) == EMBEDDING_CASES + ["graph_sequence"]
    rounds = [r for c in cases.values() for r in c["rounds"] if r["kind"] == "embedding"]
    features = [f for r in rounds for _, f, _, _ in r["arrivals"] if f is not None]
    assert {f.dtype for f in features} == {torch.float32, torch.float16, torch.bfloat16, torch.float64}
    assert {1, 3, 64, 257} <= {int(np.prod(f.shape[1:])) for f in features}
    assert {len(r["arrivals"]) for r in rounds} >= set(range(2, 10))
    assert any(f is None for _, f, _, _ in cases["silent_worker"]["rounds"][0]["arrivals"])
    assert any(f is None and ids == () for _, ids, f in cases["stranger"]["rounds"][0]["out"])
    nobody = cases["nobody_sends"]["rounds"][0]
    assert all(f is None for _, f, _, _ in nobody["arrivals"]) and all(b for _, _, _, b in nobody["arrivals"])
    assert all(f is None and ids == () for _, ids, f in nobody["out"])
    order = [w for w, _, _, _ in cases["f32_row257_n9"]["rounds"][0]["arrivals"]]
    assert order != sorted(order)
    # a boundary holding ids nobody owns: wanted, never answered
    r = cases["f32_row64_n4"]["rounds"][0]
    assert any(set(b) - set(ids) for (_, _, _, b), (_, ids, _) in zip(r["arrivals"], r["out"]))
    assert [r["kind"] for r in cases["graph_sequence"]["rounds"]] == ["topology", "embedding", "embedding", "fedavg"]


@pytest.mark.parametrize("name", EMBEDDING_CASES)
@pytest.mark.parametrize("tensor_boundary", [False, True])
def test_embedding_golden_on_cpu(name, tensor_boundary):
    algo = embedding()
    for r, rnd in enumerate(golden_cases()[name]["rounds"]):
        res = run_embedding_round(algo, rnd["arrivals"], tensor_boundary=tensor_boundary)
        check_embedding_result(res, rnd["out"], MultipleWorkerMessage, FeatureMessage, what=f"{name}/{r}")


@pytest.mark.parametrize("name", EMBEDDING_CASES + ["graph_sequence"])
def test_restatement_against_the_goldens(name):
    for rnd in golden_cases()[name]["rounds"]:
        if rnd["kind"] != "embedding":
            continue
        got = ref.route_round(rnd["arrivals"])
        assert list(got) == [w for w, _, _ in rnd["out"]]
        for w, ids, feature in rnd["out"]:
            assert got[w][0] == ids
            if feature is None:
                assert got[w][1] is None
            else:
                assert np.array_equal(got[w][1], ref.as_bytes(feature))


def test_topology_golden():
    rnd = golden_cases()["graph_sequence"]["rounds"][0]
    algo = GraphTopologyAlgorithm()
    assert not algo.process_worker_data(0, None)
    assert not algo.process_worker_data(0, Message(other_data={"x": 1}))
    for w, nodes in rnd["arrivals"]:
        assert algo.process_worker_data(worker_id=w, worker_data=topology_message(nodes))
    res = algo.aggregate_worker_data()
    assert type(res) is Message and res.in_round and list(res.other_data) == ["training_node_indices"]
    got = res.other_data["training_node_indices"]
    assert [(w, sorted(v)) for w, v in got.items()] == rnd["out"] and all(type(v) is set for v in got.values())
    with pytest.raises(AssertionError):
        algo.process_worker_data(3, Message(other_data={"training_node_indices": {1}, "more": 2}))


def test_graph_algorithm_golden_sequence_on_cpu():
    """The reference's GraphAlgorithm sequence up to the FedAvg round (which folds on a GPU:
    tests/test_gpu_graph.py runs the whole sequence)."""
    algo = GraphAlgorithm(device="cpu")
    rounds = golden_cases()["graph_sequence"]["rounds"]
    for w, nodes in rounds[0]["arrivals"]:
        assert algo.process_worker_data(worker_id=w, worker_data=topology_message(nodes))
    res = algo.aggregate_worker_data()
    assert [(w, sorted(v)) for w, v in res.other_data["training_node_indices"].items()] == rounds[0]["out"]
    algo.clear_worker_data()
    for r in (1, 2):
        res = run_embedding_round(algo, rounds[r]["arrivals"])
        check_embedding_result(res, rounds[r]["out"], MultipleWorkerMessage, FeatureMessage, what=f"round {r}")


def test_registered_and_exported():
    entry = AlgorithmRepository.config["fed_graph"]
    assert entry["algorithm_cls"] is GraphAlgorithm
    assert issubclass(GraphAlgorithm, CompositeAggregationAlgorithm)


# ---- the composite ---------------------------------------------------------------------------
class Recorder(AggregationAlgorithm):
    def __init__(self, takes) -> None:
        super().__init__()
        self.takes, self.calls = takes, []

    def set_old_parameter(self, old_parameter):
        self.calls.append(("old", old_parameter))

    def set_config(self, config):
        self.calls.append(("config", config))

    def process_worker_data(self, worker_id, worker_data):
        self.calls.append(("process", worker_id))
        return self.takes(worker_data)

    def aggregate_worker_data(self):
        self.calls.append(("aggregate",))
        return self

    def clear_worker_data(self):
        self.calls.append(("clear",))

    def exit(self):
        self.calls.append(("exit",))


def test_composite_dispatch_reset_and_forwarding():
    a, b = Recorder(lambda m: m == "a"), Recorder(lambda m: m in ("b", "b2"))
    comp = CompositeAggregationAlgorithm()
    comp.append_algorithm(b)
    comp.prepend_algorithm(a)
    with pytest.raises(AssertionError):
        comp.aggregate_worker_data()  # nothing was taken
    assert comp.process_worker_data(1, "b")  # a refuses, b takes the round
    assert a.calls == [("process", 1)] and b.calls == [("process", 1)]
    assert comp.process_worker_data(2, "b2") and a.calls == [("process", 1)]  # b only from now on
    with pytest.raises(AssertionError):
        comp.process_worker_data(3, "a")  # the round's algorithm must keep taking
    assert comp.aggregate_worker_data() is b
    assert comp.process_worker_data(4, "a") and comp.aggregate_worker_data() is a  # the choice was reset
    with pytest.raises(NotImplementedError, match="Failed to process_worker_data"):
        comp.process_worker_data(5, "nobody")
    a.calls.clear(), b.calls.clear()
    comp.set_old_parameter({"p": 1})
    comp.set_config("cfg")
    comp.clear_worker_data()
    comp.exit()
    assert a.calls == b.calls == [("old", {"p": 1}), ("config", "cfg"), ("clear",), ("exit",)]


def test_graph_algorithm_refuses_what_no_member_takes():
    algo = GraphAlgorithm(device="cpu")
    assert algo.process_worker_data(0, topology_message({1, 2}))
    with pytest.raises(AssertionError):  # an embedding message inside the topology round
        algo.process_worker_data(1, feature_message(None, None, {1}))


# ---- the embedding exchange: recognition, assertions, refusals ----------------------------------
def test_recognition_and_the_reference_assertions():
    algo = embedding()
    assert not algo.process_worker_data(0, None)
    assert not algo.process_worker_data(0, Message(other_data={"boundary": {1}}))
    assert not algo.process_worker_data(0, ParameterMessage(parameter={"a": torch.zeros(1)}))
    assert is_feature_message(FeatureMessage(feature=None)) and is_feature_message(foreign.FeatureMessage(feature=None))
    assert not is_feature_message(Message()) and not is_feature_message(None)
    with pytest.raises(AssertionError):
        algo.aggregate_worker_data()  # neither features nor boundaries
    with pytest.raises(AssertionError):  # other_data must be empty after the two pops
        algo.process_worker_data(0, FeatureMessage(feature=torch.zeros(1, 2),
                                                   other_data={"node_indices": [3], "boundary": set(), "more": 1}))
    with pytest.raises(AssertionError):  # no feature: node_indices is not popped, as in the reference
        algo.process_worker_data(0, FeatureMessage(feature=None, other_data={"node_indices": [3], "boundary": set()}))
    with pytest.raises(KeyError):
        algo.process_worker_data(0, FeatureMessage(feature=None, other_data={}))


def test_a_node_sent_twice_is_an_assertion_error_at_aggregation():
    algo = embedding()
    assert algo.process_worker_data(0, feature_message(torch.zeros(2, 3), [5, 9], {1}))
    assert algo.process_worker_data(1, feature_message(torch.ones(2, 3), [9, 11], {5}))
    with pytest.raises(AssertionError, match="sent twice"):
        algo.aggregate_worker_data()
    algo.clear_worker_data()
    assert algo.process_worker_data(0, feature_message(torch.zeros(2, 3), [7, 7], {1}))
    with pytest.raises(AssertionError, match="sent twice"):
        algo.aggregate_worker_data()
    algo.clear_worker_data()  # and the object stays usable
    assert algo.process_worker_data(0, feature_message(torch.ones(1, 3), [7], {7}))
    res = algo.aggregate_worker_data()
    assert res.worker_data[0].other_data["node_indices"] == (7,)


@pytest.mark.parametrize("second, match", [
    (lambda: feature_message(torch.zeros(1, 3, dtype=torch.float16), [4], set()), "worker 8.*dtype"),
    (lambda: feature_message(torch.zeros(1, 4), [4], set()), "worker 8.*shape"),
    (lambda: feature_message(torch.zeros(1, 3), [-4], set()), "worker 8.*negative"),
    (lambda: feature_message(torch.zeros(2, 3), [4], set()), "worker 8.*1 node indices"),
    (lambda: FeatureMessage(feature=None, other_data={"boundary": torch.tensor([3, 3])}), "worker 8.*increasing"),
    (lambda: FeatureMessage(feature=None, other_data={"boundary": torch.tensor([3.0])}), "worker 8.*int64"),
])
def test_value_errors_name_the_worker(second, match):
    algo = embedding()
    assert algo.process_worker_data(2, feature_message(torch.zeros(1, 3), [1], set()))
    with pytest.raises(ValueError, match=match):
        algo.process_worker_data(8, second())


def test_not_implemented_past_the_kernel_limits():
    algo = embedding()
    with pytest.raises(NotImplementedError, match="2\\^28"):
        algo.process_worker_data(0, feature_message(torch.zeros(1, 1), [1 << 28], set()))
    algo = embedding()
    for w in range(1024):
        assert algo.process_worker_data(w, feature_message(torch.zeros(1, 1), [w], set()))
    with pytest.raises(NotImplementedError, match="1024"):
        algo.process_worker_data(1024, feature_message(torch.zeros(1, 1), [1024], set()))


def test_ids_past_the_node_space_and_negative_ids_miss():
    algo = embedding()
    assert algo.process_worker_data(0, feature_message(torch.arange(6.0).view(3, 2), [0, 10, 4], {-1, 10, 11, 1 << 40}))
    assert algo.process_worker_data(1, feature_message(None, None, {-5, 0, 4, 9}))
    res = algo.aggregate_worker_data()
    assert res.worker_data[0].other_data["node_indices"] == (10,)
    assert res.worker_data[0].feature.tolist() == [[2.0, 3.0]]
    assert res.worker_data[1].other_data["node_indices"] == (0, 4)
    assert res.worker_data[1].feature.tolist() == [[0.0, 1.0], [4.0, 5.0]]


def test_foreign_wire_classes_in_the_same_modules_classes_out():
    rnd = golden_cases()["silent_worker"]["rounds"][0]
    res = run_embedding_round(embedding(), rnd["arrivals"], feature_cls=foreign.FeatureMessage)
    check_embedding_result(res, rnd["out"], foreign.MultipleWorkerMessage, foreign.FeatureMessage)
    topo = GraphTopologyAlgorithm()
    assert topo.process_worker_data(0, topology_message({1}, foreign.Message))
    assert type(topo.aggregate_worker_data()) is foreign.Message


def test_output_device_cpu_is_the_default_on_a_cpu_device():
    rnd = golden_cases()["f32_row64_n4"]["rounds"][0]
    res = run_embedding_round(embedding(output_device="cpu"), rnd["arrivals"])
    check_embedding_result(res, rnd["out"])
