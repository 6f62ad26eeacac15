"""The reference's ``GraphTopologyAlgorithm``
(``simulation_lib/algorithm/graph_topology_algorithm.py:7-30``): the workers of a federated GNN
exchange their training node indices once, before training. Host logic only.

A message is taken when its ``other_data`` holds ``"training_node_indices"`` (popped; nothing else
may be left). The answer is one in-round ``Message`` of the caller's wire module whose
``other_data["training_node_indices"]`` maps every worker to what it sent. As in the reference the
map is never cleared.
"""

from __future__ import annotations

from typing import Any

from ..message import Message, is_message, wire_class
from .aggregation_algorithm import AggregationAlgorithm


class GraphTopologyAlgorithm(AggregationAlgorithm):
    def __init__(self) -> None:
        super().__init__()
        self._training_node_indices: dict[int, Any] = {}
        self.__like: Any = None

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if worker_data is not None and is_message(worker_data) and "training_node_indices" in worker_data.other_data:
            self._training_node_indices[worker_id] = worker_data.other_data.pop("training_node_indices")
            assert not worker_data.other_data
            self.__like = worker_data
            return True
        return False

    def aggregate_worker_data(self) -> Message:
        return wire_class(self.__like, "Message")(
            in_round=True, other_data={"training_node_indices": self._training_node_indices})
