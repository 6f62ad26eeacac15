"""The reference's ``GraphAlgorithm`` (``simulation_lib/algorithm/graph_algorithm.py:7-12``): the
server of its federated-GNN method, a composite of the topology exchange, the embedding exchange
and FedAvg, tried in that order."""

from __future__ import annotations

import torch

from .composite_aggregation_algorithm import CompositeAggregationAlgorithm
from .fed_avg_algorithm import FedAVGAlgorithm
from .graph_embedding_algorithm import GraphNodeEmbeddingPassingAlgorithm
from .graph_topology_algorithm import GraphTopologyAlgorithm


class GraphAlgorithm(CompositeAggregationAlgorithm):
    """``device`` / ``output_device`` are the embedding exchange's (a GPU, or the CPU). FedAvg
    always folds on a GPU: on ``device`` when that is one, else on the default GPU."""

    def __init__(self, device: torch.device | str | None = None,
                 output_device: torch.device | str | None = None) -> None:
        super().__init__()
        self.append_algorithm(GraphTopologyAlgorithm())
        self.append_algorithm(GraphNodeEmbeddingPassingAlgorithm(device=device, output_device=output_device))
        fed_device = device if device is not None and torch.device(device).type == "cuda" else None
        self.append_algorithm(FedAVGAlgorithm(device=fed_device))
