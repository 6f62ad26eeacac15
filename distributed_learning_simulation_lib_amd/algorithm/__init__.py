from .aggregation_algorithm import AggregationAlgorithm
from .bulyan_aggregation_algorithm import BulyanFedAVGAlgorithm
from .clipped_aggregation_algorithm import ClippedFedAVGAlgorithm
from .composite_aggregation_algorithm import CompositeAggregationAlgorithm
from .fed_avg_algorithm import FedAVGAlgorithm
from .fltrust_aggregation_algorithm import FLTrustFedAVGAlgorithm
from .geometric_median_algorithm import GeometricMedianFedAVGAlgorithm
from .graph_algorithm import GraphAlgorithm
from .graph_embedding_algorithm import GraphNodeEmbeddingPassingAlgorithm
from .graph_topology_algorithm import GraphTopologyAlgorithm
from .krum_aggregation_algorithm import KrumFedAVGAlgorithm
from .personalized_aggregation_algorithm import PersonalizedFedAVGAlgorithm
from .robust_aggregation_algorithm import RobustFedAVGAlgorithm
from .server_opt_algorithm import ServerOptFedAVGAlgorithm
from .sparse_fed_avg_algorithm import SparseFedAVGAlgorithm

__all__ = ["AggregationAlgorithm", "BulyanFedAVGAlgorithm", "ClippedFedAVGAlgorithm", "CompositeAggregationAlgorithm",
           "FLTrustFedAVGAlgorithm", "FedAVGAlgorithm", "GeometricMedianFedAVGAlgorithm", "GraphAlgorithm",
           "GraphNodeEmbeddingPassingAlgorithm", "GraphTopologyAlgorithm", "KrumFedAVGAlgorithm",
           "PersonalizedFedAVGAlgorithm",
           "RobustFedAVGAlgorithm", "ServerOptFedAVGAlgorithm", "SparseFedAVGAlgorithm"]
