from .aggregation_algorithm import AggregationAlgorithm
from .bulyan_aggregation_algorithm import BulyanFedAVGAlgorithm
from .clipped_aggregation_algorithm import ClippedFedAVGAlgorithm
from .composite_aggregation_algorithm import CompositeAggregationAlgorithm
from .fed_avg_algorithm import FedAVGAlgorithm
from .fltrust_aggregation_algorithm import FLTrustFedAVGAlgorithm
from .foolsgold_aggregation_algorithm import FoolsGoldFedAVGAlgorithm
from .geometric_median_algorithm import GeometricMedianFedAVGAlgorithm
from .graph_algorithm import GraphAlgorithm
from .graph_embedding_algorithm import GraphNodeEmbeddingPassingAlgorithm
from .graph_topology_algorithm import GraphTopologyAlgorithm
from .krum_aggregation_algorithm import KrumFedAVGAlgorithm
from .lowrank_fed_avg_algorithm import LowRankFedAVGAlgorithm
from .mx_fed_avg_algorithm import MXFedAVGAlgorithm
from .personalized_aggregation_algorithm import PersonalizedFedAVGAlgorithm
from .robust_aggregation_algorithm import RobustFedAVGAlgorithm
from .rotated_sign_fed_avg_algorithm import RotatedSignFedAVGAlgorithm
from .secagg_fed_avg_algorithm import SecAggFedAVGAlgorithm
from .server_opt_algorithm import ServerOptFedAVGAlgorithm
from .sign_fed_avg_algorithm import SignFedAVGAlgorithm
from .sign_vote_algorithm import SignMajorityVoteAlgorithm
from .sparse_fed_avg_algorithm import SparseFedAVGAlgorithm

__all__ = ["AggregationAlgorithm", "BulyanFedAVGAlgorithm", "ClippedFedAVGAlgorithm", "CompositeAggregationAlgorithm",
           "FLTrustFedAVGAlgorithm", "FedAVGAlgorithm", "FoolsGoldFedAVGAlgorithm", "GeometricMedianFedAVGAlgorithm", "GraphAlgorithm",
           "GraphNodeEmbeddingPassingAlgorithm", "GraphTopologyAlgorithm", "KrumFedAVGAlgorithm",
           "LowRankFedAVGAlgorithm", "MXFedAVGAlgorithm", "PersonalizedFedAVGAlgorithm",
           "RobustFedAVGAlgorithm", "RotatedSignFedAVGAlgorithm", "SecAggFedAVGAlgorithm", "ServerOptFedAVGAlgorithm", "SignFedAVGAlgorithm", "SignMajorityVoteAlgorithm",
           "SparseFedAVGAlgorithm"]
