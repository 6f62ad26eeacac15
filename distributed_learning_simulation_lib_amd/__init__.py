"""MI355X-native server-side FedAvg aggregation for distributed_learning_simulation_lib.

The hot path — the weighted reduction of N clients' parameter tensors into one global model
(reference ``simulation_lib/algorithm/fed_avg_algorithm.py``) — runs in hand-written gfx950
HIP kernels behind the C ABI of ``include/fedavg_hip.h``; this package is the host side that
keeps the reference's plugin surface.
"""

import functools

from .algorithm import (
    AggregationAlgorithm,
    BulyanFedAVGAlgorithm,
    ClippedFedAVGAlgorithm,
    CompositeAggregationAlgorithm,
    FedAVGAlgorithm,
    FLTrustFedAVGAlgorithm,
    GeometricMedianFedAVGAlgorithm,
    GraphAlgorithm,
    GraphNodeEmbeddingPassingAlgorithm,
    GraphTopologyAlgorithm,
    KrumFedAVGAlgorithm,
    PersonalizedFedAVGAlgorithm,
    RobustFedAVGAlgorithm,
    ServerOptFedAVGAlgorithm,
    SparseFedAVGAlgorithm,
)
from .algorithm_repository import AlgorithmRepository
from .dp import (
    DifferentialPrivacyEmbeddingEndpoint,
    DifferentialPrivacyParameterEndpoint,
    add_dp_noise,
    add_dp_noise_to_parameter,
    compute_dp_sigma,
    normal_stream,
)
from .fedavg import ClientTable, FedAvgContext, ModelLayout, NaNAggregationError
from .message import (
    DeltaParameterMessage,
    FeatureMessage,
    Message,
    ModelParameter,
    MultipleWorkerMessage,
    ParameterMessage,
    ParameterMessageBase,
    get_message_size,
)
from .quantized import (
    BroadcastDequantizer,
    BroadcastQuantizer,
    NNADQClientEndpoint,
    QuantClientEndpoint,
    StochasticQuantClientEndpoint,
    philox_uniforms,
)
from .sparse import SparseDelta, TopKErrorFeedback, TopKSparseEndpoint, topk_sparsify, topk_sparsify_parameter

__all__ = [
    "AggregationAlgorithm",
    "AlgorithmRepository",
    "BroadcastDequantizer",
    "BroadcastQuantizer",
    "BulyanFedAVGAlgorithm",
    "ClientTable",
    "ClippedFedAVGAlgorithm",
    "CompositeAggregationAlgorithm",
    "DeltaParameterMessage",
    "DifferentialPrivacyEmbeddingEndpoint",
    "DifferentialPrivacyParameterEndpoint",
    "FeatureMessage",
    "FedAVGAlgorithm",
    "FLTrustFedAVGAlgorithm",
    "FedAvgContext",
    "GeometricMedianFedAVGAlgorithm",
    "GraphAlgorithm",
    "GraphNodeEmbeddingPassingAlgorithm",
    "GraphTopologyAlgorithm",
    "KrumFedAVGAlgorithm",
    "Message",
    "ModelLayout",
    "ModelParameter",
    "MultipleWorkerMessage",
    "NNADQClientEndpoint",
    "NaNAggregationError",
    "ParameterMessage",
    "ParameterMessageBase",
    "PersonalizedFedAVGAlgorithm",
    "QuantClientEndpoint",
    "RobustFedAVGAlgorithm",
    "ServerOptFedAVGAlgorithm",
    "SparseDelta",
    "SparseFedAVGAlgorithm",
    "StochasticQuantClientEndpoint",
    "TopKErrorFeedback",
    "TopKSparseEndpoint",
    "add_dp_noise",
    "add_dp_noise_to_parameter",
    "compute_dp_sigma",
    "get_message_size",
    "normal_stream",
    "philox_uniforms",
    "topk_sparsify",
    "topk_sparsify_parameter",
]


def _register_builtin() -> None:
    """The reference registers "fed_avg" at import (common_method/__init__.py:6-11). The
    client class is the simulator's worker, outside this package: it is left as None."""
    if not AlgorithmRepository.has_algorithm("fed_avg"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_avg",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=FedAVGAlgorithm,
        )
    # the robust rules (not reference algorithms): the same server, another aggregation rule
    for name, mode in (("fed_trimmed_mean", "trimmed_mean"), ("fed_median", "median")):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=functools.partial(RobustFedAVGAlgorithm, mode=mode),
            )
    # Krum (one client kept) and Multi-Krum (num_selected=None: n - f clients, resolved per round)
    for name, selected in (("krum", 1), ("multi_krum", None)):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=functools.partial(KrumFedAVGAlgorithm, num_selected=selected),
            )
    # the geometric median (RFA): smoothed Weiszfeld iterations over the same server
    if not AlgorithmRepository.has_algorithm("fed_geometric_median"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_geometric_median",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=GeometricMedianFedAVGAlgorithm,
        )
    # centred clipping about the previous global model: the radius has no default, so the entry
    # is the class itself and the caller binds it (functools.partial(entry, radius=...))
    if not AlgorithmRepository.has_algorithm("fed_centered_clipping"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_centered_clipping",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=ClippedFedAVGAlgorithm,
        )
    # Bulyan: iterated Krum, then per coordinate the mean of the values around the median
    if not AlgorithmRepository.has_algorithm("fed_bulyan"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_bulyan",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=BulyanFedAVGAlgorithm,
        )
    # FLTrust: cosine trust scores against the root worker's update; the root worker has no default,
    # so the entry is the class itself and the caller binds it (functools.partial(entry, root_worker=...))
    if not AlgorithmRepository.has_algorithm("fed_fltrust"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_fltrust",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=FLTrustFedAVGAlgorithm,
        )
    # the FedOpt server optimisers (Reddi et al.): the learning rate of the adaptive ones has no
    # default, so the caller binds it (functools.partial(entry, learning_rate=...)); "fed_avgm" runs
    # as it is, at learning rate 1.0
    for name, optimizer in (("fed_avgm", "avgm"), ("fed_adagrad", "adagrad"), ("fed_yogi", "yogi"),
                            ("fed_adam", "adam")):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=functools.partial(ServerOptFedAVGAlgorithm, optimizer=optimizer),
            )
    # FedAvg over sparsified parameter diffs (top-k clients with error feedback), folded as they are
    if not AlgorithmRepository.has_algorithm("fed_avg_sparse"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_avg_sparse",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=SparseFedAVGAlgorithm,
        )
    # the reference's federated-GNN server (graph_worker): topology exchange, embedding exchange, FedAvg
    if not AlgorithmRepository.has_algorithm("fed_graph"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_graph",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=GraphAlgorithm,
        )
    # FedAvg whose workers clip and noise their updates before sending (the Gaussian mechanism): the
    # plain server and rule behind the differential-privacy client endpoint
    if not AlgorithmRepository.has_algorithm("fed_avg_dp"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_avg_dp",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            client_endpoint_cls=DifferentialPrivacyParameterEndpoint,
            algorithm_cls=FedAVGAlgorithm,
        )
    # sparse FedAvg whose workers sparsify their diffs before sending (top-k with error feedback): the
    # sparse rule behind the top-k client endpoint
    if not AlgorithmRepository.has_algorithm("fed_avg_sparse_topk"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_avg_sparse_topk",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            client_endpoint_cls=TopKSparseEndpoint,
            algorithm_cls=SparseFedAVGAlgorithm,
        )
    # FedAvg whose workers send their updates, and receive the broadcast, as QSGD or NNADQ records: the
    # plain server and rule (which folds records as they are) behind the quantised client endpoints. The
    # NNADQ weight has no default: the caller binds it through the endpoint's keyword arguments
    for name, endpoint_cls in (("fed_avg_qsgd", StochasticQuantClientEndpoint), ("fed_avg_nnadq", NNADQClientEndpoint)):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                client_endpoint_cls=endpoint_cls,
                algorithm_cls=FedAVGAlgorithm,
            )


_register_builtin()
