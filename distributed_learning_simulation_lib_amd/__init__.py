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
    FoolsGoldFedAVGAlgorithm,
    GeometricMedianFedAVGAlgorithm,
    GraphAlgorithm,
    GraphNodeEmbeddingPassingAlgorithm,
    GraphTopologyAlgorithm,
    KrumFedAVGAlgorithm,
    LowRankFedAVGAlgorithm,
    MXFedAVGAlgorithm,
    PersonalizedFedAVGAlgorithm,
    RobustFedAVGAlgorithm,
    RotatedSignFedAVGAlgorithm,
    SecAggFedAVGAlgorithm,
    ServerOptFedAVGAlgorithm,
    SignFedAVGAlgorithm,
    SignMajorityVoteAlgorithm,
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
from .lowrank import (
    LowRankDelta,
    LowRankEndpoint,
    LowRankErrorFeedback,
    lowrank_compress,
    lowrank_compress_parameter,
)
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
from .mx import MXDelta, MXEndpoint, MXErrorFeedback, mx_compress, mx_compress_parameter
from .rotated import (
    RotatedSignDelta,
    RotatedSignEndpoint,
    RotatedSignErrorFeedback,
    rotated_sign_compress,
    rotated_sign_compress_parameter,
)
from .quantized import (
    BroadcastDequantizer,
    BroadcastQuantizer,
    NNADQClientEndpoint,
    QuantClientEndpoint,
    StochasticQuantClientEndpoint,
    philox_uniforms,
)
from .secagg import MaskedDelta, SecAggEndpoint, SecAggSession, secagg_mask_parameter
from .sign import SignDelta, SignEndpoint, SignErrorFeedback, sign_compress, sign_compress_parameter
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
    "FoolsGoldFedAVGAlgorithm",
    "GeometricMedianFedAVGAlgorithm",
    "GraphAlgorithm",
    "GraphNodeEmbeddingPassingAlgorithm",
    "GraphTopologyAlgorithm",
    "KrumFedAVGAlgorithm",
    "LowRankDelta",
    "LowRankEndpoint",
    "LowRankErrorFeedback",
    "LowRankFedAVGAlgorithm",
    "MXDelta",
    "MXEndpoint",
    "MXErrorFeedback",
    "MXFedAVGAlgorithm",
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
    "RotatedSignDelta",
    "RotatedSignEndpoint",
    "RotatedSignErrorFeedback",
    "RotatedSignFedAVGAlgorithm",
    "SecAggEndpoint",
    "SecAggFedAVGAlgorithm",
    "SecAggSession",
    "ServerOptFedAVGAlgorithm",
    "SignDelta",
    "SignEndpoint",
    "SignErrorFeedback",
    "SignFedAVGAlgorithm",
    "SignMajorityVoteAlgorithm",
    "SparseDelta",
    "SparseFedAVGAlgorithm",
    "StochasticQuantClientEndpoint",
    "TopKErrorFeedback",
    "TopKSparseEndpoint",
    "add_dp_noise",
    "add_dp_noise_to_parameter",
    "compute_dp_sigma",
    "get_message_size",
    "lowrank_compress",
    "lowrank_compress_parameter",
    "mx_compress",
    "mx_compress_parameter",
    "normal_stream",
    "philox_uniforms",
    "rotated_sign_compress",
    "rotated_sign_compress_parameter",
    "secagg_mask_parameter",
    "sign_compress",
    "sign_compress_parameter",
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
    # FoolsGold: the look-alikes among the clients' accumulated updates are down-weighted (a sybil defence)
    if not AlgorithmRepository.has_algorithm("fed_foolsgold"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_foolsgold",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            algorithm_cls=FoolsGoldFedAVGAlgorithm,
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
    # FedAvg over 1-bit sign deltas, folded from the bits, and the same with workers that compress their
    # diffs before sending (scaled sign with error feedback): the sign rule behind the sign endpoint
    for name, endpoint in (("fed_avg_sign", {}), ("fed_avg_sign_ef", {"client_endpoint_cls": SignEndpoint})):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=SignFedAVGAlgorithm,
                **endpoint,
            )
    # signSGD with majority vote over the same 1-bit deltas, and the same behind the sign endpoint: the
    # step has no default, so the entry is the class itself and the caller binds it
    # (functools.partial(entry, learning_rate=...))
    for name, endpoint in (("fed_sign_majority", {}), ("fed_sign_majority_ef", {"client_endpoint_cls": SignEndpoint})):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=SignMajorityVoteAlgorithm,
                **endpoint,
            )
    # FedAvg over low-rank factor pairs, folded from the factors, and the same with workers that compress
    # their diffs before sending (one power-iteration step with error feedback, rank 4 unless the caller
    # binds another through the endpoint's keyword arguments)
    for name, endpoint in (("fed_avg_lowrank", {}), ("fed_avg_lowrank_ef", {"client_endpoint_cls": LowRankEndpoint})):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=LowRankFedAVGAlgorithm,
                **endpoint,
            )
    # FedAvg over MX block-scaled deltas (FP8 / FP4 codes under E8M0 block scales), folded from the codes,
    # and the same with workers that compress their diffs before sending (MXFP8 with error feedback unless
    # the caller binds fmt="mxfp4" through the endpoint's keyword arguments)
    for name, endpoint in (("fed_avg_mx", {}), ("fed_avg_mx_ef", {"client_endpoint_cls": MXEndpoint})):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=MXFedAVGAlgorithm,
                **endpoint,
            )
    # FedAvg over randomly rotated 1-bit deltas, folded in the rotated domain, and the same with workers that
    # compress their diffs before sending: the caller binds the session's seed through the endpoint's keyword
    # arguments (endpoint_kwargs: {seed}), the same on every client
    for name, endpoint in (("fed_avg_rsign", {}), ("fed_avg_rsign_ef", {"client_endpoint_cls": RotatedSignEndpoint})):
        if not AlgorithmRepository.has_algorithm(name):
            from .server import AggregationServer

            AlgorithmRepository.register_algorithm(
                algorithm_name=name,
                client_cls=None,  # type: ignore[arg-type]
                server_cls=AggregationServer,
                algorithm_cls=RotatedSignFedAVGAlgorithm,
                **endpoint,
            )
    # FedAvg under secure aggregation: the unmasking rule behind the masking endpoint. The session seed has no
    # default: the caller binds it on both sides (functools.partial(entry, session_seed=...) and the endpoint's
    # keyword arguments session_seed, frac_bits, value_bits)
    if not AlgorithmRepository.has_algorithm("fed_avg_secagg"):
        from .server import AggregationServer

        AlgorithmRepository.register_algorithm(
            algorithm_name="fed_avg_secagg",
            client_cls=None,  # type: ignore[arg-type]
            server_cls=AggregationServer,
            client_endpoint_cls=SecAggEndpoint,
            algorithm_cls=SecAggFedAVGAlgorithm,
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
