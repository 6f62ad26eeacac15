/*
 * fedavg_hip.h — C ABI of the MI355X-native FedAvg aggregation path.
 *
 * This is the drop-in boundary for the server-side weighted FedAvg reduction of
 * cyyever/distributed_learning_simulation_lib. Every entry point below replaces one
 * piece of the reference's Python hot path (paths relative to the reference root):
 *
 *   fedavg_accumulate    <- FedAVGAlgorithm.process_worker_data / _accumulate_parameter
 *                           simulation_lib/algorithm/fed_avg_algorithm.py:20-64
 *   fedavg_aggregate     <- FedAVGAlgorithm._aggregate_parameter / _apply_total_weight
 *                           simulation_lib/algorithm/fed_avg_algorithm.py:71-99
 *   fedavg_weighted_avg  <- AggregationAlgorithm.weighted_avg (ratio path, accumulate=False)
 *                           simulation_lib/algorithm/aggregation_algorithm.py:51-76
 *   fedavg_partial       <- the per-shard half of _accumulate_parameter when clients are
 *                           sharded across GPUs (fp64 partial sum, no division)
 *   fedavg_*_delta       <- DeltaParameterMessage.restore fused into the fold (message.py:40-61,
 *                           aggregation_server.py:121-125)
 *   fedavg_check         <- the NaN assertions fed_avg_algorithm.py:35,93,97
 *   fedavg_find_nan_clients <- which client tripped fed_avg_algorithm.py:35
 *
 * Conventions
 *  - Plain C types only. Device pointers are `const void*` / `void*`; a stream is a
 *    `hipStream_t` passed as `void*` (NULL = the legacy default stream).
 *  - A "layout" is the ordered list of named tensors of one model (the keys of
 *    ParameterMessage.parameter, message.py:24-31). Segment t has seg_numel[t] elements.
 *  - A client table is row-major [num_clients][num_segments] of device pointers; a NULL
 *    entry means "this client did not send this tensor" (it is skipped, exactly like a
 *    missing key in the reference's per-name dictionaries, fed_avg_algorithm.py:56-62).
 *  - Weights are fp64, [num_clients][num_segments] (the value _get_weight returns for
 *    that (client, tensor), fed_avg_algorithm.py:66-69).
 *  - Accumulation is fp64 in arrival order: acc = x0*w0, then acc = acc + xk*wk, with the
 *    product and the sum each rounded (no FMA), exactly the reference's
 *    `tmp = x.to(f64) * w; acc += tmp`. Results are bit-identical to the reference for the
 *    single-GPU kernels.
 *  - Every call is asynchronous on `stream`. Arithmetic faults (NaN) are latched in a
 *    device flag and reported by fedavg_check(), which synchronises the stream.
 *  - Return value: FEDAVG_OK (0) or a negative/positive status below; the text of the
 *    last error of the calling thread is returned by fedavg_last_error().
 *  - The library never frees caller memory. Client buffers must stay valid until the
 *    call's stream work completes. One host thread per context.
 */
#ifndef FEDAVG_HIP_H
#define FEDAVG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAVG_ABI_VERSION 1

/* element types */
enum fedavg_dtype {
  FEDAVG_F32 = 0,
  FEDAVG_F16 = 1,
  FEDAVG_BF16 = 2,
  FEDAVG_F64 = 3,
  /* Quantised client records (server-side dequantisation fused into the fold,
   * StochasticQuantServerEndpoint.get, simulation_lib/topology/quantized_endpoint.py:69-77 and
   * :102-111). A client "tensor" pointer then points at one QSGD record of the tensor
   * (16-byte aligned, fedavg_qsgd_record_bytes(numel) bytes):
   *   [0, 8)   norm, fp64 (for FEDAVG_QSGD_F32 an fp32 value held exactly)
   *   [8, 12)  quantisation level s, int32 in [1, 255] (the reference uses 255)
   *   [16, 16 + numel)             slot per element, uint8 in [0, s]
   *   [fedavg_qsgd_sign_offset(numel), + ceil(numel / 8))  sign bits in numpy.packbits order
   *            (element i: byte i / 8, bit 7 - i % 8; 1 = non-negative)
   * The dequantised element is x = ((norm * sign) * slot) / s computed in fp32 (QSGD_F32) or
   * fp64 (QSGD_F64) — the codec's dtype — and is then folded exactly like a dense input
   * (tmp = x.to(f64) * w; acc += tmp). Accepted by every fold entry point except the delta
   * ones; split policies do not apply. */
  FEDAVG_QSGD_F32 = 4,
  FEDAVG_QSGD_F64 = 5,
  /* NNADQ records (NNADQServerEndpoint, quantized_endpoint.py:114-142, dequantised by
   * QuantServerEndpoint.get :69-77): a deterministic per-tensor affine code, 16-byte aligned,
   * fedavg_nnadq_record_bytes(numel) bytes:
   *   [0, 8)   lo, fp64 (for FEDAVG_NNADQ_F32 an fp32 value held exactly)
   *   [8, 16)  step, fp64 (likewise)
   *   [16, 20) levels L, int32 in [1, 255] (codes are in [0, L])
   *   [32, 32 + numel)  code per element, uint8
   * The dequantised element is x = code * step + lo (two roundings) in fp32 (NNADQ_F32) or
   * fp64 (NNADQ_F64), then folded exactly like a dense input. Same entry points as QSGD. */
  FEDAVG_NNADQ_F32 = 6,
  FEDAVG_NNADQ_F64 = 7,
};

/* status codes */
enum fedavg_status {
  FEDAVG_OK = 0,
  FEDAVG_ERR_NAN_INPUT = 1,    /* a client tensor holds NaN   (fed_avg_algorithm.py:35) */
  FEDAVG_ERR_NAN_ACCUM = 2,    /* accumulator became NaN      (fed_avg_algorithm.py:93) */
  FEDAVG_ERR_NAN_RESULT = 3,   /* acc / total_weight is NaN   (fed_avg_algorithm.py:97) */
  FEDAVG_ERR_INVALID = 4,      /* bad argument / dtype / size */
  FEDAVG_ERR_HIP = 5,          /* HIP runtime error */
  FEDAVG_ERR_STATE = 6,        /* e.g. aggregate with nothing accumulated (:88 assert) */
  FEDAVG_ERR_RCCL = 7,         /* RCCL missing or a collective failed (sharded path) */
};

/* flag bits latched by the kernels (read through fedavg_check) */
#define FEDAVG_FLAG_ACC_NAN 0x1u
#define FEDAVG_FLAG_RESULT_NAN 0x2u
#define FEDAVG_FLAG_CENTRAL_NAN 0x4u /* personalized path: the centralized average */
#define FEDAVG_FLAG_INPUT_NAN 0x8u   /* robust rules: a client tensor holds NaN */

typedef struct fedavg_ctx fedavg_ctx;

int32_t fedavg_abi_version(void);

/* Compile-time variants the library was built with: 0 for the product build. Non-zero bits
 * mark timing-only ablation builds whose results are WRONG by design (the kernel A/B studies of
 * rounds 1-3; their sources are no longer shipped, so this build always reports 0):
 * FEDAVG_BUILD_ABLATE_EPILOGUE (reciprocal multiply, no NaN checks), FEDAVG_BUILD_ABLATE_QSGD.
 * Bindings refuse to load such a build unless asked to (_native.py). */
#define FEDAVG_BUILD_ABLATE_EPILOGUE 0x1
#define FEDAVG_BUILD_ABLATE_QSGD 0x2
int32_t fedavg_build_flags(void);

/* A compile-time constant of the kernels' geometry, by name, into *out (test support: the
 * property tests place their sizes around every edge the kernels have, derived from the build
 * instead of copied into the tests). Names: "tile", "tile_wide", "split_tile"; per input dtype
 * d in {f32, f16, bf16, f64}: "ae_<d>", "lanes_<d>" (elements per lane / lanes per tile of the
 * whole-layout table), "ae4096_<d>", "lanes4096_<d>" (the 4096-element table), "group_<d>"
 * (clients loaded per group), "pipe_<d>" (clients per pipeline stage, 0 = no pipeline);
 * "qsgd_tile", "qsgd_ae", "qsgd_group"; "nnadq_tile", "nnadq_ae", "nnadq_group",
 * "nnadq_header"; "pers_chunk", "pers_jb" (receivers per wave),
 * "pers_group" (receivers per launch), "pers_u", "pers_ring_stage", "pers_ring_depth";
 * "robust_tile", "robust_lanes", "robust_max_clients" and "robust_ae_<d>" (elements of one 16-byte
 * load: what a lane sorts per pass over its tile) of fedavg_robust_aggregate;
 * "krum_chunk" (elements per workgroup), "krum_tile" (elements staged per step), "krum_block"
 * (clients per row / column block), "krum_reg" (edge of a lane's pair block), "krum_threads",
 * "krum_max_clients" and "krum_ae_<d>" (elements of one 16-byte load) of fedavg_pairwise_sqdist;
 * "point_chunk" (elements per workgroup), "point_threads", "point_batch" (clients between two
 * workgroup barriers: it does not enter the summation order), "point_max_clients" and
 * "point_ae_<d>" (elements of one 16-byte load) of fedavg_sqdist_to_point;
 * "clip_tile" (elements per workgroup), "clip_threads", "clip_max_clients" and "clip_ae_<d>"
 * (elements of one 16-byte load) of fedavg_fold_about_point;
 * "mam_tile", "mam_lanes" and "mam_ae_<d>" (as the "robust_" ones) of fedavg_mean_around_median;
 * "trust_chunk" (elements per workgroup: equal to "point_chunk"), "trust_threads", "trust_batch"
 * (clients between two workgroup barriers: it does not enter the summation order),
 * "trust_max_clients" and "trust_ae_<d>" (elements of one 16-byte load) of
 * fedavg_moments_about_point;
 * "opt_tile" (elements per workgroup), "opt_threads", "opt_max_clients" and "opt_ae_<d>" (elements
 * of one 16-byte load) of fedavg_server_opt_step;
 * "sparse_tile" (elements per workgroup), "sparse_threads", "sparse_batch" (clients between two
 * pairs of workgroup barriers = LDS planes: it does not enter the result) and "sparse_max_clients"
 * of fedavg_sparse_aggregate_delta;
 * "route_chunk" (wanted ids per workgroup of the rank walk), "route_threads", "route_max_sources" and
 * "route_max_node_space" of fedavg_route_rows;
 * "quant_tile" (elements per workgroup), "quant_threads" and "quant_per_lane" (consecutive elements a
 * lane encodes) of fedavg_quant_encode, and of fedavg_quant_decode (a lane decodes as many);
 * "dp_tile" (elements per piece of a sum and per workgroup of the apply pass), "dp_threads" (lanes
 * that share a piece) and "dp_ae_<d>" (elements of one 16-byte group: what a lane adds in a row) of
 * fedavg_dp_noise;
 * "topk_tile" (elements per workgroup of the write pass: the unit of the per-tile counts),
 * "topk_chunk" (consecutive tiles per workgroup of the histogram and count passes) and
 * "topk_threads" of fedavg_topk_sparsify.
 * FEDAVG_ERR_INVALID for an unknown name. */
int32_t fedavg_kernel_constant(const char* name, int64_t* out);

/* Byte size of one QSGD record of a numel-element tensor, and the offset of its sign bits
 * (see FEDAVG_QSGD_F32). Pure functions; -1 for numel < 0. */
int64_t fedavg_qsgd_record_bytes(int64_t numel);
int64_t fedavg_qsgd_sign_offset(int64_t numel);
/* Byte size of one NNADQ record of a numel-element tensor (see FEDAVG_NNADQ_F32); -1 for
 * numel < 0. */
int64_t fedavg_nnadq_record_bytes(int64_t numel);
const char* fedavg_last_error(void);

/*
 * Create a context for one model layout on one device.
 *  seg_numel[num_segments]: element count of each named tensor, in dict order.
 *  accumulator: optional caller-owned fp64 device buffer of fedavg_acc_numel() elements
 *               (e.g. a torch tensor, so a collective can run on it); NULL = the context
 *               allocates its own.
 * The fp64 accumulator uses a padded flat layout: segment t starts at
 * fedavg_segment_offset(ctx, t), a multiple of FEDAVG_ACC_ALIGN elements (256 bytes: every
 * tile boundary in accumulator coordinates is then divisible by 32, so the scatter exchange of
 * the multi-GPU round splits a chunk evenly over 2 / 4 / 8 ranks with 16-B aligned windows).
 * fedavg_layout_acc_numel gives the size before a context exists (for caller-owned buffers).
 */
#define FEDAVG_ACC_ALIGN 32
int64_t fedavg_layout_acc_numel(const int64_t* seg_numel, int32_t num_segments);
int32_t fedavg_ctx_create(fedavg_ctx** out, int32_t device, const int64_t* seg_numel,
                          int32_t num_segments, void* accumulator);
int32_t fedavg_ctx_destroy(fedavg_ctx* ctx);
int64_t fedavg_acc_numel(const fedavg_ctx* ctx);
int64_t fedavg_segment_offset(const fedavg_ctx* ctx, int32_t seg);
void* fedavg_accumulator(const fedavg_ctx* ctx);

/* Summation-order policy:
 *  1 = (default) the exact client-order kernel: bit-identical to the reference;
 *  0 = auto: the LDS split-client kernel when the layout is too small to fill the chip
 *      (< 512 tiles of 2048 elements) and a call carries >= 16 clients, else exact order;
 *  2 = the split-client kernel whenever a call carries >= 4 clients.
 * The split kernel reorders the fp64 sum (four wave partials combined in LDS). */
int32_t fedavg_set_split_policy(fedavg_ctx* ctx, int32_t policy);

/* Fused fold (default on): when every product x*w of a call is exact in fp64 — the weight's
 * significand fits next to the input's (fp32 x: weights with <= 29 significant bits, e.g.
 * integer dataset sizes < 2^29; fp16/bf16 x: <= 42 / 45 bits) — the kernel folds with one
 * fma(x, w, acc), which rounds exactly like the reference's acc + round(x*w). Otherwise (or
 * when disabled) the product and the sum are rounded separately. Results are identical
 * either way; this only trades VALU work. */
int32_t fedavg_set_fused_fold(fedavg_ctx* ctx, int32_t enable);

/* Forget accumulated state and the NaN flag (AggregationAlgorithm.clear_worker_data,
 * aggregation_algorithm.py:107-109). Asynchronous on stream. */
int32_t fedavg_reset(fedavg_ctx* ctx, void* stream);

/* Host-side per-segment total weight so far (fed_avg_algorithm.py:59-62). out[num_segments]. */
int32_t fedavg_total_weights(const fedavg_ctx* ctx, double* out);

/*
 * Streaming accumulate of a wave of clients into the fp64 accumulator, in table order.
 * Equivalent to calling _accumulate_parameter for every (client, tensor) of the wave in
 * arrival order (fed_avg_algorithm.py:43-64). Per-segment total weights accumulate on the
 * host in the same order.
 */
int32_t fedavg_accumulate(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                          const double* weights, int32_t num_clients, void* stream);

/*
 * Finish the round: optionally fold a last wave of clients (num_clients may be 0), then
 * out[t] = acc[t] / total_weight[t] converted to out_dtype (FEDAVG_F32 or FEDAVG_F64),
 * written through out_ptrs[num_segments] (device pointers). Resets the accumulator state
 * (fed_avg_algorithm.py:88-99). The acc and result NaN checks are fused in the kernel.
 * FEDAVG_ERR_STATE if nothing was ever accumulated for some segment (the :88 assert).
 */
int32_t fedavg_aggregate(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                         const double* weights, int32_t num_clients, void* const* out_ptrs,
                         int32_t out_dtype, void* stream);

/*
 * Delta updates (DeltaParameterMessage, message.py:34-61): every client tensor of the call is a
 * delta against the server's cached global model `base_ptrs[num_segments]` (fp64 device
 * tensors, e.g. the ModelCache copy, util/model_cache.py:27-34). The fold uses
 * x = base + delta (fp64, rounded — exactly restore()'s `old.to(float64) + v`, message.py:54),
 * fusing the restore into the reduce: the base is read once per tile instead of one restored
 * fp64 copy per client. Otherwise identical to fedavg_accumulate / fedavg_aggregate (arrival
 * order is preserved across mixed full/delta calls because the accumulator carries over).
 */
int32_t fedavg_accumulate_delta(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                const double* weights, int32_t num_clients,
                                const void* const* base_ptrs, void* stream);
int32_t fedavg_aggregate_delta(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                               const double* weights, int32_t num_clients,
                               const void* const* base_ptrs, void* const* out_ptrs,
                               int32_t out_dtype, void* stream);

/*
 * Non-streaming ratio path (accumulate=False): out = sum_k ratio[k] * x_k in fp64, no
 * division (aggregation_algorithm.py:51-76). `ratios` is [num_clients][num_segments];
 * the caller computes ratios exactly like get_ratios (aggregation_algorithm.py:42-49).
 * Does not touch the accumulator.
 */
int32_t fedavg_weighted_avg(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                            const double* ratios, int32_t num_clients, void* const* out_ptrs,
                            int32_t out_dtype, void* stream);

/*
 * Multi-GPU shard step: acc[tiles in [tile_begin, tile_end)] = (acc_in ? acc : 0) +
 * sum_k w_k x_k, fp64, written to the accumulator (no division); acc_in = the context holds
 * accumulated data for the segment (earlier waves through fedavg_accumulate, or
 * fedavg_set_accumulated) and zero_init == 0. Used by the sharded
 * driver that reduces the per-GPU partials with RCCL and then calls fedavg_aggregate
 * with num_clients = 0 on the root. tile_end = -1 means "all tiles". zero_init != 0 starts
 * every segment at the additive identity -0.0 (so the shard's fold is exact, and a shard
 * without clients contributes identities).
 */
int32_t fedavg_partial(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                       const double* weights, int32_t num_clients, int32_t zero_init,
                       int32_t tile_begin, int32_t tile_end, void* stream);
/* Number of tiles and the accumulator element range [*acc_begin, *acc_end) of tiles
 * [tile_begin, tile_end), for chunking a collective over the partial. */
int32_t fedavg_num_tiles(const fedavg_ctx* ctx);
int32_t fedavg_tile_range(const fedavg_ctx* ctx, int32_t tile_begin, int32_t tile_end,
                          int64_t* acc_begin, int64_t* acc_end);
/* Declare that segments' accumulators hold data and add host totals (after an external
 * collective summed partials into the accumulator): total_weights[num_segments]. */
int32_t fedavg_set_accumulated(fedavg_ctx* ctx, const double* total_weights);
/* Finalize only tiles [tile_begin, tile_end) of the accumulator into out_ptrs (used to
 * pipeline finalize behind a chunked collective). Does not reset state. */
int32_t fedavg_finalize_range(fedavg_ctx* ctx, void* const* out_ptrs, int32_t out_dtype,
                              int32_t tile_begin, int32_t tile_end, void* stream);

/*
 * Prepared aggregation ("plan"): the client table, weights and outputs of a
 * fedavg_aggregate call are validated, compacted and uploaded ONCE; fedavg_plan_run then
 * launches the fused fold + divide with no host staging (persistent client slots, e.g. a
 * server that reuses its device buffers round after round). A run is exactly
 * fedavg_aggregate(ctx, <the planned arguments>) on a context with nothing accumulated.
 * The buffers named by the plan must outlive it.
 */
typedef struct fedavg_plan fedavg_plan;
int32_t fedavg_plan_create(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                           const double* weights, int32_t num_clients, void* const* out_ptrs,
                           int32_t out_dtype, fedavg_plan** out);
int32_t fedavg_plan_run(fedavg_plan* plan, void* stream);
int32_t fedavg_plan_destroy(fedavg_plan* plan);
/* Plans for the multi-GPU shard step, launched per tile range (chunked collective):
 * a partial plan is fedavg_partial(ctx, <clients>, zero_init, tb, te); a finalize plan is
 * fedavg_finalize_range with the given per-segment total weights baked in. */
int32_t fedavg_plan_create_partial(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                   const double* weights, int32_t num_clients, int32_t zero_init,
                                   fedavg_plan** out);
int32_t fedavg_plan_create_finalize(fedavg_ctx* ctx, const double* total_weights,
                                    void* const* out_ptrs, int32_t out_dtype, fedavg_plan** out);
int32_t fedavg_plan_run_range(fedavg_plan* plan, int32_t tile_begin, int32_t tile_end, void* stream);

/*
 * Move accumulated state between contexts (a layout that grows when a tensor name first appears
 * in a later client, fed_avg_algorithm.py:55-62): per segment, valid[t] != 0 marks the
 * accumulator as holding data with total weight total_weights[t] (NULL: -0.0); valid[t] == 0
 * makes the next fold of that segment an assignment.
 */
int32_t fedavg_set_segment_state(fedavg_ctx* ctx, const double* total_weights, const int32_t* valid);
/* The reverse: per segment the host total weight so far and whether the accumulator holds data
 * (total_weights[num_segments], valid[num_segments]; either may be NULL). */
int32_t fedavg_segment_state(const fedavg_ctx* ctx, double* total_weights, int32_t* valid);

/*
 * Per-element weights (a _get_weight override returning a tensor of the parameter's shape,
 * fed_avg_algorithm.py:51-62, divided elementwise at :94-96):
 *   acc[e] = (acc_in ? acc[e] + round(x[e] * w[e]) : round(x[e] * w[e]))
 *   tot[e] = (acc_in ? tot[e] + w[e] : w[e]), rounded to fp32 after every add when
 *            total_fp32[t] (the reference keeps the total in the first weight's dtype)
 * weight_ptrs[K][T]: device fp32 / fp64 (weight_dtypes[K][T]) tensors of the segment's size, or
 * NULL = the scalar scalar_weights[k][t]; totals: fp64 device buffer in accumulator coordinates
 * (fedavg_acc_numel elements), owned by the caller. fedavg_finalize_elementwise writes
 * out = acc / tot (IEEE, fp32 / fp64), with the :93 / :97 NaN checks, and resets the state.
 */
int32_t fedavg_accumulate_elementwise(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                      const void* const* weight_ptrs, const int32_t* weight_dtypes,
                                      const double* scalar_weights, const int32_t* total_fp32, int32_t num_clients,
                                      void* totals, void* stream);
int32_t fedavg_finalize_elementwise(fedavg_ctx* ctx, const void* totals, void* const* out_ptrs, int32_t out_dtype,
                                    void* stream);

/* Pieces of the scatter exchange (fedavg_sharded_round_scatter; also usable from a host-driven
 * exchange, sharded.py). `finalize` is a finalize plan (its totals, outputs and out dtype).
 *  fedavg_plan_finalize_window: res[p] = src[p - lo] / W[seg(p)] for accumulator positions p in
 *      [lo, hi) that belong to a segment (padding is skipped); res is a buffer of the plan's out
 *      dtype in accumulator coordinates (fedavg_acc_numel elements); NaN checks as finalize.
 *  fedavg_plan_copy_out: the plan's outputs <- res (accumulator coordinates), every tile; a NaN
 *      in res raises the result flag (another rank's failed window reaches the root's check). */
int32_t fedavg_plan_finalize_window(fedavg_plan* finalize, const double* src, int64_t lo, int64_t hi, void* res,
                                    void* stream);
int32_t fedavg_plan_copy_out(fedavg_plan* finalize, const void* res, void* stream);
int32_t fedavg_plan_out_dtype(const fedavg_plan* plan); /* FEDAVG_F32 / FEDAVG_F64; -1 if none */

/*
 * Robust aggregation rules: the coordinate-wise trimmed mean and median of the clients' updates.
 * NOT an algorithm of the reference (it has none besides the weighted mean): the contract is
 * DESIGN.md "Robust rules", restated independently in tests/robust_reference.py.
 *
 * Per segment t, the n_t non-NULL entries of column t of client_ptrs[num_clients][num_segments]
 * count (1 <= n_t <= 64: each lane sorts an element's n_t values in registers). Per element the
 * values, converted exactly to fp64, are sorted in the IEEE total order (-inf < ... < -0.0 < +0.0
 * < ... < +inf) into s_0 <= ... <= s_{n-1}; with k = trim_k[t] (0 <= 2k < n_t) the result is
 *   (s_k + s_{k+1} + ... + s_{n-k-1}) / (n - 2k)
 * summed in ascending order from s_k, every add rounded in fp64 (no FMA), IEEE division.
 * mode FEDAVG_ROBUST_MEDIAN is that with k = (n_t - 1) / 2 (trim_k is ignored and may be NULL):
 * s_{(n-1)/2} for odd n, (s_{n/2-1} + s_{n/2}) / 2.0 for even n. No weights: both rules are
 * unweighted. out_ptrs[num_segments]: FEDAVG_F64, or FEDAVG_F32 = that fp64 result rounded to
 * nearest even. One launch over the whole layout; the accumulator is not touched. A NaN input
 * latches FEDAVG_FLAG_INPUT_NAN, a NaN result (+inf and -inf both kept) FEDAVG_FLAG_RESULT_NAN;
 * fedavg_check reports them. in_dtype: FEDAVG_F32 / F16 / BF16 / F64 (no records, no deltas).
 * FEDAVG_ERR_INVALID (bad mode / dtype / k, more than 64 clients for a segment, NULL tables),
 * FEDAVG_ERR_STATE (a segment no client sent; an open dynamic wave) — all before any launch.
 */
#define FEDAVG_ROBUST_TRIMMED_MEAN 0
#define FEDAVG_ROBUST_MEDIAN 1
#define FEDAVG_ROBUST_MAX_CLIENTS 64
int32_t fedavg_robust_aggregate(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                int32_t num_clients, int32_t mode, const int32_t* trim_k,
                                void* const* out_ptrs, int32_t out_dtype, void* stream);

/*
 * The mean around the median (MeaMed; Xie, Koyejo, Gupta, "Generalized Byzantine-tolerant SGD"):
 * per element the mean of the beta values closest to the median. It is the coordinate step of
 * Bulyan (El Mhamdi, Guerraoui, Rouault, ICML 2018). NOT an algorithm of the reference: the contract
 * is DESIGN.md §5k, restated independently in tests/bulyan_reference.py.
 *
 * Tables, dtypes and compaction as fedavg_robust_aggregate: per segment t the n_t non-NULL entries
 * of column t count (1 <= n_t <= 64), and beta = keep[t] with 1 <= keep[t] <= n_t (any beta, not
 * only those with n_t - beta even). Per element the values, converted exactly to fp64, are sorted
 * in the IEEE total order into s_0 <= ... <= s_{n-1}; med = s_{(n-1)/2}, the LOWER median (always
 * an input value). The window starts at
 *   a = #{ t in [0, n - beta) : (s_{t+beta} - med) < (med - s_t) }
 * with one rounded fp64 subtraction on each side and the IEEE comparison (false on NaN, i.e. on
 * inf - inf); the predicate holds on a prefix of t, so a is the first t at which it fails, and a
 * tie keeps the lower value. The result is (s_a + s_{a+1} + ... + s_{a+beta-1}) / beta: summed in
 * ascending order from s_a (no leading zero), every add rounded in fp64 (no FMA), IEEE division.
 * keep[t] == n_t is the plain sorted-order mean; keep[t] == 1 is the lower median (where a -0.0 lies
 * below a +0.0 median it ties with it and, as ties keep the lower value, -0.0 is returned).
 * out_ptrs[num_segments]: FEDAVG_F64, or FEDAVG_F32 = that fp64 result rounded to nearest even.
 * An element's result depends on its own n values and on beta only. One launch over the whole
 * layout, asynchronous on `stream`; the accumulator and its state are not touched; nothing outside
 * a tensor is read or written. A NaN input latches FEDAVG_FLAG_INPUT_NAN, a NaN result (+inf and
 * -inf both in a window) FEDAVG_FLAG_RESULT_NAN; fedavg_check reports them.
 * FEDAVG_ERR_INVALID (NULL tables, a bad dtype — records included —, num_clients < 1, a client
 * pointer not aligned to its element, more than 64 clients for a segment, keep NULL or out of
 * range), FEDAVG_ERR_STATE (a segment no client sent; an open dynamic wave) — all before any launch.
 */
int32_t fedavg_mean_around_median(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                  int32_t num_clients, const int32_t* keep,
                                  void* const* out_ptrs, int32_t out_dtype, void* stream);

/*
 * Pairwise squared distances between the clients' whole updates: the device half of Krum and
 * Multi-Krum (scores and selection are host arithmetic on the n x n result). NOT an algorithm of
 * the reference: the contract is DESIGN.md §5h, restated independently in tests/krum_reference.py.
 *
 * client_ptrs[num_clients][num_segments], every entry non-NULL (distances compare whole updates).
 *   out[i * n + j] = sum over every element e of every segment of (x_i[e] - x_j[e])^2
 * with each value converted exactly to fp64, one fp64 subtraction, and the square and add in fp64
 * (an FMA): never the norm / inner-product form, which cancels for updates that share a model.
 * All terms are non-negative, so each entry is within (P + 2) * 2^-53 relative of the exact value
 * (P = the layout's element count) whatever the order. The order is fixed all the same: within a
 * chunk of "krum_chunk" elements of a segment ascending element order into one accumulator per
 * pair, then the chunks in layout order; it depends on the layout only, never on the device or on
 * timing (no floating-point atomics), so the same inputs give the same bits. out is exactly
 * symmetric (i < j is computed and mirrored) with a +0.0 diagonal; num_clients == 1 writes one +0.0.
 * `out` is device memory, n * n doubles. Asynchronous on `stream`; the accumulator is not touched.
 * A NaN input latches FEDAVG_FLAG_INPUT_NAN (tested at the load). +inf / -inf inputs are legal
 * (that client's distances are +inf); two clients with a same-signed infinity in the same element
 * give inf - inf, which latches FEDAVG_FLAG_ACC_NAN. fedavg_check reports the flags.
 * in_dtype: FEDAVG_F32 / F16 / BF16 / F64 (no records, no deltas). Refused before any launch:
 * FEDAVG_ERR_INVALID (NULL table, entry or out; bad dtype; num_clients < 1 or >
 * FEDAVG_KRUM_MAX_CLIENTS), FEDAVG_ERR_STATE (an open dynamic wave).
 */
#define FEDAVG_KRUM_MAX_CLIENTS 256
int32_t fedavg_pairwise_sqdist(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                               int32_t num_clients, double* out /* [n][n], device */, void* stream);

/*
 * Squared distance of every client's whole update to one fp64 point: the device half of the
 * geometric median's Weiszfeld iteration (RFA), and with no point the clients' squared norms. NOT
 * an algorithm of the reference: the contract is DESIGN.md §5i, restated independently in
 * tests/geomed_reference.py.
 *
 * client_ptrs[num_clients][num_segments], every entry non-NULL. point_ptrs[num_segments] (a host
 * array): point_ptrs[t] is a device fp64 tensor of segment t's element count, 8-byte aligned;
 * point_ptrs == NULL is the origin (out[i] = |x_i|^2); a NULL entry inside a non-NULL point_ptrs is
 * FEDAVG_ERR_INVALID.
 *   out[i] = sum over every element e of every segment of (x_i[e] - z[e])^2
 * with each value converted exactly to fp64, then d = x - z, q = d * d, acc = acc + q: three
 * separately rounded fp64 operations, NO FMA (unlike fedavg_pairwise_sqdist: these distances become
 * continuous weights, so numpy and torch must be able to restate them bit for bit). All terms are
 * non-negative, so each entry is within (P + 2) * 2^-53 relative of the exact value (P = the
 * layout's element count) whatever the order. The order is fixed all the same. With C =
 * "point_chunk", L = "point_threads" and N = "point_ae_<d>" of the client dtype:
 *   - every segment is cut into chunks of C elements (its last chunk is shorter); a chunk's
 *     positions past its end count as x = z = +0.0, which adds +0.0 and changes no bit;
 *   - lane l (0 <= l < L) owns the positions (k * L + l) * N + i, k = 0 .. C / (N * L) - 1,
 *     i = 0 .. N - 1, and adds them in ascending order into one accumulator from +0.0;
 *   - the 64 lanes of a wave are combined by the halving tree a[l] <- a[l] + a[l + off],
 *     l < off, off = 32, 16, 8, 4, 2, 1; the L / 64 waves are added in wave order,
 *     ((w0 + w1) + w2) + w3;
 *   - the chunk partials are added sequentially from +0.0 in layout order (segment by segment,
 *     ascending offset) by a second kernel the stream orders after the first.
 * It depends on the layout and on in_dtype (through N) alone: never on num_clients, on the client's
 * row, on the other clients of the table, on the device or on timing (no floating-point atomics),
 * so the same inputs give the same bits. `out` is device memory, num_clients doubles. Asynchronous
 * on `stream`; the accumulator is not touched; nothing outside a tensor is read or written.
 * A NaN client or point value latches FEDAVG_FLAG_INPUT_NAN (tested at the load). +inf / -inf in a
 * client are legal (that client's entry is +inf). An infinite point element makes every finite
 * client's entry +inf and, against the same infinity in a client, inf - inf = NaN, which latches
 * FEDAVG_FLAG_ACC_NAN (tested on the result).
 * fedavg_check reports the flags. in_dtype: FEDAVG_F32 / F16 / BF16 / F64 (no records, no deltas).
 * Refused before any launch: FEDAVG_ERR_INVALID (NULL table, entry or out; bad dtype; a misaligned
 * pointer; num_clients < 1 or > FEDAVG_POINT_MAX_CLIENTS), FEDAVG_ERR_STATE (an open dynamic wave).
 */
#define FEDAVG_POINT_MAX_CLIENTS 1024
int32_t fedavg_sqdist_to_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                               int32_t num_clients, const double* const* point_ptrs /* [num_segments] or NULL */,
                               double* out /* [n], device */, void* stream);

/*
 * The fold about a point: the device half of centred clipping's step (Karimireddy, He, Jaggi,
 * "Learning from History for Byzantine Robust Optimization"; norm bounding is its one-iteration
 * case). NOT an algorithm of the reference: the contract is DESIGN.md §5j, restated independently in
 * tests/clip_reference.py.
 *
 * client_ptrs[num_clients][num_segments], every entry non-NULL; in_dtype FEDAVG_F32 / F16 / BF16 /
 * F64 (no records, no deltas). coefficients[num_clients] is a host array. point_ptrs[num_segments]
 * and out_ptrs[num_segments] are host arrays of device pointers: point_ptrs[t] an fp64 tensor of
 * segment t's element count, 8-byte aligned; out_ptrs[t] an out_dtype (FEDAVG_F32 / F64) tensor of
 * the same count. Per element e of every segment, with z the point and c the coefficients:
 *   d_i = x_i[e] - z[e];  p_i = c_i * d_i;  acc = p_0, then acc = acc + p_i for i = 1 .. n - 1 in
 *   table order;  r = acc / divisor (IEEE division);  out[e] = z[e] + r
 * with every client value converted exactly to fp64 and every operation a separately rounded fp64
 * operation: NO FMA, and no leading 0 + (the first product starts the sum, so a sum of -0.0
 * products stays -0.0: signed zeros come out as the five operations give them). An fp32 output is
 * the fp64 result rounded to nearest even.
 * The result depends on the element's own values, the coefficients in table order and the divisor
 * alone: never on the tiling, the other elements or tensors, the device, timing or earlier calls
 * (no atomics). Asynchronous on `stream`; the accumulator and its state are not touched; nothing
 * outside a tensor is read or written.
 * A NaN in a client or in the point latches FEDAVG_FLAG_INPUT_NAN (tested at the load); a NaN in acc
 * (a NaN input, inf - inf, 0 * inf) latches FEDAVG_FLAG_ACC_NAN; a NaN in the fp64 result latches
 * FEDAVG_FLAG_RESULT_NAN. fedavg_check reports the flags.
 * Refused before any launch: FEDAVG_ERR_INVALID (a NULL table, entry, point entry, out entry or
 * coefficient array; a bad dtype; a pointer not aligned to its element; num_clients < 1 or >
 * FEDAVG_POINT_MAX_CLIENTS; a non-finite coefficient; a divisor that is not finite and > 0;
 * out_ptrs[t] == point_ptrs[t]: the step is not in-place, callers ping-pong two buffers),
 * FEDAVG_ERR_STATE (an open dynamic wave).
 */
int32_t fedavg_fold_about_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                const double* coefficients /* [n], host */, int32_t num_clients,
                                double divisor,
                                const double* const* point_ptrs /* [num_segments], device fp64 */,
                                void* const* out_ptrs /* [num_segments], device */,
                                int32_t out_dtype, void* stream);

/*
 * The two moments of every client's whole update about one fp64 point: the device half of FLTrust's
 * trust scores (Cao, Fang, Liu, Gong, "FLTrust: Byzantine-robust Federated Learning via Trust
 * Bootstrapping", NDSS 2021). NOT an algorithm of the reference: the contract is DESIGN.md §5l,
 * restated independently in tests/trust_reference.py.
 *
 * client_ptrs[num_clients][num_segments], every entry non-NULL; in_dtype FEDAVG_F32 / F16 / BF16 /
 * F64 (no records, no deltas). centre_ptrs[num_segments] and direction_ptrs[num_segments] are host
 * arrays of device pointers to fp64 tensors of the segments' element counts, 8-byte aligned;
 * centre_ptrs == NULL is the origin, direction_ptrs is required. With v the centre and g the
 * direction, for client i and every element e of every segment:
 *   d = x_i[e] - v[e];  q = d * d;  p = d * g[e];  S_i = S_i + q;  T_i = T_i + p
 * with every client value converted exactly to fp64 and every operation a separately rounded fp64
 * operation, NO FMA. out[i] = T_i (the dots) and out[num_clients + i] = S_i (the squared norms);
 * `out` is device memory, 2 * num_clients doubles.
 * Both sums follow the summation order of fedavg_sqdist_to_point word for word, with C =
 * "trust_chunk" (== "point_chunk"), L = "trust_threads" and N = "trust_ae_<d>": chunks of C elements
 * per segment, padded with x = v = g = +0.0 (an accumulator that starts at +0.0 is never -0.0, so
 * the padding's +0.0 changes no bit of either sum); lane l owns the positions (k * L + l) * N + i in
 * ascending order, one accumulator per sum from +0.0; the halving tree over the 64 lanes of a wave;
 * the waves in wave order; the chunk partials sequentially from +0.0 in layout order, in a second
 * kernel the stream orders after the first. So out[num_clients + i] is bit for bit what
 * fedavg_sqdist_to_point returns for the same table and point, and a client's two entries depend on
 * the layout, in_dtype and its own values alone: never on num_clients, its row, the other clients,
 * the device or timing (no floating-point atomics). A dot's terms have both signs: it is within
 * (P + 2) * 2^-53 * sum_e |(x - v) * g| of the exact value (P = the layout's element count).
 * Asynchronous on `stream`; the accumulator is not touched; nothing outside a tensor is read or
 * written.
 * A NaN in a client, the centre or the direction latches FEDAVG_FLAG_INPUT_NAN (tested at the load);
 * a NaN in any output (inf - inf, 0 * inf, +inf + -inf in a dot) latches FEDAVG_FLAG_ACC_NAN (tested
 * on the result). fedavg_check reports the flags.
 * Refused before any launch, with the flags and `out` untouched: FEDAVG_ERR_INVALID (a NULL client
 * table, direction table or out; a NULL client, centre or direction entry; a bad dtype; a client
 * pointer not aligned to its element size; a centre, direction or out pointer not aligned to 8
 * bytes; num_clients < 1 or > FEDAVG_POINT_MAX_CLIENTS), FEDAVG_ERR_STATE (an open dynamic wave).
 */
int32_t fedavg_moments_about_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                   int32_t num_clients,
                                   const double* const* centre_ptrs /* [num_segments] fp64, or NULL: the origin */,
                                   const double* const* direction_ptrs /* [num_segments] fp64, required */,
                                   double* out /* [2][n], device: dots, then squared norms */, void* stream);

/*
 * The server optimiser step: the fold about a point with the FedOpt epilogue fused onto it (Reddi et
 * al., "Adaptive Federated Optimization", ICLR 2021: FedAvgM, FedAdagrad, FedYogi, FedAdam). NOT an
 * algorithm of the reference: the contract is DESIGN.md §5m, restated independently in
 * tests/opt_reference.py.
 *
 * client_ptrs, in_dtype, coefficients, num_clients, divisor, point_ptrs, out_ptrs and out_dtype are
 * those of fedavg_fold_about_point. m_in, v_in, m_out and v_out are host arrays [num_segments] of
 * device pointers to fp64 tensors of the segments' element counts, 8-byte aligned: the moments
 * before the step and where the moments after it are written. FEDAVG_OPT_AVGM keeps no second
 * moment: v_in and v_out are not read and may be NULL. one_minus_beta1 and one_minus_beta2 are
 * passed in (the caller computes 1 - beta once) so a restatement uses the very same doubles.
 * Per element e of every segment, with z the point, c the coefficients, m and v the moments:
 *   d_i = x_i[e] - z[e];  p_i = c_i * d_i;  acc = p_0, then acc = acc + p_i for i = 1 .. n - 1 in
 *   table order;  delta = acc / divisor       (so far bit for bit the r of fedavg_fold_about_point)
 *   AVGM:     a = beta1 * m;  m' = a + delta;                               u = lr * m'
 *   others:   a = beta1 * m;  b = one_minus_beta1 * delta;  m' = a + b;  q = delta * delta
 *     ADAGRAD:  v' = v + q
 *     ADAM:     e = beta2 * v;  f = one_minus_beta2 * q;  v' = e + f
 *     YOGI:     g = v - q;  s = +1.0 if g > 0, -1.0 if g < 0, else +0.0;
 *               f = one_minus_beta2 * q;  h = f * s;  v' = v - h
 *     r = sqrt(v');  den = r + tau;  num = lr * m';  u = num / den
 *   out[e] = z[e] + u;  m_out[e] = m';  v_out[e] = v'
 * with every client value converted exactly to fp64 and every line one separately rounded IEEE fp64
 * operation: NO FMA, no reciprocal, IEEE division, a correctly rounded square root, no bias
 * correction (the paper has none). An fp32 output is the fp64 result rounded to nearest even.
 * The results depend on the element's own values, the coefficients in table order, the divisor and
 * the hyper-parameters alone: never on the tiling, the other elements or tensors, the device,
 * timing or earlier calls (no atomics, no workspace, one kernel). Asynchronous on `stream`; the
 * accumulator and its state are not touched; nothing outside a tensor is read or written.
 * A NaN in a client, the point, m or v latches FEDAVG_FLAG_INPUT_NAN (tested at the load); a NaN in
 * acc latches FEDAVG_FLAG_ACC_NAN; a NaN in out, m' or v' latches FEDAVG_FLAG_RESULT_NAN. In the
 * adaptive modes an infinite client value makes u = inf / inf: it latches FEDAVG_FLAG_RESULT_NAN,
 * an error and not a drop. (FEDAVG_OPT_AVGM has no quotient: there it gives an infinite out and m'
 * and no flag, as the weighted mean itself would.) The step is not in-place: a caller ping-pongs
 * two buffers per moment and swaps them once fedavg_check came back clean, so a failed round leaves
 * its state intact.
 * Refused before any launch: FEDAVG_ERR_INVALID (everything fedavg_fold_about_point refuses; an
 * unknown mode; lr not finite or not > 0; beta1 or beta2 outside [0, 1); in the adaptive modes tau
 * not finite or not > 0; a NULL moment table or entry that the mode needs, or one not aligned to 8
 * bytes; for any segment out_ptrs[t] == point_ptrs[t], m_out[t] == m_in[t] or
 * v_out[t] == v_in[t]), FEDAVG_ERR_STATE (an open dynamic wave).
 */
#define FEDAVG_OPT_AVGM 0
#define FEDAVG_OPT_ADAGRAD 1
#define FEDAVG_OPT_YOGI 2
#define FEDAVG_OPT_ADAM 3
int32_t fedavg_server_opt_step(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                               const double* coefficients /* [n], host */, int32_t num_clients,
                               double divisor,
                               const double* const* point_ptrs /* [num_segments], device fp64 */,
                               const double* const* m_in, const double* const* v_in /* NULL for AVGM */,
                               double* const* m_out, double* const* v_out /* NULL for AVGM */,
                               int32_t mode, double lr, double beta1, double one_minus_beta1,
                               double beta2, double one_minus_beta2, double tau,
                               void* const* out_ptrs /* [num_segments], device */,
                               int32_t out_dtype, void* stream);

/*
 * The sparse delta fold: FedAvg over clients that send, per tensor, nnz (index, value) pairs of a
 * parameter diff against the server's cached global model (top-k sparsification with error
 * feedback on the client). A sparse delta is a DeltaParameterMessage whose missing entries are
 * +0.0, so the result is the reference's restore() (message.py:40-61) followed by FedAVGAlgorithm
 * (fed_avg_algorithm.py:43-99) on the densified delta, bit for bit, and bit for bit what
 * fedavg_aggregate_delta gives on the densified tensors. The contract is DESIGN.md §5n, restated
 * independently in tests/sparse_reference.py.
 *
 * index_ptrs[num_clients][num_segments] and value_ptrs[num_clients][num_segments] are host arrays of
 * device pointers; nnz[num_clients][num_segments] is a host array, 0 <= nnz <= the segment's element
 * count. An index array holds nnz STRICTLY INCREASING int32 flat positions in [0, element count),
 * 4-byte aligned; a value array nnz values of value_dtype (FEDAVG_F32 / F16 / BF16 / F64), aligned to
 * the element; both may be NULL only where nnz == 0. weights[num_clients] is a host array.
 * base_ptrs[num_segments] are fp64 tensors of the segments' element counts, 8-byte aligned (the
 * cached global model); out_ptrs[num_segments] out_dtype (FEDAVG_F32 / F64) tensors of the same
 * counts. Per element e of every segment, with b the base and w the weights:
 *   d_i = the value client i stores for e, converted exactly to fp64, or +0.0 if it has none
 *   x_i = b[e] + d_i   (performed even for d_i = +0.0, so b = -0.0 gives +0.0)
 *   p_i = x_i * w_i;  acc = p_0, then acc = acc + p_i for i = 1 .. n - 1 in table order
 *   out[e] = acc / divisor   (IEEE division)
 * every line one separately rounded fp64 operation: NO FMA, no leading 0 +. An fp32 output is the
 * fp64 result rounded to nearest even. The result depends on the element's base value, the entries
 * that name it, the weights in table order and the divisor alone: never on the tiling, the client
 * batch ("sparse_batch"), other elements, the device, timing or earlier calls (no atomics).
 * Asynchronous on `stream`; the accumulator and its state are not touched.
 * A NaN in any x_i (a NaN value, a NaN base, inf - inf) latches FEDAVG_FLAG_INPUT_NAN; a NaN in acc
 * latches FEDAVG_FLAG_ACC_NAN; a NaN in the fp64 result latches FEDAVG_FLAG_RESULT_NAN. fedavg_check
 * reports the flags.
 * Index violations (an index that is negative, >= the element count, or not greater than its
 * predecessor) are an input error: a pass over the index arrays in the same call latches a word of
 * the context's sparse state (not the NaN words), which fedavg_sparse_index_errors reports. The fold
 * is safe whatever the indices are: an entry reaches a tile only after its index has been checked to
 * lie inside that tile, otherwise it is dropped; nothing outside an output tensor is written and
 * nothing outside [0, nnz) of an index or value array is read. The outputs of a call that reports a
 * violation are unspecified.
 * Refused before any launch: FEDAVG_ERR_INVALID (a NULL table; a NULL index or value array with
 * nnz > 0; a bad dtype; a pointer not aligned to its element; nnz outside [0, element count];
 * num_clients < 1 or > FEDAVG_POINT_MAX_CLIENTS; a non-finite weight; a divisor that is not finite
 * and > 0; out_ptrs[t] == base_ptrs[t]; a segment of more than 2^31 - 1 elements), FEDAVG_ERR_STATE
 * (an open dynamic wave).
 */
int32_t fedavg_sparse_aggregate_delta(fedavg_ctx* ctx,
                                      const int32_t* const* index_ptrs /* [n][num_segments], device */,
                                      const void* const* value_ptrs /* [n][num_segments], device */,
                                      const int64_t* nnz /* [n][num_segments], host */,
                                      int32_t value_dtype, const double* weights /* [n], host */,
                                      int32_t num_clients, double divisor,
                                      const double* const* base_ptrs /* [num_segments], device fp64 */,
                                      void* const* out_ptrs /* [num_segments], device */,
                                      int32_t out_dtype, void* stream);

/*
 * Synchronise `stream` and report whether a sparse fold since the last report met an index
 * violation: *out = 1 if so, else 0. The word is cleared by the report, so the context stays usable.
 * FEDAVG_ERR_INVALID for a NULL context or out.
 */
int32_t fedavg_sparse_index_errors(fedavg_ctx* ctx, void* stream, int32_t* out);

/*
 * The broadcast encoder: the `send` half of the reference's StochasticQuantServerEndpoint /
 * NNADQServerEndpoint (simulation_lib/topology/quantized_endpoint.py:79-96), which quantises the
 * aggregated model before it goes out to every worker. num_tensors device tensors of one dtype are
 * turned into QSGD or NNADQ records (the layouts of FEDAVG_QSGD_F32 / FEDAVG_NNADQ_F32 above) where
 * they lie. The contract is DESIGN.md §5p, restated independently in tests/quant_encode_reference.py
 * on top of oracle/qsgd_oracle.py and oracle/nnadq_oracle.py.
 *
 * codec: FEDAVG_QSGD_F32 / QSGD_F64 / NNADQ_F32 / NNADQ_F64; the codec's dtype F (fp32 or fp64) is
 * the inputs' dtype. in_ptrs[num_tensors] (host array of device pointers): tensor t holds numels[t]
 * (host, >= 0) elements of F, aligned to the element only (NULL allowed where numels[t] == 0).
 * record_ptrs[num_tensors]: 16-byte aligned device buffers of fedavg_qsgd_record_bytes(numels[t]) /
 * fedavg_nnadq_record_bytes(numels[t]) bytes. EVERY byte of every record is written (header gaps,
 * the padding of the slot / code area and of the sign area as zeros): the buffers may be
 * uninitialised. A tensor does not depend on the layout of the context, only on its own device.
 *
 * Every line below is one separately rounded operation in F: no FMA, no reciprocal, IEEE division.
 *   QSGD:  norm = max|x|;  q = |x| / norm;  r = q * level;  fl = floor(r);  d = r - fl;
 *          slot = fl + (u < d ? 1 : 0), 0 everywhere when norm == 0, clamped to [0, level];
 *          sign bit = !(x < 0) (so -0.0 gives 1); header: norm widened to fp64, level.
 *   NNADQ: lo = min x;  hi = max x;  in fp64: r = (hi - lo) / (weight * max(|lo|, |hi|)),
 *          L = clamp(ceil(r), 1, 255), or 1 when r is not finite and positive;
 *          step = (hi - lo) / L in F;  code = clamp(rint((x - lo) / step), 0, L) (half to even),
 *          0 everywhere when step is not positive and finite; header: lo and step widened, L.
 * lo and hi are the extrema in the IEEE total order (-0.0 < +0.0), max|x| = max(-lo, hi) with a
 * zero norm stored as +0.0. An empty tensor gets norm 0 / lo 0, step 0, L 1.
 *
 * u is the uniform of element i of tensor t from Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57;
 * Weyl constants 0x9E3779B9, 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32) and counter
 * (block & 0xffffffff, block >> 32, id, draw), id = tensor_ids[t] (tensor_ids == NULL: id = t).
 *   fp32: block = i / 4, u = (out[i % 4] >> 8) * 2^-24
 *   fp64: block = i / 2, lo = out[2 * (i % 2)], hi = out[2 * (i % 2) + 1],
 *         u = ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53
 * NNADQ draws nothing: its records do not depend on seed, draw or the ids.
 *
 * Three launches whatever num_tensors is (a minimum / maximum pass over tiles of "quant_tile"
 * elements, a header pass, the encode pass over the same tiles), no atomics, no host round trip:
 * asynchronous on `stream`. The result depends on the inputs and the arguments alone. The
 * accumulator and its state are not touched; nothing outside the records is written. A call's tile
 * partials live in the context: calls on one context are ordered by their stream.
 * A non-finite input element latches FEDAVG_FLAG_INPUT_NAN (fedavg_check reports
 * FEDAVG_ERR_NAN_INPUT); the records of such a call are unspecified but stay inside their buffers.
 * Refused before any launch: FEDAVG_ERR_INVALID (a bad codec; a NULL table; num_tensors < 1 or >
 * 2^20; a negative count; a NULL or misaligned input or record; QSGD: level outside [1, 255]; NNADQ:
 * a weight that is not finite and > 0; more than 2^31 - 1 tiles), FEDAVG_ERR_STATE (an open dynamic
 * wave).
 */
int32_t fedavg_quant_encode(fedavg_ctx* ctx, int32_t codec, const void* const* in_ptrs /* [T], device */,
                            const int64_t* numels /* [T], host */,
                            const uint32_t* tensor_ids /* [T], host, or NULL: 0 .. T - 1 */,
                            int32_t num_tensors, void* const* record_ptrs /* [T], device */,
                            int32_t level, double weight, uint64_t seed, uint32_t draw, void* stream);

/*
 * The record decoder: the `get` half of the reference's QuantClientEndpoint
 * (simulation_lib/topology/quantized_endpoint.py:32-39), which dequantises the server's broadcast on
 * every worker, and the dequantisation of QuantServerEndpoint.get (:69-77) for consumers that take
 * dense tensors. num_tensors QSGD or NNADQ records of one codec (the layouts of FEDAVG_QSGD_F32 /
 * FEDAVG_NNADQ_F32 above) become dense tensors where they lie, in one launch. The contract is
 * DESIGN.md §5u; the expected values are oracle/qsgd_oracle.py:dequantize and
 * oracle/nnadq_oracle.py:dequantize.
 *
 * codec: FEDAVG_QSGD_F32 / QSGD_F64 / NNADQ_F32 / NNADQ_F64; the codec's dtype F (fp32 or fp64) is
 * the outputs' dtype. record_ptrs[num_tensors] (host array of device pointers): 16-byte aligned
 * records of numels[t] (host, >= 0) elements. out_ptrs[num_tensors]: numels[t] elements of F each,
 * aligned to the element only (a model's parameters are arbitrary views): 16-byte stores are used
 * where an address allows, single elements before and after, and the bits do not depend on which.
 * out64_ptrs (NULL, or [num_tensors]; FEDAVG_QSGD_F32 and FEDAVG_NNADQ_F32 only): fp64 buffers of
 * numels[t] elements, aligned to 8 bytes, that receive the exact widening of the same x in the same
 * pass (the copy a worker's model cache keeps). A record, an output and a wide output may be NULL
 * where numels[t] == 0. Outputs overlap neither each other nor the records.
 *
 * Every operation is separately rounded in F: no FMA, no reciprocal, IEEE division.
 *   QSGD:  norm = F(header norm);  level = F(header level);  sign = +1 where the element's bit is
 *          set, else -1;  a = norm * sign;  b = a * F(slot);  x = b / level
 *   NNADQ: lo = F(header lo);  step = F(header step);  t = F(code) * step;  x = t + lo
 * for every record byte pattern: slots above level, codes above levels and products that overflow
 * decode by the same lines.
 *
 * One launch whatever num_tensors is, over tiles of "quant_tile" elements: a lane reads one 16-byte
 * group of slots or codes and its 2 sign bytes, a workgroup its own record's header. No atomics, no
 * host round trip: asynchronous on `stream`. Exactly numels[t] elements of every output are written
 * and nothing else; the records are only read; the accumulator and its state are not touched.
 * FEDAVG_FLAG_INPUT_NAN is latched (fedavg_check reports FEDAVG_ERR_NAN_INPUT) by a header whose
 * level / levels lies outside [1, 255] and by a decoded element that is not finite; the outputs of
 * such a call are unspecified but stay inside their buffers.
 * Refused before any launch: FEDAVG_ERR_INVALID (a bad codec; a NULL table; num_tensors < 1 or >
 * 2^20; a negative count; a NULL or misaligned record; a NULL output or one not aligned to its
 * element; out64_ptrs with an _F64 codec; more than 2^31 - 1 tiles), FEDAVG_ERR_STATE (an open
 * dynamic wave).
 */
int32_t fedavg_quant_decode(fedavg_ctx* ctx, int32_t codec, const void* const* record_ptrs /* [T], device */,
                            const int64_t* numels /* [T], host */, int32_t num_tensors,
                            void* const* out_ptrs /* [T], device, dtype F */,
                            void* const* out64_ptrs /* [T] or NULL, device, fp64 */, void* stream);

/*
 * The clip-and-noise pass of the differential-privacy endpoints: the arithmetic of the reference's
 * add_dp_noise / add_dp_noise_to_parameter (simulation_lib/dp.py:13-47) on num_tensors device tensors
 * of one dtype (FEDAVG_F32 / F16 / BF16 / F64) where they lie. The contract is DESIGN.md §5r, restated
 * independently in tests/dp_reference.py.
 *
 * in_ptrs[num_tensors] (host array of device pointers): tensor t holds numels[t] (host, >= 0)
 * elements, aligned to the element only (NULL allowed where numels[t] == 0). out_ptrs[num_tensors]:
 * buffers of the same dtype and sizes; out_ptrs[t] == in_ptrs[t] is allowed (an element is read and
 * then written by the same lane), any other overlap is not. Nothing outside the outputs is written.
 *   row_len == 0: all tensors together are one vector with one norm (add_dp_noise_to_parameter).
 *   row_len > 0:  num_tensors == 1 and numels[0] % row_len == 0; every row of row_len elements has its
 *                 own norm (add_dp_noise on a 2-D+ tensor; a 1-D tensor is one row).
 * noise_scale is the fp64 product sigma * C, formed by the caller.
 *
 * Every line is one separately rounded fp64 operation after the exact widening of the element: no
 * FMA, no reciprocal, IEEE division, the correctly rounded square root.
 *   q = x * x;  acc = acc + q                                 (the sum of squares, from +0.0)
 *   norm = sqrt(acc);  t = norm / C;  s = (t < 1) ? 1 : t     (a NaN t stays NaN)
 *   y = x / s;  n = z * noise_scale;  o = y + n;  out = o rounded once, to nearest even, into the dtype
 * (so with noise_scale == 0 a zero comes back with the sign of y + z * 0: -0.0 only where x is -0.0
 * and z < 0).
 *
 * The order of the sum. G = "dp_ae_<d>", Tl = "dp_tile". A sum (whole-list mode: the one sum; row
 * mode: a row's) is cut into pieces of Tl elements: whole-list mode cuts every tensor from its first
 * element (a tensor's last piece is shorter, an empty tensor has none) and takes the pieces of all
 * tensors in list order; row mode cuts every row from its first element. A piece's partial: with
 * its elements in groups of G consecutive ones (group 0 starts at the piece's start), lane j of
 * "dp_threads" = 256 adds the squares of groups j, j + 256, ... in increasing element index, from
 * +0.0 (a lane without elements holds +0.0); the 256 lane sums combine by the adjacent-pair tree:
 * v[j] = v[2j] + v[2j + 1], eight times. The sum: lane j adds the partials j, j + 256, ... of its
 * pieces in increasing index from +0.0, and the same tree combines the lanes. The order depends on
 * numels, row_len and the dtype's G alone. All terms are >= 0: any order is within
 * (P + 2) * 2^-53 relative of the exact sum of P terms.
 *
 * z is element i's normal deviate of tensor t: the Philox4x32-10 block of fedavg_quant_encode's fp64
 * stream, key (seed & 0xffffffff, seed >> 32), counter (block & 0xffffffff, block >> 32, id, draw),
 * block = i / 2, id = tensor_ids[t] (tensor_ids == NULL: id = t); in row mode i counts through the
 * whole tensor. With the output words w0..w3:
 *   a = (w1 >> 5) * 2^26 + (w0 >> 6);  b = (w3 >> 5) * 2^26 + (w2 >> 6)          (53-bit integers)
 *   u1 = (a + 1) * 2^-53 in (0, 1];  u2 = b * 2^-53 in [0, 1)
 *   r = sqrt(-2 * LN(u1));  z[2 block] = r * COS(u2);  z[2 block + 1] = r * SIN(u2)
 * LN, COS and SIN are the sequences below: each line one rounded fp64 + - * /, no FMA, no library
 * function; integer steps where marked. Constants are hex floats.
 *   LN(u1), v = a + 1:
 *     d = (double)v (exact); E = d's unbiased exponent, F = d's 52 fraction bits     (integer)
 *     up = F >= 0x6a09e667f3bcd;  e = E - 53 + up;  m = the double with fraction F and unbiased
 *     exponent -up, in [sqrt(1/2), sqrt(2))                                          (integer)
 *     f = m - 1;  g = 2 + f;  s = f / g;  w = s * s
 *     p = L10;  then for k = 9 .. 1:  p = p * w;  p = p + Lk;    then  p = p * w;  p = p * s
 *     q = s + p;  lm = q + q;  el = (double)e * 0x1.62e42fefa39efp-1;  LN = el + lm
 *     L1..L10 = 1/3 .. 1/21 = 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3,
 *       0x1.c71c71c71c71cp-4, 0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4,
 *       0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5, 0x1.8618618618618p-5
 *     t = LN * -2;  r = sqrt(t)           (LN <= 0; u1 = 1 gives LN = +0.0, t = -0.0, r = -0.0)
 *   COS(u2), SIN(u2): k = b >> 50 (the octant), fi = b mod 2^50, gi = k odd ? 2^50 - fi : fi (integer)
 *     g = (double)gi * 2^-50 (exact);  x = g * 0x1.921fb54442d18p-1;  w = x * x
 *     p = S8;  then for k = 7 .. 1:  p = p * w;  p = p + Sk;    then  p = p * w;  p = p * x;  sn = x + p
 *     c = C8;  then for k = 7 .. 1:  c = c * w;  c = c + Ck;    then  c = c * w;  cs = 1 + c
 *     S1..S8 = -1/3!, 1/5!, .., 1/17! = -0x1.5555555555555p-3, 0x1.1111111111111p-7,
 *       -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19, -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33,
 *       -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49
 *     C1..C8 = -1/2!, 1/4!, .., 1/16! = -0x1p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10,
 *       0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37,
 *       0x1.ae7f3e733b81fp-45
 *     k = 1, 2, 5, 6: COS = sn, SIN = cs; else COS = cs, SIN = sn; then COS is negated (its sign bit
 *     flipped) for k = 2..5 and SIN for k = 4..7.
 *
 * Three launches whatever num_tensors is (the piece partials, one s per row or one in all, the apply
 * pass over tiles of Tl elements that start at even indices of their tensor, so no pair belongs to
 * two workgroups), no atomics, no host round trip: asynchronous on `stream`. The result depends on
 * the inputs and the arguments alone. The accumulator and its state are not touched. A call's
 * partials and s values live in the context: calls on one context are ordered by their stream.
 * A non-finite input element latches FEDAVG_FLAG_INPUT_NAN (fedavg_check reports
 * FEDAVG_ERR_NAN_INPUT); the outputs of such a call are unspecified but stay inside their buffers.
 * Refused before any launch: FEDAVG_ERR_INVALID (a bad dtype; a NULL table; num_tensors < 1 or >
 * 2^20; a negative count; a NULL input or output where numel > 0, or one not aligned to its element;
 * a C that is not finite and > 0; a noise_scale that is not finite and >= 0; a negative row_len, one
 * that does not divide the tensor, or row_len > 0 with num_tensors != 1; more than 2^31 - 1 tiles),
 * FEDAVG_ERR_STATE (an open dynamic wave).
 */
int32_t fedavg_dp_noise(fedavg_ctx* ctx, int32_t dtype, const void* const* in_ptrs /* [T], device */,
                        const int64_t* numels /* [T], host */,
                        const uint32_t* tensor_ids /* [T], host, or NULL: 0 .. T - 1 */, int32_t num_tensors,
                        void* const* out_ptrs /* [T], device */, int64_t row_len, double C, double noise_scale,
                        uint64_t seed, uint32_t draw, void* stream);

/*
 * The client-side top-k step with error feedback (the `_sparsify` of the reference's
 * worker/error_feedback_worker.py with top-k as the scheme) on num_tensors device tensors of one dtype
 * (FEDAVG_F32 / F16 / BF16 / F64) where they lie: what sparse.topk_sparsify computes per tensor. The
 * contract is DESIGN.md §5s; the oracle is the CPU path of sparse.topk_sparsify.
 *
 * Tensor t holds numels[t] (host, 0 .. 2^31 - 1) elements at delta_ptrs[t], aligned to the element
 * only, and sends keeps[t] (host, 0 .. numels[t]) of them. error_ptrs (NULL: no tensor has a residual
 * yet) holds per tensor its residual of the same size and dtype, or NULL.
 *   total[e] = delta[e] + error[e], the IEEE sum rounded once to nearest even into the dtype (for
 *              fp16 / bf16 the fp32 sum rounded to the dtype, which is the same value); without an
 *              error total[e] is delta[e] bit for bit.
 *   key[e]   = the bits of total[e] with the sign cleared, as an unsigned integer; every NaN has the
 *              one largest key. So +0.0 and -0.0 tie, inf beats every finite value, NaNs tie above inf.
 *   S        = the keeps[t] elements of largest (key, -index): among equal keys the lower index wins.
 *   index_ptrs[t][j] = the j-th element of S in increasing order (int32); value_ptrs[t][j] =
 *   total[index_ptrs[t][j]] bit for bit; residual_ptrs[t][e] = +0.0 for e in S, total[e] otherwise.
 * residual_ptrs[t] may be error_ptrs[t] or delta_ptrs[t] (every element is read and then written by
 * the same lane in the first pass); no other overlap is allowed. index_ptrs[t] and value_ptrs[t] hold
 * keeps[t] entries (NULL allowed where keeps[t] == 0, as the others are where numels[t] == 0).
 * Nothing outside the outputs is written.
 *
 * No sort: a radix select over the key's digits from the top (fp32 11 + 10 + 10 bits, fp16 / bf16
 * 8 + 7, fp64 11 + 11 + 11 + 10 + 10 + 10) finds per tensor the threshold key, then a count per tile
 * of "topk_tile" elements, a scan over each tensor's tiles and an order-preserving write. 2 launches
 * per digit and 3 more (fp32 9, fp16 / bf16 7, fp64 15) whatever num_tensors is, one grid over the
 * tiles of all tensors; no atomics on global memory, no floating-point reduction, no host round trip:
 * asynchronous on `stream`. The result depends on the inputs alone. The accumulator, its state and
 * the NaN flags are not touched. A call's histograms, select states and tile counts live in the
 * context (8 KiB per chunk of "topk_chunk" tiles): calls on one context are ordered by their stream.
 * Refused before any launch: FEDAVG_ERR_INVALID (a bad dtype; a NULL table other than error_ptrs;
 * num_tensors < 1 or > 2^20; a negative count; keeps[t] > numels[t]; numels[t] > 2^31 - 1; a NULL
 * delta or residual where numel > 0, a NULL index or value buffer where keep > 0, or a buffer not
 * aligned to its element; more than 2^31 - 1 tiles), FEDAVG_ERR_STATE (an open dynamic wave).
 */
int32_t fedavg_topk_sparsify(fedavg_ctx* ctx, int32_t dtype, const void* const* delta_ptrs /* [T], device */,
                             const void* const* error_ptrs /* [T], device, or NULL; entries may be NULL */,
                             const int64_t* numels /* [T], host */, const int64_t* keeps /* [T], host */,
                             int32_t num_tensors, int32_t* const* index_ptrs /* [T], device */,
                             void* const* value_ptrs /* [T], device */, void* const* residual_ptrs /* [T], device */,
                             void* stream);

/*
 * Synchronise `stream` and report the NaN flag: FEDAVG_OK, FEDAVG_ERR_NAN_INPUT (robust rules),
 * FEDAVG_ERR_NAN_ACCUM or FEDAVG_ERR_NAN_RESULT. *flags_out (optional) receives the raw flag bits.
 */
int32_t fedavg_check(fedavg_ctx* ctx, void* stream, uint32_t* flags_out);

/*
 * Diagnostic (error path only): for each client of the table, does any of its tensors hold
 * NaN? out_bad[num_clients] receives 0/1. Synchronous.
 */
int32_t fedavg_find_nan_clients(fedavg_ctx* ctx, const void* const* client_ptrs,
                                int32_t in_dtype, int32_t num_clients, int32_t* out_bad,
                                void* stream);

/* Kernel timing for bench.py: when enabled, every main-kernel launch is bracketed by a pair
 * of HIP events recorded on the launch stream. fedavg_prof_collect synchronises those
 * events, returns the summed kernel milliseconds and the launch count, and clears them. */
int32_t fedavg_prof_enable(fedavg_ctx* ctx, int32_t enable);
int32_t fedavg_prof_collect(fedavg_ctx* ctx, double* total_ms, int32_t* launches);

/* HBM ceiling probes (bench.py's measured copy / read roofline): mode 0 = 16-B copy of
 * `bytes` from src to dst, mode 1 = 16-B read-only stream of src (dst: >= 8 KiB scratch). */
int32_t fedavg_bw_probe(const void* src, int64_t bytes, void* dst, int32_t mode, void* stream);

/* =====================================================================================
 * PersonalizedFedAVG (simulation_lib/algorithm/personalized_aggregation_algorithm.py:9-57)
 *
 * Every receiver j keeps its own FedAvg over the other workers' updates, weighted by
 * worker_weights[j].get(i, 0) (:23-43); the centralized model is the equal-weight average of
 * the receivers' results in receiver order (:45-57 -> aggregation_algorithm.py:51-76).
 * One call replaces the whole round: N arrivals x M receivers, all client buckets resident.
 *
 *  client_ptrs[N][T]  arrival-ordered client tensors (NULL = the client did not send tensor t)
 *  client_ids[N]      worker id of each arrival
 *  weights[M][N]      receiver j's weight for arrival k (the .get(i, 0) value)
 *  receiver_ids[M]    worker id of each receiver (unique; receiver order = key order): receiver
 *                     j skips the arrivals whose id equals its own (:31-32)
 *  out_ptrs[M][T]     receiver results: acc_j / W_j (fed_avg_algorithm.py:71-99), fp32 or fp64
 *  central_ptrs[T]    optional: sum_j round(out_j * (1/M)) in receiver order, fp32 or fp64
 * Per receiver and segment the sum is the reference's arrival-order fp64 chain with separately
 * rounded products (fused to one fma only when the host proves every product exact), so every
 * output is bit-identical to the reference's float64 result (the fp32 outputs: its cast).
 * FEDAVG_ERR_STATE when a receiver folds no client for some segment (the :88 assertion). NaN
 * conditions (input NaN, inf*0, 0/0, inf-inf) latch flags reported by fedavg_pers_check.
 * ===================================================================================== */
typedef struct fedavg_pers fedavg_pers;
int32_t fedavg_pers_create(fedavg_pers** out, int32_t device, const int64_t* seg_numel, int32_t num_segments);
int32_t fedavg_pers_destroy(fedavg_pers* p);
/* fused fold when every product is provably exact (default on; results identical either way) */
int32_t fedavg_pers_set_fused_fold(fedavg_pers* p, int32_t enable);
int32_t fedavg_pers_aggregate(fedavg_pers* p, const void* const* client_ptrs, int32_t in_dtype,
                              int32_t num_clients, const int64_t* client_ids, const double* weights,
                              const int64_t* receiver_ids, int32_t num_receivers,
                              void* const* out_ptrs, int32_t out_dtype, void* const* central_ptrs,
                              int32_t central_dtype, void* stream);
/* Synchronise `stream`, report and clear the NaN flags (FEDAVG_FLAG_*): FEDAVG_OK,
 * FEDAVG_ERR_NAN_ACCUM (a receiver's accumulator: input NaN, inf*0, inf-inf) or
 * FEDAVG_ERR_NAN_RESULT (a receiver's result, e.g. 0/0, or the centralized average). */
int32_t fedavg_pers_check(fedavg_pers* p, void* stream, uint32_t* flags_out);
int32_t fedavg_pers_prof_enable(fedavg_pers* p, int32_t enable);
int32_t fedavg_pers_prof_collect(fedavg_pers* p, double* total_ms, int32_t* launches);
/* fp64 VALU ceiling probe (independent v_fma_f64 chains): measured TFLOP/s */
int32_t fedavg_fp64_probe(int64_t waves, int32_t iters, double* tflops_out, void* stream);

/* =====================================================================================
 * The routed row gather: the server half of the reference's graph embedding exchange
 * (GraphNodeEmbeddingPassingAlgorithm, simulation_lib/algorithm/graph_embedding_algorithm.py:38-59).
 * S workers send row blocks whose rows carry node ids; N workers each want a list of node ids and
 * get back, packed, the ids that somebody sent and those nodes' rows. A routed copy and nothing
 * else: no arithmetic touches a row, so every output byte is a source byte. The contract is
 * DESIGN.md §5o, restated independently in tests/graph_reference.py.
 *
 * A routing does not depend on a model layout, so it has a handle of its own. The handle owns the
 * dense int32 table node -> sent row (grown on demand, empty between calls), the call's workspace
 * and the error words; it serves one stream at a time (calls on several streams need the caller's
 * ordering).
 *
 * src_ptrs[num_sources] is a host array of device pointers to contiguous row blocks of
 * src_rows[num_sources] rows (host; 0 allowed, the pointer may then be NULL) of one common row_bytes;
 * elem_bytes (1, 2, 4 or 8) divides row_bytes and every row block is aligned to it. src_ids is a
 * device int64 array of R = sum(src_rows) node ids in source order: row r of the concatenation
 * carries node src_ids[r]; every id lies in [0, node_space) and no id appears twice. want_ids is a
 * device int64 array of B ids, the N = num_lists want lists concatenated; want_off[N + 1] (host)
 * cuts it, and every list is STRICTLY INCREASING. For list j let H_j be its ids that some source
 * sent, in the list's own order. Then
 *   out_count[j] = |H_j|                                  (device int32 [N])
 *   out_ids[want_off[j] + k] = the k-th id of H_j          (device int64 [B])
 *   out_rows row want_off[j] + k = that node's source row, unchanged   (device, B * row_bytes)
 * Every list packs into its own slot, which begins at want_off[j]: no count has to be known before
 * the outputs are allocated. Slots past the count are unspecified (this implementation leaves them
 * untouched) and nothing outside the three buffers is ever written. A wanted id that is negative,
 * >= node_space or sent by nobody is a miss; the table is never read out of range for it. With
 * num_sources = 0 every list misses everything. The result depends on the inputs alone: never on
 * the chunking ("route_chunk"), timing or earlier calls (no atomics; the table is put back to empty
 * by un-scattering the sent ids before the call's work on the stream ends, error or not).
 * Rows move by 16-byte loads and stores when row_bytes, out_rows and every source block are
 * multiples of 16, else element by element, with the same bytes out.
 * Asynchronous on `stream`.
 * Input errors found on the device latch bits that fedavg_route_errors reports: 1 = a node id was
 * sent twice (found by write-then-verify), 2 = a want list is not strictly increasing, 4 = a sent
 * id lies outside [0, node_space) (the row is then nobody's). The outputs of such a call are
 * unspecified but stay inside the buffers, and the handle stays usable.
 * Refused before any launch: FEDAVG_ERR_INVALID (a NULL handle or table; num_sources < 0 or > 1024;
 * num_lists < 1; a bad elem_bytes; row_bytes < 1 or not a multiple of elem_bytes; a pointer not
 * aligned to its element; a negative src_rows entry; R or B >= 2^31; node_space < 0 or > 2^28 (a
 * 1 GiB table); want_off not non-decreasing from 0).
 * ===================================================================================== */
typedef struct fedavg_route fedavg_route;
int32_t fedavg_route_create(fedavg_route** out, int32_t device);
int32_t fedavg_route_destroy(fedavg_route* route);
int32_t fedavg_route_rows(fedavg_route* route,
                          const void* const* src_ptrs /* [num_sources], host array of device pointers */,
                          const int64_t* src_rows /* [num_sources], host */, int32_t num_sources,
                          int64_t row_bytes, int32_t elem_bytes,
                          const int64_t* src_ids /* [R], device */,
                          const int64_t* want_ids /* [B], device */,
                          const int64_t* want_off /* [num_lists + 1], host */, int32_t num_lists,
                          int64_t node_space, void* out_rows /* device, B * row_bytes */,
                          int64_t* out_ids /* [B], device */, int32_t* out_count /* [num_lists], device */,
                          void* stream);
/*
 * Synchronise `stream`, report the error bits latched since the last report (see fedavg_route_rows)
 * into *out and clear them. FEDAVG_ERR_INVALID for a NULL handle or out.
 */
int32_t fedavg_route_errors(fedavg_route* route, void* stream, int32_t* out);

/* =====================================================================================
 * Host ingest (aggregation_server.py:129: updates arrive as CPU tensors). Copy one client's
 * n tensors (pageable host memory, srcs[i], nbytes[i]) into a pinned staging bucket at byte
 * offsets dst_off[i], with a persistent pool of host threads (FEDAVG_PACK_THREADS, default
 * min(OMP_NUM_THREADS or cores, 8)); the caller then moves the bucket with one DMA.
 * Synchronous. A NULL source or 0 bytes is skipped.
 * ===================================================================================== */
int32_t fedavg_host_pack(void* dst, const void* const* srcs, const int64_t* nbytes, const int64_t* dst_off,
                         int32_t n);
int32_t fedavg_host_pack_threads(void);

/* =====================================================================================
 * Multi-GPU exchange step (replaces nothing in the reference, which
 * sends every update to one server process: aggregation_server.py:111-145). One process per
 * GPU; the library owns an RCCL communicator (bound at run time from the process's RCCL,
 * librccl.so.1 — torch's when torch is loaded; FEDAVG_RCCL_LIB overrides).
 *   rank 0: fedavg_comm_unique_id(id); the caller ships the FEDAVG_COMM_ID_BYTES to every rank
 *   every rank: fedavg_comm_create(&comm, id, world, rank, device)   (collective)
 *   every round: fedavg_sharded_round(comm, ctx, partial_plan, finalize_plan_or_NULL, chunks,
 *                root, stream)
 * A round launches the partial plan in `chunks` tile ranges on `stream`; after each range its
 * fp64 partial is summed into the root's accumulator by ncclReduce on the communicator's
 * high-priority stream (overlapping the next range's kernel); `stream` then waits for the last
 * reduce and the root runs the finalize plan over every tile. Asynchronous; check with
 * fedavg_check on the root. Results: each rank's fold is exact, the cross-rank fp64 sum is
 * RCCL's order. With profiling enabled on ctx, only the first chunk's launch of
 * a round is timed (fedavg_prof_collect).
 * ===================================================================================== */
#define FEDAVG_COMM_ID_BYTES 128
typedef struct fedavg_comm fedavg_comm;
int32_t fedavg_comm_unique_id(void* id_out);
int32_t fedavg_comm_create(fedavg_comm** out, const void* id, int32_t world, int32_t rank, int32_t device);
int32_t fedavg_comm_destroy(fedavg_comm* comm);
int32_t fedavg_sharded_round(fedavg_comm* comm, fedavg_ctx* ctx, fedavg_plan* partial, fedavg_plan* finalize,
                             int32_t chunks, int32_t root, void* stream);
/*
 * The same round with a scatter exchange instead of a reduce to the root (DESIGN.md §5 cost
 * table). Every rank passes a finalize plan (non-root ranks: scratch outputs of the same
 * layout). Per chunk [A, B) of the accumulator (B - A = G*L + R):
 *   ncclReduceScatter of acc[A, A + G*L) (rank r receives the sums of window
 *   [A + r*L, A + (r+1)*L)) — plus, when R > 0, an ncclReduce of the R-element tail to the root,
 *   in one group — on the comm stream behind the chunk's partial kernel; each rank divides its
 *   window (fedavg_plan_finalize_window) and ncclGather collects the windows, in the output dtype,
 *   into the root's result buffer (accumulator coordinates). `stream` then waits for the last
 *   gather and the root copies the result into its outputs (fedavg_plan_copy_out). A NaN on any
 *   rank's window surfaces in the root's fedavg_check (as FEDAVG_ERR_NAN_RESULT).
 * Root ingress: (G-1)/G of the fp64 partial + (G-1)/G of the result, against the whole fp64
 * partial for fedavg_sharded_round; every rank egresses the same (G-1)/G of its partial.
 */
int32_t fedavg_sharded_round_scatter(fedavg_comm* comm, fedavg_ctx* ctx, fedavg_plan* partial,
                                     fedavg_plan* finalize, int32_t chunks, int32_t root, void* stream);
/*
 * Either round with caller-chosen chunks: tile_edges[0..num_edges) runs from 0 to
 * fedavg_num_tiles(ctx), strictly increasing; chunk k is tiles [tile_edges[k], tile_edges[k+1]).
 * Uneven chunks shift the exposed part of the exchange: a short last chunk shortens the tail when
 * the exchange keeps up with the fold, a short first chunk starts the exchange sooner when it
 * does not (sharded.tune_exchange times the shapes on the node). exchange: FEDAVG_EXCHANGE_*.
 * fedavg_sharded_round(..., chunks, ...) is this call with `chunks` equal ranges.
 */
#define FEDAVG_EXCHANGE_REDUCE 0
#define FEDAVG_EXCHANGE_SCATTER 1
int32_t fedavg_sharded_round_edges(fedavg_comm* comm, fedavg_ctx* ctx, fedavg_plan* partial, fedavg_plan* finalize,
                                   const int32_t* tile_edges, int32_t num_edges, int32_t exchange, int32_t root,
                                   void* stream);

/* =====================================================================================
 * Dynamic waves — the round's first wave folded while its clients still arrive.
 * Replaces, for the plugin's round (FedAVGAlgorithm.process_worker_data x N then
 * aggregate_worker_data, simulation_lib/algorithm/fed_avg_algorithm.py:20-113, driven by
 * simulation_lib/server/aggregation_server.py:111-145), the wave that could only start once every
 * arrival was staged: the kernel is launched at the first arrival with an open client count.
 *
 *   fedavg_dyn_open(ctx, in_dtype, max_clients, stream)
 *       launch the wave (zero-initialised: the accumulator must hold nothing yet) on a private
 *       stream, behind what `stream` holds so far. While it is open every other launch on the
 *       context fails with FEDAVG_ERR_STATE.
 *   fedavg_dyn_publish(ctx, client_ptrs[K][T], weights[K][T], K, stream, &published)
 *       hand rows [already published, K) of the caller's client table to the wave (rows keep
 *       their indices: the same table the caller appends to). Rows must carry every tensor, 16-B
 *       aligned, one weight per row (else FEDAVG_ERR_INVALID: close the wave and fold the rest
 *       the ordinary way). Nothing is published (published = 0) while `stream` has unfinished
 *       work — the tensors of those rows may not be written yet.
 *   fedavg_dyn_close(ctx, out_ptrs or NULL, out_dtype, join, stream, &folded, &finalized)
 *       fix the count. With out_ptrs (16-B aligned) the wave divides by the published rows'
 *       totals (arrival order) into the outputs: finalized = 1, the round is done (check with
 *       fedavg_check on `stream`). Otherwise — NULL outputs, or the wave ended itself after
 *       FEDAVG_DYN_IDLE_US (200) µs without a new row or FEDAVG_DYN_LIFE_US (2 s) in all — it
 *       stores the fp64 accumulator of rows [0, folded) (the context's state says so) and the
 *       caller folds rows [folded, K) with the ordinary calls; `stream` then continues after the
 *       wave. A finalized wave with join = 1 likewise orders `stream` after it; with join = 0
 *       it does not — the outputs are complete once the next fedavg_check on this context
 *       returns (it waits for the wave), which spares `stream` the cross-stream wait (a stream
 *       that waited on another's event can still read as busy right after its synchronize).
 *       folded counts the caller's rows from 0 (every wave of the round, see below).
 *   A wave that ended itself stays open for the caller: the next publication that hands over
 *       rows launches a fresh wave continuing from the fp64 accumulator (its rows [0, folded) are
 *       there) — the reference server's poll loop hands updates over in bursts with a sleep in
 *       between (simulation_lib/server/server.py:133-146), and each burst after the idle limit is
 *       folded while it arrives. Rows published to the ended wave after it stopped reading are
 *       handed to the new one. The close divides by the totals of every published row.
 *   fedavg_dyn_state(ctx, &active, &published)
 *   fedavg_dyn_info(ctx, info, n): the first n of {active, published, rows in the accumulator from
 *       waves that ended themselves this round, continued waves (cumulative), wave launches
 *       (cumulative)}.
 * Per element the fold is the reference's arrival-order chain (separately rounded product and
 * sum): the bits equal fedavg_aggregate's.
 * ===================================================================================== */
int32_t fedavg_dyn_open(fedavg_ctx* ctx, int32_t in_dtype, int32_t max_clients, void* stream);
int32_t fedavg_dyn_publish(fedavg_ctx* ctx, const void* const* client_ptrs, const double* weights, int32_t num_clients,
                           void* stream, int32_t* published_out);
int32_t fedavg_dyn_close(fedavg_ctx* ctx, void* const* out_ptrs, int32_t out_dtype, int32_t join, void* stream,
                         int32_t* folded_out, int32_t* finalized_out);
int32_t fedavg_dyn_state(const fedavg_ctx* ctx, int32_t* active, int32_t* published);
int32_t fedavg_dyn_info(const fedavg_ctx* ctx, int32_t* info, int32_t n);
/* GPU-clock timing of the context's last wave when it ran with fedavg_prof_enable on (each tile
 * workgroup then stores its finishing time; this call waits for the wave and reads them): the first
 * n of {µs from the mirror handing the tiles their last rows to the wave's last workgroup finishing
 * (the fold after the last publication, result stores included), µs from the mirror seeing the
 * close to that end, µs from the last rows to the close} — -1 where not recorded. */
int32_t fedavg_dyn_timing(const fedavg_ctx* ctx, double* out, int32_t n);
/* The wave's idle limit and lifetime in microseconds for the following launches (0 keeps the
 * current value; the defaults come from FEDAVG_DYN_IDLE_US / FEDAVG_DYN_LIFE_US, 200 us / 2 s). */
int32_t fedavg_dyn_configure(fedavg_ctx* ctx, int64_t idle_us, int64_t life_us);
/* With fedavg_prof_enable on: the summed time of the closed waves' body launches (enqueue at
 * the open to the launch's end, so the arrival phase is included) and their count; clears them. */
int32_t fedavg_dyn_prof_collect(fedavg_ctx* ctx, double* total_ms, int32_t* waves);

/* =====================================================================================
 * Single-process multi-device mode ("a communicator created by the library
 * from a device list"). The reference drives aggregation from ONE server process
 * (simulation_lib/server/server.py:122-152 -> aggregation_server.py:111-145 ->
 * FedAVGAlgorithm.process_worker_data / aggregate_worker_data, fed_avg_algorithm.py:20-113);
 * this object lets that one process shard the sum of fed_avg_algorithm.py:43-64 over G MI355X.
 *
 *   fedavg_multi_create(&m, devices, G, seg_numel, T, accumulators_or_NULL)
 *       one context per device entry (fedavg_multi_context: fold that device's shard with the
 *       single-device calls above), one library stream and one high-priority exchange stream per
 *       entry, peer access enabled between distinct devices (fedavg_multi_peer_access). Entries
 *       may repeat a device (aliased devices: tests on one GPU).
 *   fedavg_multi_round(m, partials[G], totals, outs, out_dtype, root, edges, n_edges, exchange,
 *                      streams)
 *       one round of device-resident clients: partials[g] is a zero-initialised partial plan on
 *       context g (NULL = device g holds no client). Exchanges:
 *        FEDAVG_EXCHANGE_PEER  — chunk k (tiles [edges[k], edges[k+1])) is cut into G windows,
 *          device j owns window j. Device g's partial kernel for window j != g stores its fp64
 *          partial straight into device j's receive slot over xGMI; device j then folds its own
 *          window and, in the same kernel, sums the G partials of it in device order
 *          S_0 + S_1 + ... (its own from registers; deterministic), divides by totals[t] and
 *          stores the result into the root's outputs (a peer store). Cross-device order is
 *          carried by events (no spinning kernel). Needs peer access (or aliased devices).
 *        FEDAVG_EXCHANGE_REDUCE — each chunk's partials are reduced to the root's accumulator by
 *          an in-process RCCL communicator (ncclCommInitAll, created on first use; RCCL's
 *          summation order), then the root divides.
 *       streams[g]: the caller's stream of entry g (NULL = the library's); each entry's work is
 *       ordered after what the caller enqueued there before, and streams[root] is ordered after
 *       the whole round.
 *   fedavg_multi_combine(m, totals, outs, out_dtype, root, exchange, streams)
 *       the streaming form: every context's accumulator already holds its shard's fp64 partial
 *       (folded in waves with fedavg_accumulate on context g); segments a context never folded
 *       count as the identity. FEDAVG_ERR_STATE if no context folded some segment (the :88
 *       assertion). Resets every context's accumulated state (fed_avg_algorithm.py:90,98).
 *   fedavg_multi_check(m, flags_out): synchronise every stream of the object and report the OR
 *       of every context's NaN flags like fedavg_check; fedavg_multi_reset clears them.
 *   fedavg_multi_round_check(m, flags_out): the same report after waiting for the end of the
 *       last round / combine only (one event, behind every entry's exchange work) — the per-round
 *       form of the reference's assertions (fed_avg_algorithm.py:35,93,97) for a server that
 *       enqueued nothing else on the object's streams since; fedavg_multi_check before any round.
 * Results: each device's fold is the exact arrival-order chain of its clients; PEER sums the
 * partials in device order (bit-identical to that host composition), REDUCE in RCCL's order.
 * Every call returns with the caller's current device (hipGetDevice) unchanged. Destroy the
 * plans made on the entries' contexts before (or after) fedavg_multi_destroy: a plan keeps its
 * device, not its context, for its own destroy, but must not be run once the object is gone.
 * ===================================================================================== */
#define FEDAVG_EXCHANGE_PEER 2
#define FEDAVG_MULTI_MAX_DEVICES 16
typedef struct fedavg_multi fedavg_multi;
int32_t fedavg_multi_create(fedavg_multi** out, const int32_t* devices, int32_t num_devices, const int64_t* seg_numel,
                            int32_t num_segments, void* const* accumulators);
int32_t fedavg_multi_destroy(fedavg_multi* m);
int32_t fedavg_multi_num_devices(const fedavg_multi* m);
int32_t fedavg_multi_device(const fedavg_multi* m, int32_t index);
fedavg_ctx* fedavg_multi_context(fedavg_multi* m, int32_t index);
void* fedavg_multi_stream(fedavg_multi* m, int32_t index);
/* 1 when every pair of distinct devices of the object has peer access enabled, else 0 */
int32_t fedavg_multi_peer_access(const fedavg_multi* m);
int32_t fedavg_multi_round(fedavg_multi* m, fedavg_plan* const* partials, const double* total_weights,
                           void* const* out_ptrs, int32_t out_dtype, int32_t root, const int32_t* tile_edges,
                           int32_t num_edges, int32_t exchange, void* const* streams);
int32_t fedavg_multi_combine(fedavg_multi* m, const double* total_weights, void* const* out_ptrs, int32_t out_dtype,
                             int32_t root, int32_t exchange, void* const* streams);
int32_t fedavg_multi_check(fedavg_multi* m, uint32_t* flags_out);
int32_t fedavg_multi_round_check(fedavg_multi* m, uint32_t* flags_out);
int32_t fedavg_multi_reset(fedavg_multi* m);
/* Measurement of fedavg_multi_round (bench.py's N > 1 line): while enabled, every round records
 * three timing events on entry 0's stream (device 0) — the round's start, the end of entry 0's
 * last chunk fold (its client reads; the peer stores of its other windows), and the round's end
 * behind every entry's exchange work. fedavg_multi_prof_collect waits for them and returns the
 * summed fold and tail (fold end -> round end: the exposed exchange + division that the
 * reference's single server process, simulation_lib/server/server.py:122-152, waits for after the
 * last fold) times in ms over the recorded rounds, then clears them. The markers sit between the
 * round's launches, so time profiled rounds apart from the timed ones. */
int32_t fedavg_multi_prof_enable(fedavg_multi* m, int32_t on);
int32_t fedavg_multi_prof_collect(fedavg_multi* m, double* fold_ms, double* tail_ms, int32_t* rounds);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_HIP_H */
