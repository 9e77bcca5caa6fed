/*
 * gf_hip.h -- C ABI of libgf_hip.so: MI355X (gfx950) kernels for GraphFlow's second-order CCN/SMP hot path.
 *
 * Boundary contract.  Plain pointers and sizes only; no C++/torch types.  Every entry point
 * returns a gf_status (never aborts, unlike the reference's assert()s) and records a message retrievable with
 * gf_last_error().  Each declaration cites the reference interface it replaces (paths relative to the
 * HyTruongSon/GraphFlow tree).
 *
 * Two calling modes share the same kernels:
 *   mode B "device"  *_f32   : device pointers, a batch of independent graphs, asynchronous on the context's
 *                              HIP stream.  This is the measured path.
 *   mode A "host"    *_host_*: host pointers in the reference's own container layout (N separate Tensor3D
 *                              buffers, double or float); the call stages H2D, runs the same kernels, stages D2H
 *                              and synchronises -- what an Entity-style op's forward()/backward() calls, exactly
 *                              as GraphFlow_gpu/RisiContraction_18_gpu.h:1509-1562 does around its CUDA kernel.
 *
 * Layouts (row-major, channel fastest):
 *   P   [batch][N][N][N][C]   P[g][a][b][c][f]  == tensors[a]->value[(b*N+c)*C+f]     (RisiContraction_18.h:48-53)
 *   A   [batch][N][N]         adj->value[d*N+e]                                        (Matrix.h:34-36)
 *   Out [batch][N][N][K][C]   value[(x*N+y)*K*C + k*C + f]                             (RisiContraction_18.h:29,103)
 *   G   same shape as Out (the op's own `gradient`), dP same shape as P (the inputs' `gradient`).
 */
#ifndef GF_HIP_H_INCLUDED
#define GF_HIP_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gf_ctx gf_ctx;

typedef enum {
    GF_OK = 0,
    GF_ERR_INVALID = 1,     /* bad argument (null pointer, non-positive size, unknown K) */
    GF_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed */
    GF_ERR_NOMEM = 3,       /* workspace allocation failed */
    GF_ERR_UNSUPPORTED = 4, /* shape outside what the kernels implement */
    GF_ERR_TIMEOUT = 5      /* a data-parallel rank waited longer than GF_DIST_TIMEOUT_S for its peers (gf_dist_*) */
} gf_status;

/* ---- context: device + stream + workspace ---------------------------------------------------------------------
 * Replaces the per-op-object cudaMalloc'd buffers and optional cudaStream_t of RisiContraction_18_gpu
 * (GraphFlow_gpu/RisiContraction_18_gpu.h:853-874, 947-955).  One context per host thread / per GPU; not thread-safe,
 * matching the reference's "one model clone per worker thread" rule (SMP_omega.h:115-129).
 * `stream` is a hipStream_t; NULL is the device's default (null) stream, which is where the reference's GPU ops run
 * until set_gpu_stream is called.  gf_ctx_use_private_stream gives the context its own non-blocking stream, the
 * analogue of the per-worker cudaStream_t of SMP_omega_gpu_multistreams.h:130-135.                                 */
gf_status gf_ctx_create(gf_ctx **out, int device, void *stream);
gf_status gf_ctx_use_private_stream(gf_ctx *ctx);
gf_status gf_ctx_destroy(gf_ctx *ctx);
gf_status gf_ctx_set_stream(gf_ctx *ctx, void *stream);     /* RisiContraction_18_gpu::set_gpu_stream (:947) */
void     *gf_ctx_get_stream(gf_ctx *ctx);
gf_status gf_ctx_synchronize(gf_ctx *ctx);                  /* cudaStreamSynchronize in SMP_omega_gpu_multistreams.h:765-771 */
gf_status gf_ctx_reserve(gf_ctx *ctx, size_t workspace_bytes); /* pre-size the scratch so timed regions never allocate */
/* Tracing: per-kernel HIP-event timing on the context's stream (the reference only has wall-clock gettimeofday in its
 * tests, tests/test_RisiContraction_18_gpu.cu:31-40).  Enabling resets the table; reading synchronises the stream. */
gf_status gf_ctx_set_timing(gf_ctx *ctx, int enable);
/* Restrict the timing to launches of ONE kernel name (NULL or "" = all).  The two events around a launch cost about as
 * much as a small kernel and keep neighbouring kernels from overlapping their ramp-up/tail: timing every launch slowed a
 * 72-launch SMP step by 5 %; timing only the kernel under study does not. */
gf_status gf_ctx_set_timing_filter(gf_ctx *ctx, const char *kernel_name);
int       gf_ctx_timing_count(gf_ctx *ctx);
gf_status gf_ctx_timing_get(gf_ctx *ctx, int index, const char **name, double *total_ms, long long *launches);
/* Measurement aid ("a measured device-to-device copy ceiling from the box"): `iters` copies of n floats src -> dst by a
 * hand-written kernel on the context's stream, bracketed by HIP events; *ms_per_copy = their average.  mode 0: float4 loads / stores,
 * grid-stride, one workgroup slot per CU x 8; mode 1: the same with non-temporal loads and stores.  n % 4 == 0.  No reference
 * counterpart (its tests time with gettimeofday, tests/test_RisiContraction_18_gpu.cu:31-40).                                       */
gf_status gf_hbm_copy_probe_f32(gf_ctx *ctx, float *dst, const float *src, size_t n, int mode, int iters, double *ms_per_copy);
const char *gf_last_error(gf_ctx *ctx);                     /* a per-thread copy: valid until this thread's next gf_last_error; ctx may be NULL for create errors */
const char *gf_version(void);
/* Per-context options.  GF_OPT_R18_GENERIC_KERNELS != 0 routes RisiContraction_18 through the layout-agnostic generic
 * kernels (any N, any C, one thread per table / output element) instead of the slab kernels: the independent second
 * implementation the parity tests hold the fast path against.  (The reference's GPU op has a comparable switch -- its CPU
 * fallback under a complexity threshold, RisiContraction_18_gpu.h:961-968 -- but both routes here run on the device.) */
typedef enum {
    GF_OPT_R18_GENERIC_KERNELS = 1,
    /* != 0: the block products of the fused SMP level at 64 channels run on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32) instead of
     * the f16 pipe with two-half fp32 operands (the default; component-wise fp32-grade inside a 2^17 window per 64-column block,
     * DESIGN.md section 5).  The environment variable GF_SMP_SPLIT=0 selects the same for every context of the process. */
    GF_OPT_SMP_FP32_PRODUCTS = 2
} gf_option;
gf_status gf_ctx_set_option(gf_ctx *ctx, int option, int value);

/* ---- data parallelism: one RCCL communicator per context ----------------------------------------------------------------
 * Replaces the master/worker exchange of SMP_omega::Threaded_BatchLearn (GraphFlow/SMP_omega.h:750-792): copy_value of the
 * master's parameters into every worker clone (:710-728, :771-773) = gf_dist_broadcast_f32; the serial add_gradient loop over
 * the clones (:730-740, :784-786) = gf_dist_allreduce_sum_f32.  A worker is one GPU: one context per GPU, in one process per
 * GPU (torchrun / mpirun style) or one host thread per GPU (the reference's std::thread style).
 * Rank 0 calls gf_dist_unique_id and hands the GF_DIST_ID_BYTES bytes to the other ranks by any host channel (a file, a
 * socket, MPI, torch.distributed, shared memory between threads); then EVERY rank calls gf_dist_init with the same id.
 * Collectives are in place, asynchronous and ordered on the context's stream.  RCCL is loaded on the first gf_dist_* call;
 * when it is missing the call fails with GF_ERR_UNSUPPORTED (nothing else in the library needs it).
 * Once a context has a communicator, gf_smp_backward on it returns the gradient SUMMED OVER ALL RANKS: each level's weight
 * gradients are all-reduced on the communicator's own stream as soon as the reverse sweep has produced them, while the sweep
 * continues below (gf_smp_set_grad_allreduce(smp, 0) turns that off for a handle).                                          */
#define GF_DIST_ID_BYTES 128
gf_status gf_dist_unique_id(gf_ctx *ctx, void *id_out /* GF_DIST_ID_BYTES */);
gf_status gf_dist_init(gf_ctx *ctx, const void *id /* GF_DIST_ID_BYTES */, int rank, int world);
gf_status gf_dist_finalize(gf_ctx *ctx);                   /* also done by gf_ctx_destroy */
int       gf_dist_rank(const gf_ctx *ctx);                 /* 0 when the context has no communicator */
int       gf_dist_world(const gf_ctx *ctx);                /* 1 when the context has no communicator */
gf_status gf_dist_allreduce_sum_f32(gf_ctx *ctx, float *buf, size_t n);
gf_status gf_dist_broadcast_f32(gf_ctx *ctx, float *buf, size_t n, int root);
/* Watchdog.  gf_dist_init, the join at the end of gf_smp_backward's overlapped all-reduces, and this call wait for the peers at most
 * GF_DIST_TIMEOUT_S seconds (environment, default 180, 0 = for ever) and then fail with GF_ERR_TIMEOUT; gf_last_error names the
 * rank, the world size, the device and the last collective handed to RCCL.  gf_dist_quiesce waits (by polling, under that limit)
 * until everything issued so far on the communicator's stream and on the context's stream has completed: call it before a
 * blocking hipStreamSynchronize / hipDeviceSynchronize that would otherwise hang on a peer that never joined.  No-op without a
 * communicator. */
gf_status gf_dist_quiesce(gf_ctx *ctx);

/* ---- tensor contractions, mode B (device pointers, batched) -----------------------------------------------------
 * K selects the family: 4, 10, 18 or 50.
 *   K=18: RisiContraction_18::forward/backward (GraphFlow/RisiContraction_18.h:73-331, 333-560), A gated by A>0 (:90,:345)
 *   K=10: RisiContraction_10 (RisiContraction_10.h:73-153, 155-225), no gate
 *   K=50: RisiContraction_50 (RisiContraction_50.h:73-441, 443-802), no gate
 *   K=4 : RisiContraction_4  (RisiContraction_4.h:68-125, 127-173), A ignored (may be NULL)
 * forward : Out is overwritten (the reference zeroes value first).
 * backward: accumulate != 0 -> dP += vjp (the reference's `+=` contract); accumulate == 0 -> dP = vjp (write-only
 *           fast path, legal when dP has a single consumer, as in the SMP DAG).  A receives no gradient.             */
gf_status gf_contract_forward_f32(gf_ctx *ctx, int K, const float *P, const float *A, float *Out,
                                  int N, int C, int batch);
gf_status gf_contract_backward_f32(gf_ctx *ctx, int K, const float *G, const float *A, float *dP,
                                   int N, int C, int batch, int accumulate);
/* Scratch bytes the two calls above need for (K,N,C,batch); gf_ctx_reserve(max over your shapes) up front. */
size_t gf_contract_workspace_bytes(int K, int N, int C, int batch);

/* ---- tensor contractions, mode A (host pointers, one graph, reference container layout) --------------------------
 * tensors[a] points at the a-th neighbour's Tensor3D::value ([N][N][C]); grads[a] at its ::gradient (always `+=`).
 * Blocking: returns after the result is in host memory.                                                              */
gf_status gf_contract_forward_host_f64(gf_ctx *ctx, int K, const double *const *tensors, const double *A,
                                       double *out_value, int N, int C);
gf_status gf_contract_backward_host_f64(gf_ctx *ctx, int K, const double *out_gradient, const double *A,
                                        double *const *grads, int N, int C);
gf_status gf_contract_forward_host_f32(gf_ctx *ctx, int K, const float *const *tensors, const float *A,
                                       float *out_value, int N, int C);
gf_status gf_contract_backward_host_f32(gf_ctx *ctx, int K, const float *out_gradient, const float *A,
                                        float *const *grads, int N, int C);

/* ---- RisiContraction_18_dropout (GraphFlow/RisiContraction_18_dropout.h:106-477 / :479-783) ----------------------------
 * keep_mask bit k = use[k]: a dropped slice is 0 in forward and ignored in backward.  Train mode: scale = 1 and the mask
 * the host drew (:113-125); test mode: keep_mask = all 18 bits, scale = nKept/18 (:465-471).  The host side
 * (graphflow_amd/host/RisiContraction_hip.h) draws the mask with rand() exactly as the reference does.                  */
gf_status gf_contract18_dropout_forward_f32(gf_ctx *ctx, unsigned keep_mask, float scale, const float *P, const float *A,
                                            float *Out, int N, int C, int batch);
gf_status gf_contract18_dropout_backward_f32(gf_ctx *ctx, unsigned keep_mask, const float *G, const float *A, float *dP,
                                             int N, int C, int batch, int accumulate);
gf_status gf_contract18_dropout_forward_host_f64(gf_ctx *ctx, unsigned keep_mask, double scale, const double *const *tensors,
                                                 const double *A, double *out_value, int N, int C);
gf_status gf_contract18_dropout_backward_host_f64(gf_ctx *ctx, unsigned keep_mask, const double *out_gradient, const double *A,
                                                  double *const *grads, int N, int C);
gf_status gf_contract18_dropout_forward_host_f32(gf_ctx *ctx, unsigned keep_mask, double scale, const float *const *tensors,
                                                 const float *A, float *out_value, int N, int C);
gf_status gf_contract18_dropout_backward_host_f32(gf_ctx *ctx, unsigned keep_mask, const float *out_gradient, const float *A,
                                                  float *const *grads, int N, int C);

/* ---- dense feature mixers, mode B (device pointers) ------------------------------------------------------------------
 * All row-major.  One strided-batched fp32 MFMA GEMM underneath (v_mfma_f32_32x32x2_f32, exact fp32).
 * backward: a NULL gradient pointer skips that operand; accumulate != 0 -> `+=` (the reference contract), else `=`.
 *   MatMul        C[M,N] = A[M,K] B[K,N]                       GraphFlow/MatMul.h:48-67 / :69-82
 *                 (GPU prior art: GraphFlow_gpu/MatMul_gpu.h:28-111)
 *   MatTensorMul  Out[R,J,D] = sum_k X[R,Kd] F[Kd,J,D]         GraphFlow/MatTensorMul.h:47-68 / :70-85
 *   TensorMatMul  Out[R,J,D] = sum_k F[R,Kd,D] Y[Kd,J]         GraphFlow/TensorMatMul.h:46-67 / :69-84                  */
gf_status gf_matmul_forward_f32(gf_ctx *ctx, const float *A, const float *B, float *C, int M, int K, int N);
gf_status gf_matmul_backward_f32(gf_ctx *ctx, const float *dC, const float *A, const float *B, float *dA, float *dB,
                                 int M, int K, int N, int accumulate);
gf_status gf_mattensormul_forward_f32(gf_ctx *ctx, const float *X, const float *F, float *Out, int R, int Kd, int J, int D);
gf_status gf_mattensormul_backward_f32(gf_ctx *ctx, const float *G, const float *X, const float *F, float *dX, float *dF,
                                       int R, int Kd, int J, int D, int accumulate);
gf_status gf_tensormatmul_forward_f32(gf_ctx *ctx, const float *F, const float *Y, float *Out, int R, int Kd, int J, int D);
gf_status gf_tensormatmul_backward_f32(gf_ctx *ctx, const float *G, const float *F, const float *Y, float *dF, float *dY,
                                       int R, int Kd, int J, int D, int accumulate);
/* CustomMatMulTensor (GraphFlow/CustomMatMulTensor.h:47-68 / :70-85), the channel mix of the SMP_2D_ver6-8 drivers:
 *   Out[rows,Kout] = T[rows,V] W^T,  W = [Kout,V] row-major, rows = nRows*nColumns positions of the Tensor3D.
 *   backward: dW (+)= G^T T,  dT (+)= G W.                                                                           */
gf_status gf_custommatmultensor_forward_f32(gf_ctx *ctx, const float *W, const float *T, float *Out, long long rows, int V,
                                            int Kout);
gf_status gf_custommatmultensor_backward_f32(gf_ctx *ctx, const float *G, const float *W, const float *T, float *dW,
                                             float *dT, long long rows, int V, int Kout, int accumulate);
/* StackTensor3D (GraphFlow/StackTensor3D.h:54-73 / :75-90): `tensors` / `grads` are DEVICE arrays of nRows device
 * pointers, each to per_tensor floats; forward copies them into one contiguous buffer, backward scatter-adds back. */
gf_status gf_stack_forward_f32(gf_ctx *ctx, const float *const *tensors, float *out, int nRows, size_t per_tensor);
gf_status gf_stack_backward_f32(gf_ctx *ctx, const float *G, float *const *grads, int nRows, size_t per_tensor);

/* ---- dense feature mixers, mode A (host pointers; gradients are always `+=`; NULL gradient pointers are skipped) --- */
gf_status gf_matmul_forward_host_f64(gf_ctx *ctx, const double *A, const double *B, double *C, int M, int K, int N);
gf_status gf_matmul_backward_host_f64(gf_ctx *ctx, const double *dC, const double *A, const double *B, double *dA,
                                      double *dB, int M, int K, int N);
gf_status gf_mattensormul_forward_host_f64(gf_ctx *ctx, const double *X, const double *F, double *Out, int R, int Kd, int J, int D);
gf_status gf_mattensormul_backward_host_f64(gf_ctx *ctx, const double *G, const double *X, const double *F, double *dX,
                                            double *dF, int R, int Kd, int J, int D);
gf_status gf_tensormatmul_forward_host_f64(gf_ctx *ctx, const double *F, const double *Y, double *Out, int R, int Kd, int J, int D);
gf_status gf_tensormatmul_backward_host_f64(gf_ctx *ctx, const double *G, const double *F, const double *Y, double *dF,
                                            double *dY, int R, int Kd, int J, int D);
gf_status gf_custommatmultensor_forward_host_f64(gf_ctx *ctx, const double *W, const double *T, double *Out, long long rows,
                                                 int V, int Kout);
gf_status gf_custommatmultensor_backward_host_f64(gf_ctx *ctx, const double *G, const double *W, const double *T, double *dW,
                                                  double *dT, long long rows, int V, int Kout);
gf_status gf_custommatmultensor_forward_host_f32(gf_ctx *ctx, const float *W, const float *T, float *Out, long long rows,
                                                 int V, int Kout);
gf_status gf_custommatmultensor_backward_host_f32(gf_ctx *ctx, const float *G, const float *W, const float *T, float *dW,
                                                  float *dT, long long rows, int V, int Kout);
gf_status gf_stack_forward_host_f64(gf_ctx *ctx, const double *const *tensors, double *out, int nRows, size_t per_tensor);
gf_status gf_stack_backward_host_f64(gf_ctx *ctx, const double *G, double *const *grads, int nRows, size_t per_tensor);
gf_status gf_stack_forward_host_f32(gf_ctx *ctx, const float *const *tensors, float *out, int nRows, size_t per_tensor);
gf_status gf_stack_backward_host_f32(gf_ctx *ctx, const float *G, float *const *grads, int nRows, size_t per_tensor);
gf_status gf_matmul_forward_host_f32(gf_ctx *ctx, const float *A, const float *B, float *C, int M, int K, int N);
gf_status gf_matmul_backward_host_f32(gf_ctx *ctx, const float *dC, const float *A, const float *B, float *dA, float *dB,
                                      int M, int K, int N);
gf_status gf_mattensormul_forward_host_f32(gf_ctx *ctx, const float *X, const float *F, float *Out, int R, int Kd, int J, int D);
gf_status gf_mattensormul_backward_host_f32(gf_ctx *ctx, const float *G, const float *X, const float *F, float *dX,
                                            float *dF, int R, int Kd, int J, int D);
gf_status gf_tensormatmul_forward_host_f32(gf_ctx *ctx, const float *F, const float *Y, float *Out, int R, int Kd, int J, int D);
gf_status gf_tensormatmul_backward_host_f32(gf_ctx *ctx, const float *G, const float *F, const float *Y, float *dF,
                                            float *dY, int R, int Kd, int J, int D);

/* ---- batched SMP_omega driver (mode B): the caller of the ops above ------------------------------------------------
 * Reproduces the op DAG of SMP_omega::complete_computation_graph (GraphFlow/SMP_omega.h:584-693) for a batch of
 * molecules: host graph preparation (Floyd-Warshall :358, WL features :382, ranking :406, receptive fields with the
 * omega cap :476-537, selection maps :461, reduced adjacency :556) + device levels (promotion as an index gather,
 * RisiContraction_18, K-projection, bias, LeakyReLU) + readout (:676-692) + the reverse sweep.
 * Parameters are ONE flat fp32 device buffer in the reference's registration / save_model order
 * (SMP_omega.h:289-295, 1033-1055): H[C][F(D+1)], then K_l[18C][C], b_l[C] for l = 1..L, then W[C];
 * gradients have the same layout and hold the SUM over the batch (what sum_gradients accumulates, :808-820), so a
 * data-parallel step is one all-reduce of that buffer.                                                                */
typedef struct gf_smp gf_smp;
typedef struct {
    int nLevels, nChanels, nFeatures, nDepth, max_receptive_field, has_WL_ordering;
    /* The SMP_2D_ver6 / ver7 / ver8 wirings of the same DAG (GraphFlow/SMP_2D_ver6.h:456-560): contraction family
     * nContractions = 10 / 50 / 18 (0 means 18) and, with custom_matmul = 1, the level weight K_l stored [C][nContractions C]
     * and applied by CustomMatMulTensor instead of Reshape2D + MatMul on [nContractions C][C].  Zero-initialised trailing
     * fields give SMP_omega.  Those models have no receptive-field cap: pass max_receptive_field = max_nVertices.
     * Since round 5 the `_10` and `_50` families (nChanels <= 32) are computed on the fused RisiContraction_18 level: for a symmetric
     * reduced adjacency with a unit diagonal their slices are slices of `_18` on the activations and on their per-node transposes (plus
     * three extra products for `_50`); the parameter / gradient layout at this interface stays the caller's.  A batch the embedding cannot
     * take -- an asymmetric or negative adjacency, a `_50` Coulomb batch, a `_10` Coulomb batch with an entry <= 0 -- is computed on the
     * op-by-op `_10` / `_50` levels instead: gf_smp_prepare picks the plan per batch (round 6; it used to refuse with GF_ERR_UNSUPPORTED),
     * nothing changes at this interface.  GF_SMP_VER6_FUSED=0 / GF_SMP_VER7_FUSED=0 at create time select the op-by-op levels for every batch.
     * nContractions = 4 with custom_matmul = 0 is SMP_gamma (GraphFlow/SMP_gamma.h): RisiContraction_4, K_l = [4C][C] by Reshape2D + MatMul,
     * no receptive-field cap (pass max_receptive_field = max_nVertices), no reduced adjacency (gf_smp_prepare_coulomb gives the results of
     * gf_smp_prepare).  Refused with custom_matmul = 1, and by gf_smp_create with physics = 1 (a gamma tower is built by
     * gf_smp_model_create, gf_smp_model_config.nContractions = 4).  A level runs the fused gamma level (smp_level_gamma.hip) when the
     * channel count the device computes with is a multiple of 4 and at most 64 (gf_smp_create pads any nChanels to a multiple of 4 -- unless
     * GF_SMP_PAD_CHANNELS=0 or nLevels is beyond the padding's limit, where e.g. 5 or 10 channels stay unpadded) and its fields hold at
     * most 64 positions; otherwise, and under gf_smp_set_fused(0), promotion + the batched `_4` kernels run.  Same results either way. */
    int nContractions, custom_matmul;
    /* physics = 1: one TOWER of the `_physics` / `_pairgraphs` models (GraphFlow/SMP_omega_physics.h:29-170, :480-606;
     * SMP_omega_pairgraphs.h builds two of them): raw vertex features (nDepth must be 0; no WL histogram or ordering, the
     * receptive-field cap orders by hop distance only, :436-450), channels halve from level to level (C_l = max(1, C_{l-1} / 2),
     * K_l = [18 C_{l-1}][C_l], :141-156), and EVERY level is read out (:572-588).  Parameters: H[C][F], (K_l, b_l) l = 1..L -- no
     * readout vector.  gf_smp_forward then only fills graph_feature = [nMol][gf_smp_feature_width] (the ConcatVectors row, :590;
     * targets / predict / loss must be NULL) and the reverse sweep starts from gf_smp_backward_features.  The fully-connected
     * head on top is gf_head_*.  SMP_beta_physics / _pairgraphs = the same with max_receptive_field = max_nVertices.
     * nContractions 18 (or 0); 4 (the towers of SMP_gamma_physics / _pairgraphs, K_l = [4 C_{l-1}][C_l]) only through gf_smp_model_create. */
    int physics;
    /* first_order = 1: the FIRST-ORDER models SMP_theta (GraphFlow/SMP_theta.h) and, with physics = 1 through gf_smp_model_create only, the
     * towers of SMP_theta_physics / SMP_theta_pairgraphs.  Same graph preparation, receptive fields (growth, cap, WL ordering), level-0
     * embedding, read-out, Adam and API as SMP_omega; the level differs.  f_l[v] is a matrix [s][C] (s = |phi_l(v)|), not a tensor:
     *   S = sum over the children w (hop distance <= 1 from v, NOT the members of the field, SMP_theta.h:577-583) of X[v][w] f_{l-1}[w],
     *   f_l[v] = LeakyReLU([lambda1_s S | lambda2_s 1 1^T S] K_l + 1 b_s^T)                                      (:586-612)
     * with scalars lambda1_s, lambda2_s and a bias b_s[C] PER FIELD SIZE s = 1 .. max_nVertices and K_l = [2 C][C] ([2 C_{l-1}][C_l] in a
     * tower); the read-out sums a node's s rows (ShrinkMatrix).  Parameter order (registration order, :254-264): H; for l = 1..L: for size =
     * 1 .. max_nVertices (lambda1, lambda2, b[C_l]), then K_l; W (no W in a tower).  max_nVertices >= max_receptive_field is required:
     * the parameter count depends on it, and gf_smp_prepare refuses a molecule with more vertices.  nContractions / custom_matmul must be 0.
     * The level is smp_level_theta.hip: products on the rows of the level below, deterministic gathers; any nChanels, no channel
     * padding, no field-size limit other than int16 positions.  gf_smp_level_sizes: rows = sum of s, ppos = 0.  gf_smp_prepare_coulomb behaves
     * as gf_smp_prepare (the model has no reduced adjacency), gf_smp_set_fused has no effect (there is one plan), gf_smp_read_activation
     * returns [s][C].  Refused with GF_ERR_UNSUPPORTED before anything is launched:
     *   - gf_smp_create_classifier on a first_order = 1 configuration,
     *   - gf_smp_set_grad_allreduce(smp, 1) on a first-order handle (no data-parallel exchange: reduce the flat gradient yourself),
     *   - gf_smp_dropout_masks on a first-order handle.
     * Zero-initialised trailing fields give the behaviour described above.
     *
     * first_order = 2, 3, 4: the second first-order family, SMP_1D, SMP_1D_ver2 and SMP_1D_ver3 (GraphFlow/SMP_1D.h, SMP_1D_ver2.h,
     * SMP_1D_ver3.h).  Fields (union over the vertices within one hop, WL ordering), children, S, the per-size lambda1_s, lambda2_s, b_s and
     * the read-out are SMP_theta's; there is NO cap and no [2 C][C] matrix.  With sumS = sum_i S[i]:
     *   2  SMP_1D       z[i] = lambda1_s S[i] + lambda2_s sumS + b_s                 C_l = C;        LeakyReLU2D slope 0.01
     *   3  SMP_1D_ver2  z[i] = [lambda1_s S[i] | lambda2_s sumS] + b_s               C_l = C << l;   slope 0, level 0 included
     *   4  SMP_1D_ver3  z[i] = [lambda1_s S[i] K_eye | lambda2_s sumS K_one] + b_s   C_l = C << l;   slope 0; K_eye, K_one [C_{l-1}][C_{l-1}]
     * (the read-out's LeakyReLU keeps 0.01).  Parameter order (registration order): H [C][F (D + 1)]; for l = 1..L: for size = 1 ..
     * max_nVertices (lambda1, lambda2, b[C_l]), then for first_order = 4 K_eye, K_one; W [C_L].  The graph feature, gf_smp_feature_width and
     * the rows of W are C_L wide: C, or C << nLevels.  Required, else GF_ERR_INVALID: max_receptive_field == max_nVertices and
     * nContractions = custom_matmul = physics = 0 (gf_smp_config_param_count then answers 0, gf_smp_prepare_molecule_host GF_ERR_INVALID).
     * The gradients of lambda1_s / lambda2_s are the CLASSES', not the derivative: the reference runs its shared per-size ops once per vertex
     * of the size on accumulating gradients, so the j-th such vertex of a molecule counts j times in SMP_1D_ver2 / ver3 (as in SMP_theta)
     * and j (j + 1) (j + 2) / 6 times in SMP_1D (three shared ops in a row).  Every other gradient is plain.  The optimiser of the classes
     * is Momentum: gf_smp_momentum_step.  The level is smp_level_1d.hip: no GEMM at all in SMP_1D / ver2, one forward and two backward per
     * level in ver3; none of the 18-slice or gamma buffers.  gf_smp_create_classifier ACCEPTS these three values (SMP_1D_classification,
     * SMP_1D_ver3_classification; 3 gives the same read-out on SMP_1D_ver2): W [nClass][C_L].  Still refused with GF_ERR_UNSUPPORTED:
     * gf_smp_set_grad_allreduce(smp, 1) and gf_smp_dropout_masks.  gf_smp_model_create has no towers of these forms. */
    int first_order, max_nVertices;
    /* 1: SMP_2D, 2: SMP_2D_ver4 (GraphFlow/SMP_2D.h, SMP_2D_ver4.h) -- the second-order STEERABLE models: no contraction and no matrix
     * product.  f_l[v] is [s][s][C_l] on the field phi_l(v) = the union of the level-below fields of the vertices within one hop (no cap, WL
     * ordering).  Level 0 is MatMul(H, feature) as [1][1][C]; for l >= 1, with pi_w the position map of a child w (hop distance <= 1):
     *   S[i][j]   = sum_w f_{l-1}[w][pi_w(i)][pi_w(j)] + scalar_l * adj_v[i][j]         (terms with a missing position are zero)
     *   col[j]    = sum_k S[k][j]
     *   1  SMP_2D       z[i][j] = lambda1_s S[i][j] + lambda2_s col[j] + b_s              C_l = C
     *   2  SMP_2D_ver4  z[i][j] = [lambda1_s S[i][j] | lambda2_s col[j]] + b_s            C_l = C << l
     *   5  SMP_2D_ver5  z[i][j] = K_l [lambda1_s S[i][j] | lambda2_s col[j]] + b_s        C_l = C   (K_l [C][2 C], CustomMatMulTensor)
     *   f_l[v] = LeakyReLU3D(z), slope 0.01 at every level
     * per CHANNEL: lambda1_s, lambda2_s, scalar_l are [C_{l-1}], b_s is [C_l].  adj_v is the adjacency reduced to phi_l(v); in SMP_2D_ver4
     * its diagonal is 1 and every row is divided by its sum.  Read-out: sum over (i, j), LeakyReLU, sum over the vertices; InnerProduct with
     * W [C_L] and squared loss, or with gf_smp_create_classifier MatVecMul with W [nClass][C_L] and LogLoss (SMP_2D_classification,
     * SMP_2D_ver4_classification).  Parameter order (registration order): H [C][F (D + 1)]; for l = 1..L: for size = 1 .. max_nVertices
     * (lambda1, lambda2, b), then scalar_l; W.  gf_smp_feature_width is C_L.  Required, else GF_ERR_INVALID: first_order == 0,
     * max_receptive_field == max_nVertices <= 4096, nContractions = custom_matmul = physics = 0 (gf_smp_config_param_count then answers 0).
     * The gradients of lambda1_s / lambda2_s are the CLASSES', not the derivative (see first_order): the j-th vertex of a size in a
     * molecule counts j (j + 1) / 2 times in SMP_2D (two shared ops in a row) and j times in SMP_2D_ver4; every other gradient is plain.
     * The optimiser of the classes is Momentum: gf_smp_momentum_step.  gf_smp_read_activation returns [s][s][C_l],
     * gf_smp_read_reduced_adjacency the class's adj_v, gf_smp_level_sizes rows = sum of s^2.  The level is smp_level_2d.hip: no GEMM, no
     * atomics.  Refused with GF_ERR_UNSUPPORTED before anything is launched: gf_smp_set_grad_allreduce(smp, 1), gf_smp_dropout_masks,
     * gf_smp_backward_features, gf_smp_prepare_coulomb with a Coulomb matrix (the classes have no such constructor).  gf_smp_model_create
     * has no towers of these forms.  0 (a zero-initialised tail): everything as described above.
     * 5: SMP_2D_ver5 (GraphFlow/SMP_2D_ver5.h; the value is the class's version number, 3 and 4 are refused) -- SMP_2D_ver4's level, its
     * reduced adjacency and its multiplicity j included, with the 2 C concatenated channels projected back to C by a learned K_l [C][2 C]
     * (row = output channel, columns [eye half | one half]): the one steerable model whose width does not double per level.  Its matrix
     * block is K_l then scalar_l; gf_smp_uniform_init_host draws K_l as one block (divisor 10 * 2 C^2).  dK_l is the plain derivative (K_l
     * is one node of the class's graph).  Also required: nChanels <= 128 (a level's K1 image sits in LDS).  The level is
     * smp_level_2d_ver5.hip: the row projection on v_mfma_f32_32x32x2_f32 with fp32 accumulation, no atomics.  gf_smp_create_classifier
     * answers GF_ERR_UNSUPPORTED (there is no SMP_2D_ver5_classification); the other refusals are those of 1 and 2. */
    int steerable_2d;
    /* 1: Unrestricted_SMP_1D, 2: Unrestricted_SMP_1D_ver2, 3: Unrestricted_SMP_2D (GraphFlow/Unrestricted_SMP_*.h) -- SMP_1D, SMP_1D_ver2
     * and SMP_2D with a DENSE learned filter per field size s in place of lambda1_s I + lambda2_s 1 1^T.  Fields, children, level 0, the
     * read-out and the loss are the restricted model's (first_order = 2, 3; steerable_2d = 1).  With S the gather-sum over the children
     * (form 3: on both indices, plus scalar_l * adj_v, adj_v the molecule's adjacency on the field as it stands) and Cp = C_{l-1}:
     *   1  z[i][c]    = sum_k W_s[i][k] S[k][c] + b_s[c]                 C_l = C        LeakyReLU2D slope 0.01
     *   2  z[i]       = [ (W1_s S)[i] | (W2_s S)[i] ] + b_s              C_l = C << l   slope 0, level 0 included (the read-out keeps 0.01)
     *   3  z[i][j][c] = sum_k W_s[i][k][c] S[k][j][c] + b_s[c]           C_l = C        LeakyReLU3D slope 0.01
     * Parameter order (registration order): H [C][F (D + 1)]; for l = 1..L: for size = 1 .. max_nVertices (1: W_s [s][s]; 2: W1_s, W2_s
     * [s][s]; 3: W_s [s][s][C], the channel innermost; then b_s [C_l]), in form 3 then scalar_l [C]; W [C_L].  The entries grow with the
     * size: entry s of a level starts fl (s - 1) s (2 s - 1) / 6 + (s - 1) C_l floats into its block, fl = 1, 2, C.  Required, else
     * GF_ERR_INVALID: first_order == 0 and steerable_2d == 0, max_receptive_field == max_nVertices <= 4096, nContractions = custom_matmul
     * = physics = 0, a parameter count that fits an int (gf_smp_config_param_count then answers 0).  The classes register W_s / b_s once
     * per graph, not once per vertex: EVERY gradient is the plain derivative (unlike first_order / steerable_2d).  The optimiser of the
     * classes is Momentum: gf_smp_momentum_step; gf_smp_uniform_init_host draws every W_s, b_s as a block of its own.
     * gf_smp_read_activation returns [s][C_l] (1, 2) or [s][s][C] (3); gf_smp_read_reduced_adjacency answers -1 (1, 2) or adj_v (3);
     * gf_smp_level_sizes rows = sum of s (1, 2) or of s^2 (3).  The level is smp_level_unrestricted.hip: no GEMM, no atomics.  Refused with
     * GF_ERR_UNSUPPORTED before anything is launched: gf_smp_create_classifier (the reference has no such class), gf_smp_set_grad_allreduce
     * (smp, 1), gf_smp_dropout_masks, gf_smp_backward_features, gf_smp_prepare_coulomb with a Coulomb matrix.  gf_smp_model_create has no
     * towers of these forms.  0 (a zero-initialised tail): everything as described above. */
    int unrestricted;
    /* neighbourhood = 1: NeuralFingerprint, 2: GCN_1D, 3: GCN_2D (GraphFlow/NeuralFingerprint.h, GCN_1D.h, GCN_2D.h) -- the baselines the
     * CCN / SMP results are reported against.  One vector h_l[v] [H] per vertex and level, H = nChanels (the classes' nHiddens); no receptive-
     * field tables, no contraction, no per-size blocks:
     *   h_0[v] = softmax(W1_0 x[v])
     *   n_l[v] = aggregate of h_{l-1}[u] over N_l(v);   h_l[v] = softmax(W1_l x[v] + W2_l n_l[v])        l = 1 .. nLevels
     *   predict = <W, sum_v h_L[v]>,  loss = 0.5 (predict - target)^2
     *   1  x[v] = feature[v] (F' = nFeatures; nDepth must be 0)   N_l(v) = { u : adj[v][u] > 0 } as written: v itself is NOT a member and an
     *      asymmetric matrix is taken one-sided; an isolated vertex has n = 0                        aggregate: sum (SumVectors)
     *   2  x[v] = the shell sums, block d = sum of feature[u] over dist(u, v) == d, d = 0 .. nDepth (F' = nFeatures (nDepth + 1))
     *      N_l(v) = { u : dist(v, u) <= min(l, max_Radius) }, v included                             aggregate: sum (RisiLayer1D)
     *   3  x as 2;  N_l(v) = { u : dist(v, u) <= l } (the class stores max_Radius and never reads it: ignored here too)
     *      aggregate RisiLayer2D: n[i] = sum_k sum_{u<w} (a_u[i] a_w[k] + a_u[k] a_w[i]) = A[i] Tt - sum_u a_u[i] T_u with T_u = sum_k a_u[k],
     *      A = sum_u a_u, Tt = sum_u T_u -- evaluated in that closed form, O(m H) for m members; T_u is 1 only in exact arithmetic and the
     *      class differentiates through it, so the device does too.  A one-vertex neighbourhood gives n = 0.
     * dist is the hop distance of the other models (the classes' Floyd-Warshall, literally).  The gradient is the CLASSES': Softmax::backward
     * is diagonal-only, dz[i] = dh[i] h[i] (1 - h[i]), not the full Jacobian; every other gradient is the plain derivative (W1_l, W2_l enter
     * the graph once per level).  Parameter order (registration and save_model order): W1_0 [H][F']; for l = 1..L: W1_l [H][F'], W2_l [H][H];
     * W [H].  nLevels = 0 is valid (level 0 and the read-out).  Required, else GF_ERR_INVALID (gf_smp_config_param_count then answers 0):
     * first_order = steerable_2d = unrestricted = physics = nContractions = custom_matmul = 0, max_receptive_field == max_nVertices, form 1:
     * nDepth == 0, form 2: max_Radius >= 0, nChanels <= 128 and (F' + nChanels) (nChanels | 1) + (256 / G) nChanels floats within 160 KiB, G = the
     * power of two at or above nChanels, at least 8 and at most 64 (a level's W1_l and W2_l sit in LDS beside one vector per group of G
     * lanes: F' <= 185 at 128 channels).  gf_smp_prepare refuses a molecule above max_nVertices.  The optimiser of the classes is
     * Momentum: gf_smp_momentum_step.  gf_smp_uniform_init_host draws in the classes' order: every W1_l / W2_l by uniform_init(Matrix*)
     * (divisor 10 * nRows = 10 H), W by uniform_init(Vector*) (10 H) -- after srand(seed) the classes' weights bit for bit.
     * gf_smp_read_activation(mol, l, v) returns h_l[v] [H]; gf_smp_receptive_field N_l(v) in ascending vertex order (level 0: {v});
     * gf_smp_level_sizes nodes = rows = vertices, ppos = 0; gf_smp_feature_width H; gf_smp_read_reduced_adjacency answers -1;
     * gf_smp_set_fused has no effect.  The level is smp_level_neighbourhood.hip: one forward launch per level, deterministic gathers over
     * the neighbour lists and their transposes, dW1_l / dW2_l as deterministic TN products; no atomics.  Refused with GF_ERR_UNSUPPORTED
     * before anything is launched: gf_smp_create_classifier, gf_smp_set_grad_allreduce(smp, 1), gf_smp_dropout_masks,
     * gf_smp_backward_features, gf_smp_prepare_coulomb with a Coulomb matrix.  gf_smp_model_create has no towers of these forms.
     * neighbourhood = 4: GRU_GCN_1D, 5: GRU_GCN_2D (GraphFlow/GRU_GCN_1D.h, GRU_GCN_2D.h) -- the gated graph networks of the same comparison:
     * x, dist and the aggregates of forms 2 (4: sum) and 3 (5: RisiLayer2D in the closed form), N_l(v) = { u : dist(v, u) <= min(l, max_Radius) },
     * v included, in BOTH forms (GRU_GCN_2D does read max_Radius), and a GRU cell as the level's update:
     *   h_0[v] = softmax(W x[v])
     *   l = 1..L:  n = the aggregate of h_{l-1}[u] over N_l(v), hp = h_{l-1}[v]
     *              z = sigmoid(W_z n + U_z hp)   r = sigmoid(W_r n + U_r hp)   c = tanh(W_h n + U_h (r * hp))   h_l[v] = (1 - z) * hp + z * c
     *   g_v = sigmoid(W_g h_L[v]) * tanh(U_g h_L[v]);  graph_feature = tanh(sum_v g_v);  predict = <U, graph_feature>, squared loss
     * The parameters are shared by all levels; order (registration and save_model order): W [H][F']; W_z, U_z, W_r, U_r, W_h, U_h, W_g, U_g
     * [H][H]; U [H] -- H F' + 8 H^2 + H floats whatever nLevels is.  Gradients are the plain derivatives, summed over the levels, except level
     * 0's softmax (the classes' diagonal rule, as above).  From level 1 on h_l is no softmax vector: T = sum_k h_l[k] is kept per level.
     * Required, else GF_ERR_INVALID: form 2's rules (max_Radius >= 0 in both forms) and nChanels <= 64 -- the six [H][H | 1] images of a cell
     * are resident in LDS for the length of a level: 99.8 KB at 64 channels, 396 KB at 128 against 160 KiB per workgroup.  gf_smp_uniform_init_host
     * draws every block by uniform_init(Vector*) -- the classes initialise through sgd->params[i] -- so the divisor is 10 * the block's size
     * (10 H F', 10 H^2, 10 H), not form 2's 10 H.  Introspection, the Momentum optimiser and the five GF_ERR_UNSUPPORTED refusals are those of
     * forms 1 - 3; gf_smp_classifier_config_param_count answers 0.  The level is smp_level_gru.hip: level 0 and the reverse gather are
     * smp_level_neighbourhood.hip's kernels, one gru_cell_fwd / gru_cell_bwd launch per level, the eight weight gradients deterministic TN
     * products accumulated over the levels from the top down; no atomics.
     * neighbourhood = 6: GCN_3D, 7: GRU_GCN_3D (GraphFlow/GCN_3D.h, GRU_GCN_3D.h) -- forms 2 and 4 (x, N_l(v) = { u : dist(v, u) <= min(l,
     * max_Radius) } in both, level 0, the update, the read-out, the parameter blocks, their order and the way uniform_init draws them) with the
     * third-order aggregate  n_l[v] = KMax(RisiLayer3D(members), K = H):  T[x, y, z] = sum over ordered triples (i, j, k) of distinct members of
     * a_i[x] a_j[y] a_k[z], of whose H^3 entries the H largest are kept in ascending order (n[H - 1] the largest).  T is symmetric, so it is
     * evaluated per class x <= y <= z (6, 3 or 1 equal entries) in the closed form A_x A_y A_z - B_yz A_x - B_xz A_y - B_xy A_z + 2 sum_u
     * a_u[x] a_u[y] a_u[z], A = sum_u a_u, B_pq = sum_u a_u[p] a_u[q]; which entries of a class are kept changes no value and no gradient.
     * Between classes the choice is a kink: the device agrees with the fp64 class wherever adjacent classes around the cut differ by more
     * than the fp32 evaluation error (about 1e-6 max|T|).  Exactly equal fp32 values of two classes: the larger flat index z H^2 + y H + x of
     * the classes' largest entries is kept first.  Under three members T = 0: n = 0 exactly and nothing flows back (max_Radius = 0: every
     * level is softmax(W1_l x), or a cell with n = 0).  Required, else GF_ERR_INVALID: form 2's rules, nChanels <= 64, and max_nVertices within
     * what a neighbourhood's members take in LDS beside the select's tables: (160 KiB - 25,632 - 4 H - 4 H^2) / (4 H) vertices, 474 at 64
     * channels.  Introspection, the Momentum optimiser and the five GF_ERR_UNSUPPORTED refusals are those of forms 1 - 5.  The level is
     * smp_level_third.hip: one third_pool_fwd launch per level ahead of the update kernel of form 2 / 4, one third_pool_bwd in place of their
     * reverse gather; no float atomics, two runs give the same bits.
     * 0 (a zero-initialised tail): everything as described above, max_Radius is not read. */
    int neighbourhood, max_Radius;
    /* matrix_form = 1: LCNN (PATCHY-SAN, GraphFlow/LCNN.h), 2: GCN_MW (the Kipf-Welling GCN in matrix form, GraphFlow/GCN_MW.h) -- the two
     * matrix-form baselines.  Both run on the row-list GEMM level (smp_level_rowlist.hip): every output row is a short list of rows of the level
     * below, concatenated slot by slot (LCNN) or weighted and summed (GCN_MW), times a learned matrix; the A operand is assembled from the
     * list inside the product and never written to memory.  x [V][F'], F' = nFeatures (nDepth + 1), and dist are those of forms 2 .. 7.
     * LeakyReLU has slope 0.01, the loss is 0.5 (predict - target)^2, every gradient is the plain derivative, the optimiser is Momentum
     * (gf_smp_momentum_step).
     *   2  GCN_MW: A-hat = D^-1/2 (A + I) D^-1/2 with D the row sums of A + I (DenseGraph::create_norm_adj: A-hat[i][j] = d_i (A + I)[i][j]
     *      d_j in double, also for an asymmetric A), h_0 = LeakyReLU((A-hat x) W_0), h_l = LeakyReLU((A-hat h_{l-1}) W_l), graph feature =
     *      sum_v h_L[v] [H], predict = <W, graph feature>.  nChanels = nHiddens = H.  Parameters in registration (= save_model) order:
     *      W_0 [F'][H], W_l [H][H] for l = 1 .. nLevels, W [H]; uniform_init draws every W_l as a Matrix (divisor 10 x rows), W as a Vector.
     *      nLevels = 0 is a model.  nNeighbors, nChanels2, nDense are not read.
     *   1  LCNN(nVertices = max_nVertices, nFeatures, nNeighbors = k, nDepth, nChanels1 = nChanels, nChanels2, nDense); nLevels must be 2
     *      (the two convolutions).  Every molecule is padded to V = max_nVertices vertices: dummy vertices have zero features and no edges;
     *      dist and x are those of the padded graph.  order = the class's exchange sort, descending by the lexicographic comparison of the x
     *      rows (rank_vertices); sequence (find_sequence): for rank position i, walking d = 0 .. V - 1 and inside that the rank positions
     *      v = 0 .. V - 1, vertex order[v] is appended when dist(order[i], order[v]) == d and order[v] < molV, up to k entries; the rest is
     *      padded with the value molV (a dummy order[i] gets k pads).  Layer 1: c1[i] = [x[seq[i][0]] | .. | x[seq[i][k - 1]]] F1 + b1, F1
     *      [k][F'][C1]; a1 = LeakyReLU(c1); row i belongs to rank position i.  Layer 2: c2[i] = [a1[seq[i][0]] | ..] F2 + b2, F2 [k][C1][C2]:
     *      the class indexes a1, whose rows are RANK POSITIONS, with the VERTEX IDS of the sequence, and so does the device.  The dense layer
     *      reads the pre-activation c2 (the class's second LeakyReLU feeds nothing): dense = Dm vec(c2), Dm [nDense][V C2], vec row-major;
     *      predict = <W, dense>; the graph feature is dense (gf_smp_feature_width = nDense).  Parameters: F1, b1 [C1], F2, b2 [C2], Dm,
     *      W [nDense], each drawn as a Vector (divisor 10 x its size).  A pad entry reads row molV: with molV < V a valid row; with molV == V
     *      the class reads past its matrix, and gf_smp_prepare refuses such a batch with GF_ERR_INVALID, naming the molecule (a full-size
     *      molecule with a vertex that reaches fewer than k vertices).
     * Required, else GF_ERR_INVALID: every other form selector (first_order, steerable_2d, unrestricted, neighbourhood, physics,
     * nContractions, custom_matmul) 0, max_receptive_field == max_nVertices <= 4096, nChanels, nFeatures >= 1, nDepth >= 0; form 2: nLevels
     * in 0 .. 64; form 1: nLevels == 2, nNeighbors, nChanels2, nDense >= 1.  The kernels index an operand row and a tile count with ints:
     * every operand width -- F', nChanels, nChanels2, nDense, nNeighbors F', nNeighbors nChanels, max_nVertices nChanels2 -- is at most
     * 65536 and the parameter count fits an int; a batch of more than 2^31 - 1 rows or list entries is refused by gf_smp_prepare.
     * Refused with GF_ERR_UNSUPPORTED before anything is launched: gf_smp_create_classifier, gf_smp_set_grad_allreduce(smp, 1),
     * gf_smp_dropout_masks, gf_smp_backward_features, gf_smp_prepare_coulomb with a matrix; gf_smp_model_create has no towers of these
     * forms.  gf_smp_set_fused has no effect.  gf_smp_receptive_field(mol, l, i): LCNN: the k entries of the sequence of rank position i
     * (level 0: {order[i]}), GCN_MW: the non-zero columns of row i of A-hat, ascending.  gf_smp_read_activation: LCNN level 1: a1[i] [C1],
     * level 2: c2[i] [C2]; GCN_MW: h_l[v] [H].  gf_smp_level_sizes: nodes = rows = nMol V (LCNN) or the batch's vertices (GCN_MW), ppos = 0.
     * 0 (a zero-initialised tail): everything as described above, the three LCNN fields are not read. */
    int matrix_form, nNeighbors, nChanels2, nDense;
    /* distance_channel = 1 with neighbourhood = 2, 3, 6: GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance (GraphFlow/GCN_1D_Distance.h,
     * GCN_2D_Distance.h, GCN_3D_Distance.h) -- the only models that read DenseGraph::distance.  Each is two copies of the softmax level of
     * forms 2 / 3 / 6 side by side over the same neighbour lists, with weights of their own: the vertex channel reads the shell sums x_v[v]
     * [F'], the distance channel x_d[v] [M], M = max_nVertices: COLUMN v of the molecule's V x V distance matrix (distance[u][v], u = 0 .. V - 1),
     * padded with M - V zeros and sorted ascending (the class's Sort op; the zeros of the padding and of the diagonal sort among the values,
     * negative entries before them; the values are data, nothing flows back through the sort).  Per channel c in {v, d}:
     *   h^c_0[v] = softmax(W1^c_0 x_c[v]);   h^c_l[v] = softmax(W1^c_l x_c[v] + W2^c_l n^c_l[v]),  n^c_l = the aggregate of h^c_{l-1} over N_l(v)
     *   graph feature = [ sum_v h^v_L[v] | sum_v h^d_L[v] ]  [2 H];   predict = <W, graph feature>;   loss = 0.5 (predict - target)^2
     * N_l(v) = { u : dist(v, u) <= min(l, max_Radius) } in ALL three (GCN_2D_Distance reads max_Radius, unlike GCN_2D); the aggregate is the
     * sum (2), RisiLayer2D in the closed form (3), KMax(RisiLayer3D, H) (6).  Softmax::backward is the diagonal rule of forms 1 - 7.
     * Parameter order (registration, Momentum and uniform_init order): for l = 0 .. L: W1^v_l [H][F'], W1^d_l [H][M], and for l > 0 W2^v_l [H][H],
     * W2^d_l [H][H]; then W [2 H].  Matrices draw with the divisor 10 H, W as a Vector with 10 * 2 H.  The classes' save_model / load_model
     * use ANOTHER order -- all vertex-channel blocks by level, all distance-channel blocks by level, W -- and gf_smp_save_model /
     * gf_smp_load_model permute for these handles, so checkpoints are the classes' files.
     * The molecules come through gf_smp_prepare_distance; gf_smp_prepare / gf_smp_prepare_coulomb on such a handle are GF_ERR_INVALID.
     * Required, else GF_ERR_INVALID: neighbourhood in {2, 3, 6} with that form's rules (6: nChanels <= 64 and its max_nVertices bound),
     * max_Radius >= 0 in all three, and the LDS bound of form 2 for BOTH operand widths F' and M.  gf_smp_read_activation(mol, l, v) returns
     * [h^v_l[v] | h^d_l[v]] (2 H); gf_smp_feature_width 2 H; the other introspection calls, the Momentum optimiser and the five
     * GF_ERR_UNSUPPORTED refusals are those of forms 1 - 7.  x_d is built on the device (smp_level_distance.hip: dist_rows_sort, a bitonic
     * network across lanes up to 64 entries, through LDS above); a level is one forward launch, one node launch and one gather for both
     * channels (blockIdx.y selects the operand set); the weight gradients are 2 (2 L + 1) deterministic TN products; no atomics.
     * 0 (a zero-initialised tail): everything as described above. */
    int distance_channel;
    /* readout = 1 with neighbourhood = 2, 3, 6: GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (GraphFlow/GCN_1D_Kernel.h, GCN_2D_Kernel.h,
     * GCN_3D_Kernel.h) -- kernel learning on a PAIR of graphs.  Graphs X and Y go through the levels of forms 2 / 3 / 6 with the same weights
     * (x, dist, level 0, the update, the aggregates and the diagonal Softmax::backward are the forms' own); only what sits above h_L differs:
     *   graph feature = [ sum_v h^X_L[v] | sum_v h^Y_L[v] ]  [2 H];   predict = <W, graph feature>, W [2 H];   loss = 0.5 (predict - target)^2
     * N_l(v) = { u : dist(v, u) <= min(l, max_Radius) } in ALL three (GCN_2D_Kernel reads max_Radius, as GCN_2D_Distance does and GCN_2D does
     * not).  W1_l and W2_l enter the graph once per level: their gradient is the sum over the vertices of both graphs.  Parameter order
     * (registration, Momentum and save_model order): W1_0 [H][F']; for l = 1..L: W1_l [H][F'], W2_l [H][H]; W [2 H].  Matrices draw with the
     * divisor 10 H, W as a Vector with 10 * 2 H.  The batch comes through gf_smp_prepare_pairs (gf_smp_prepare, _coulomb and _distance on such a
     * handle are GF_ERR_INVALID): it is the 2 nPairs graphs X_0, Y_0, X_1, Y_1, .. on the lists and tables of forms 2 / 3 / 6; X and Y may have
     * different vertex counts, each at most max_nVertices.  gf_smp_forward: targets, predict, loss [nPairs], graph_feature [nPairs][2 H];
     * gf_smp_feature_width 2 H.  The molecule index of gf_smp_receptive_field, gf_smp_read_activation and gf_smp_level_sizes is 2 p for X_p,
     * 2 p + 1 for Y_p.  The read-out is smp_level_readouts.hip: one wave per pair (the two segment sums in ascending vertex order), dW as a
     * fold over the pairs in fixed order, dh_L[v] = dy[pair(v)] W[side(v) H + c] written before the levels' unchanged reverse kernels.
     * readout = 2 with neighbourhood = 2: GCA_1D (GraphFlow/GCA_1D.h, LinearGram.h) -- the graph auto-encoder.  The levels are GCN_1D's; there
     * is no W and no target:
     *   G[x][y] = <h_L[x], h_L[y]>  (V x V per molecule);   loss = 0.5 sum_{x,y} (G[x][y] - adj[x][y])^2,  adj[x][y] taken as its integer VALUE
     *   (an entry of 2 counts as 2, an asymmetric matrix is taken as written);   with E = G - adj:  dh_L[x] = sum_y (E[x][y] + E[y][x]) h_L[y]
     *   (LinearGram::backward: the diagonal term counts twice).
     * Parameters: GCN_1D's without W.  gf_smp_prepare as for form 2 (it also uploads the adjacency values as floats).  gf_smp_forward: targets,
     * predict and graph_feature must be NULL (GF_ERR_INVALID otherwise), loss [nMol] is the per-molecule loss; gf_smp_feature_width 0; gf_smp_gram
     * copies G.  gf_smp_backward works after any forward (the target is the batch itself).  The read-out is gram_readout of
     * smp_level_readouts.hip: one workgroup per molecule, h_L [V][H] staged once into LDS with the row stride H | 1, E [V][V | 1] beside it, G,
     * the loss (a fixed-order reduction) and dh_L = (E + E^T) h_L from one launch, fp32 FMAs.  Required beside form 2's rules: 4 (max_nVertices
     * (nChanels | 1) + max_nVertices (max_nVertices | 1) + 4) bytes within 160 KiB.
     * Both: required, else GF_ERR_INVALID (gf_smp_config_param_count answers 0): readout in 0 .. 2, distance_channel = matrix_form = 0, the
     * neighbourhood named above, and the underlying form's rules unchanged (the LDS bound, nChanels <= 64 and the max_nVertices bound of form
     * 6, max_Radius >= 0).  The optimiser is Momentum; the five GF_ERR_UNSUPPORTED refusals are those of forms 1 - 7; gf_smp_forward_host
     * refuses both read-outs by name (GF_ERR_UNSUPPORTED).  No float atomics; two runs give the same bits.
     * 0 (a zero-initialised tail): everything as described above. */
    int readout;
    /* covariant = 1, 2: CGCN_1D, CGCN_2D (GraphFlow/CGCN_1D.h, CGCN_2D.h) -- the covariant graph convolution networks, on a whole-network
     * vertex level (smp_level_covariant.hip).  A vertex carries ONE vector h_l[v] of length M = max_nVertices, indexed by the molecule's
     * vertex ids; nChanels must be 1.  With sp = the classes' Floyd-Warshall hop counts, x[v] [F'] the shell sums of forms 2 .. 7 and
     * N(v) = { u : adj[u][v] > 0 } (column v of the adjacency itself, ascending; a set diagonal entry makes v its own neighbour):
     *   h_0[v]    = e_v <x[v], H>                                                         (VertexRepresentation)
     *   n_l[v]    = sum_{u in N(v)} h_{l-1}[u]                                            (1: RisiLayer1D)
     *   n_l[v][i] = sum_{u in N(v)} h_{l-1}[u][i] (sum_{w in N(v), w != u} s_w),  s_u = sum_k h_{l-1}[u][k]      (2: RisiLayer2D)
     *   h_l[v][i] = LeakyReLU(sp[i][v] <= l ? (F_l n_l[v])[i] : 0), slope 0.01            (MatVecMul, Masking, LeakyReLU)
     *   graph feature = sum_v h_L[v] [M], predict = the sum of its components (there is no W), loss = 0.5 (predict - target)^2.
     * The exclusive sums of form 2 are evaluated directly, never as S - s_u.  Parameters in registration, Momentum and save_model order:
     * H [F'] (drawn as a Vector, divisor 10 F'), then F_1 .. F_L, each [M][M] row-major (a Matrix, divisor 10 M): F' + L M^2 values.
     * nLevels = 0 is a model.  Positions >= V and positions outside the mask are zero in every h_l, so a level only touches F_l[:V, :V];
     * the classes' reverse pass also puts gradient on such positions, which the mask one level down and VertexRepresentation::backward
     * discard: the device never forms it.
     * Required, else GF_ERR_INVALID (gf_smp_config_param_count answers 0): covariant in 0 .. 2, every other form selector 0 (first_order,
     * steerable_2d, unrestricted, neighbourhood, matrix_form, distance_channel, readout, physics, nContractions, custom_matmul),
     * nChanels = 1, nLevels in 0 .. 64, nFeatures >= 1, nDepth >= 0, 1 <= max_nVertices <= 75 (the kernels keep a molecule's whole
     * network in LDS: 4 (7 M (M | 1) + 2 M + 8) + M M bytes within 160 KiB).  max_receptive_field, has_WL_ordering and max_Radius are
     * not read.  gf_smp_prepare takes the molecules (one above max_nVertices is GF_ERR_INVALID); gf_smp_prepare_distance, _pairs and
     * gf_smp_forward_host answer GF_ERR_UNSUPPORTED, as do the five refusals of forms 1 - 7 (classifier, gf_smp_set_grad_allreduce(1),
     * gf_smp_dropout_masks, gf_smp_backward_features, gf_smp_prepare_coulomb with a matrix).  gf_smp_read_activation(mol, l, v) returns
     * h_l[v] [M]; gf_smp_receptive_field(mol, l, v) the set { u : sp[u][v] <= l }, ascending; gf_smp_feature_width M; gf_smp_level_sizes
     * nodes = rows = the batch's vertices; the optimiser is Momentum (gf_smp_momentum_step); checkpoints are the classes' files.
     * One forward launch (cov_network_fwd: a workgroup per molecule, all levels, h_{l-1} / h_l ping-pong and F_l[:V, :V] in LDS) and one
     * backward launch (cov_network_bwd: a workgroup per chunk of molecules -- the chunks depend on nMol only -- levels in reverse, dh_{l-1}
     * gathered over the transposed lists) plus one fold of at most 256 partial gradient images in ascending order.  No matrix pipe, no
     * float atomics; two runs give the same bits.
     * 0 (a zero-initialised tail): everything as described above. */
    int covariant;
} gf_smp_config;
gf_status gf_smp_create(gf_ctx *ctx, const gf_smp_config *cfg, gf_smp **out);
/* gf_smp_param_count of the handle gf_smp_create would build from cfg (0 on a configuration it would refuse).  Host only. */
size_t    gf_smp_config_param_count(const gf_smp_config *cfg);
/* ... of the handle gf_smp_create_classifier would build from (cfg, nClass); 0 on what it would refuse.  Host only. */
size_t    gf_smp_classifier_config_param_count(const gf_smp_config *cfg, int nClass);
/* The parameter-block table, host only: the blocks the model class registers with sgd->add (e.g. GraphFlow/SMP_omega.h:289-295: H; K_l, b_l
 * per level; W), in that order, as offsets into the flat parameter vector.  Returns the number of blocks and writes count + 1 ascending
 * offsets -- the last one is the parameter count -- when `capacity` >= count + 1; a smaller capacity (or NULL offsets) returns the count
 * and writes nothing; a configuration the create call refuses returns 0.  The table follows sgd->add where that differs from the blocks
 * weights_initialization draws: the distance classes register W1^v_0 and W1^d_0 one by one (GCN_1D_Distance.h:168-169).  AdaMax keeps
 * one infinity norm per block of this table. */
size_t    gf_smp_config_param_blocks(const gf_smp_config *cfg, size_t *offsets, size_t capacity);
size_t    gf_smp_classifier_config_param_blocks(const gf_smp_config *cfg, int nClass, size_t *offsets, size_t capacity);
gf_status gf_smp_destroy(gf_smp *smp);
size_t    gf_smp_param_count(const gf_smp *smp);
/* The `_classification` models: SMP_2D_ver6_classification (nContractions 10, custom_matmul 1) and SMP_2D_ver7_classification (50, 1) of
 * the reference (GraphFlow/SMP_2D_ver6_classification.h:189-200, :560-563, :699-713), and the same read-out on every other non-physics
 * wiring gf_smp_create takes (18, 4).  The levels, their weights, their plans (fused embedding, op-by-op fallback per batch, channel
 * padding) and the Momentum optimiser are those of the regression handle; only the read-out above graph_feature differs:
 *   scores z = MatVecMul(W[nClass][C], graph_feature), probability = softmax(z), loss = LogLoss (GraphFlow/LogLoss.h:37-76).
 * Parameter order: H, (K_l, b_l) for l = 1..L, W[nClass][C] row-major -- the reference's registration and save_model order.  Everything
 * that works through gf_smp_param_count (save / load, the optimisers, parameters_upload / download, forward_host) works on such a handle.
 * gf_smp_forward on a classifier handle:
 *   targets[m]  the label as a float (the reference's (int)target); a label outside [0, nClass) -- undefined behaviour in the reference --
 *               gives loss NaN and contributes no gradient;
 *   predict[m]  the arg-max label as a float, the lowest index on a tie (Predict's strict `>` loop, :706-712);
 *   loss[m]     LogLoss::value = log probability[label], AT MOST 0 (the reference's sign: its BatchLearn returns sums of these; the
 *               quantity the gradient descends is its negative), computed as (z_label - max z) - log sum exp(z - max z) so that it stays
 *               finite where an fp32 probability underflows, and LOG_ZERO = -256 exactly where the reference's fp64 exp underflows;
 *   targets == NULL: scores, probabilities and predict only.
 * nClass >= 2; physics = 1 is refused (GF_ERR_INVALID).  gf_smp_backward is unchanged; gf_smp_backward_features stays refused. */
gf_status gf_smp_create_classifier(gf_ctx *ctx, const gf_smp_config *cfg, int nClass, gf_smp **out);
int       gf_smp_classes(const gf_smp *smp);   /* nClass of a classifier handle, 0 for a regression handle */
/* Of the last gf_smp_forward: predict->value[c] and LogLoss::probability[c], device pointers [nMol][nClass], either may be NULL. */
gf_status gf_smp_class_scores(gf_smp *smp, float *scores, float *probability);
/* Host pointers: nVertices[nMol]; adj = the molecules' V x V int adjacency matrices back to back (DenseGraph::adj);
 * feature = their V x nFeatures matrices back to back (DenseGraph::feature).  Blocking (uploads index tables).
 * Thread safety: DIFFERENT handles of one context may be prepared at the same time from different host threads (each calling
 * thread has its own pool of preparation workers), also while another thread enqueues forward / backward on a third handle:
 * the data-loader pattern of bench.py's end_to_end loop.  One handle is used by one thread at a time. */
gf_status gf_smp_prepare(gf_smp *smp, int nMol, const int *nVertices, const int *adj, const double *feature);
/* The use_coulomb constructors of SMP_omega (SMP_omega.h:71-113): the reduced adjacency of every receptive field is taken
 * from the molecules' V x V Coulomb matrices (DenseGraph::coulomb, back to back; :568-579) instead of 1 / adj.  The
 * bonds in `adj` still define hops, features and fields.  coulomb == NULL is gf_smp_prepare. */
gf_status gf_smp_prepare_coulomb(gf_smp *smp, int nMol, const int *nVertices, const int *adj, const double *feature,
                                 const double *coulomb);
/* The molecules of a distance handle (gf_smp_config.distance_channel = 1): distance = the molecules' V x V matrices of doubles, row-major,
 * back to back like coulomb (DenseGraph::distance).  GF_ERR_INVALID, before anything is launched: an entry that is not finite (the
 * molecule is named), a molecule above max_nVertices.  GF_ERR_UNSUPPORTED on any other handle.  The context stays usable. */
gf_status gf_smp_prepare_distance(gf_smp *smp, int nMol, const int *nVertices, const int *adj, const double *feature,
                                  const double *distance);
/* The pairs of a pair handle (gf_smp_config.readout = 1): two batches in the convention of gf_smp_prepare, nVertices1 / adj1 / feature1 the
 * graphs X_p, nVertices2 / adj2 / feature2 the graphs Y_p, p = 0 .. nPairs - 1.  The device batch is X_0, Y_0, X_1, Y_1, ..  GF_ERR_INVALID
 * before anything is launched: a graph above max_nVertices (the pair and the side are named).  GF_ERR_UNSUPPORTED on any other handle.
 * The context stays usable. */
gf_status gf_smp_prepare_pairs(gf_smp *smp, int nPairs, const int *nVertices1, const int *adj1, const double *feature1, const int *nVertices2,
                               const int *adj2, const double *feature2);
/* The Gram matrices of the last gf_smp_forward of a Gram handle (gf_smp_config.readout = 2) to a DEVICE pointer: the molecules back to back,
 * V_m^2 floats each, row-major.  GF_ERR_UNSUPPORTED on any other handle, GF_ERR_INVALID before a forward. */
gf_status gf_smp_gram(gf_smp *smp, float *out);
/* Device pointers.  targets may be NULL (Predict / Feature); predict, loss [nMol] and graph_feature [nMol][C] are
 * optional outputs (graph_feature is what SMP_omega::Feature returns, :984-996). */
gf_status gf_smp_forward(gf_smp *smp, const float *params, const float *targets, float *predict, float *loss,
                         float *graph_feature);
gf_status gf_smp_backward(gf_smp *smp, const float *params, float *grads, int accumulate);
/* Data-parallel runs (the context has a communicator, gf_dist_init): 1 (default) = gf_smp_backward leaves the gradient
 * summed over all ranks, the all-reduce of each level's [K_l | b_l] segment overlapped with the rest of the reverse sweep
 * (accumulate must be 0 then); 0 = local gradients only (the caller reduces them).  No effect without a communicator. */
gf_status gf_smp_set_grad_allreduce(gf_smp *smp, int on);
/* Physics towers: columns of a feature row (sum of the levels' channel counts), and the reverse sweep from the gradient of
 * the feature rows, d_feature [nMol][width] (what the head's backward hands down: ConcatVectors::backward). */
size_t    gf_smp_feature_width(const gf_smp *smp);
gf_status gf_smp_backward_features(gf_smp *smp, const float *params, float *grads, const float *d_feature, int accumulate);
/* The fully-connected head of the `_physics` / `_pairgraphs` models for a batch of feature rows x [n][width[0]]:
 *   h_i = LeakyReLU(W_i h_{i-1}) for i = 1..nLayers (W_i = [width[i]][width[i-1]], MatVecMul + LeakyReLU), y = <h_nLayers, w>,
 *   loss = (y - t)^2 / 2      (SMP_omega_physics.h:229-238, :592-606: one hidden layer of nTotal / 2;
 *                              SMP_omega_pairgraphs.h:330-345: two, max(nTotal / 2, 10) and max(that / 2, 10)).
 * params / dparams: W_1, ..., W_nLayers, w back to back (the models' registration order).  `work` holds the activations between
 * forward and backward: gf_head_work_floats floats.  backward: dx = gradient w.r.t. x, dparams += the weight gradients. */
size_t    gf_head_param_count(int nLayers, const int *width);
size_t    gf_head_work_floats(int nLayers, const int *width, int n);
gf_status gf_head_forward_f32(gf_ctx *ctx, int nLayers, const int *width, const float *x, int n, const float *params,
                              const float *targets, float *predict, float *loss, float *work);
gf_status gf_head_backward_f32(gf_ctx *ctx, int nLayers, const int *width, const float *x, int n, const float *params, float *work,
                               float *dx, float *dparams);
/* 1 (default): fused level kernels (no promoted stack, no 18-slice contraction output in HBM) where the shape allows;
 * 0: the op-by-op pipeline.  Same results within fp32 rounding; kept switchable for parity tests. */
gf_status gf_smp_set_fused(gf_smp *smp, int on);
/* The block products of one fused level at 64 channels as stand-alone operators on caller-supplied device matrices: the same
 * kernels gf_smp_forward / gf_smp_backward launch on a level's rows (the regrouped K-projection MatMul of GraphFlow/SMP_omega.h:654-657,
 * MatMul.h:48-82).  rows x 64-column blocks, row-major:  T = [S_ab|S_bc|T6|T10] (256 columns),  O / dO = [O_loc | U] (128),
 * rowscale [rows][2] = (tot, tr) of the row's node, trow [rows] = the row holding the transposed position (any permutation of the
 * rows; gf_smp_level_wgrad_f32 checks it on the host -- one blocking copy per call -- answers GF_ERR_INVALID for a row outside the
 * matrix, and serves a table that leaves the level's gather window of 64 x 64 rows, see below, while dO is smaller than 1 GiB),
 * Wst [8][64][64] = stacked weight blocks W0..W7:
 *   forward  (backward == 0):  O_loc = tot (S_ab W0 + S_bc W1) + tr S_ab W2 + T6 W3 + T10 W4,   U = S_ab W5 + S_bc W6 + S_ab[trow] W7
 *   backward (backward != 0):  dT from dO, the transposed products (dS_ab = tot L W0^T + tr L W2^T + dU W5^T + dU[trow] W7^T, ...)
 *   wgrad:  dWst[p] = sum over rows of (T block of p)^T (dO block of p, with the factor of p)
 * On the f16 matrix pipe with two-half fp32 operands by default, on the fp32 pipe with GF_SMP_SPLIT=0 (read per call). */
gf_status gf_smp_level_products_f32(gf_ctx *ctx, int backward, int rows, const float *A, const float *rowscale, const float *Wst,
                                    const int *trow, float *Out);
gf_status gf_smp_level_wgrad_f32(gf_ctx *ctx, int rows, const float *T, const float *dO, const float *rowscale, const int *trow,
                                 float *dWst);
/* The same products in every variant the fused level has: C = 128, 64, 32 or 16 channels (blocks of C columns: T [rows][4 C], O / dO
 * [rows][2 C], Wst [8][C][C]; forward A = T -> Out = O, backward A = dO -> Out = dT), with
 *   nf = 2: rowfac [rows][2] = (tot, tr) as above;   nf = 8 (C = 32, 16): rowfac [rows][8] = one factor per stacked product 0..7 --
 *           the plain (tot, tot, tr, 1, 1, 1, 1, 1) times the node's slice-dropout factors -- in place of tot / tr / 1 above.  The factors
 *           of a row and of its transposed row must agree in product 7 (they belong to one node);
 *   nx = 3 (C = 32, 16, nf = 2): three extra products with X [3][C][C] = (X_a, X_b, X_c), SMP_2D_ver7's:
 *           O_loc += S_ab X_a + S_bc X_b + tr S_bc X_c,  dS_ab += L X_a^T,  dS_bc += L X_b^T + tr L X_c^T,
 *           dX = (S_ab^T L, S_bc^T L, S_bc^T (tr L));   nx = 0: X / dX may be NULL;
 *   trowf (or NULL): the level's PACKED table.  The low 29 bits of an entry are trow; bit 31 = the row's S_ab / T6 blocks hold data,
 *           bit 30 = the S_ab block of the TRANSPOSED row does (= that row's bit 31), bit 29 = the row's S_bc / T10 blocks hold data.
 *           A block whose bit is clear is never read and counts as zero.  The product kernels take the table for levels of fewer
 *           than 2^29 rows, the weight gradients for fewer than 2^28, and neither with GF_SMP_MASK_ZEROS=0;
 *   skip_zero_grads (backward, with trowf): the dS_ab / dT6 blocks of rows without bit 31 are NOT written (gradients of structural
 *           zeros), and dO of a row without bit 29 (no source covers it: nothing to back-propagate) counts as zero.  This relies
 *           on the level's structure: bit 31 implies bit 29, and bit 29 is the same for a row and its transposed row.
 * C = 128 (nf = 2, nx = 0; trowf and skip_zero_grads as at 64): every 128 x 128 product runs as four 64 x 64 sub-block passes of the
 * C = 64 kernels -- (reduction half, output half); the second reduction half adds to the first in a fixed order, so two runs give the
 * same bits -- and a row's exponent is taken per 64-column sub-block.
 * The weight gradients exist at C = 128, 32 and 16, and at C = 64 WITH a packed table (trowf; nf = 2, nx = 0; not on the fp32 pipe) --
 * with the plain table alone gf_smp_level_wgrad_f32 is the C = 64 operator and this one answers GF_ERR_UNSUPPORTED; with nf = 2 the operand columns take
 * their exponents from exact column maxima, with nf = 8 from per-channel upper bounds the operator derives from the operands.
 * Their gathered operand dU[trow] is fetched through a window of 64 x 64 rows on either side of the row's 16-row slice -- in a
 * level a transposed row lies inside its own node, at most (s - 1)^2 rows away -- and a row further off would silently load zeros:
 * that is a property of the level, so this operator checks trow on the host (one blocking copy of the tables per call; both
 * operators also refuse a trow outside the matrix, and a trowf whose low bits differ from trow) and answers GF_ERR_INVALID.
 * Combinations the kernels do not have are GF_ERR_UNSUPPORTED before anything is launched: nx = 3 with nf = 8, nx = 3 or nf = 8
 * at C = 64 or 128, and C != 64 on the fp32 pipe (GF_SMP_SPLIT=0 / GF_OPT_SMP_FP32_PRODUCTS).  The context stays usable after a refusal. */
gf_status gf_smp_level_products_ex_f32(gf_ctx *ctx, int backward, int C, int nf, int nx, int rows, const float *A, const float *rowfac,
                                       const float *Wst, const float *X, const int *trow, const int *trowf, int skip_zero_grads,
                                       float *Out);
gf_status gf_smp_level_wgrad_ex_f32(gf_ctx *ctx, int C, int nf, int nx, int rows, const float *T, const float *dO, const float *rowfac,
                                    const int *trow, const int *trowf, float *dWst, float *dX);
/* The row classes of a level's packed table, as the backward products at C = 64 take them under skip_zero_grads (panels of 32 rows of
 * ONE class: rows whose S_ab / T6 blocks are structural zeros run three of the eight products; GF_SMP_ROW_CLASSES=0, read per call,
 * selects the unclassed kernel):
 * lists (device, 4 + 2 (rows + 64) + rows / 1024 + 2 ints) receives  [0] the number of rows with bit 31, [1] of rows without, and from
 * int 4 on entries (row, packed word): the rows with bit 31 in ascending order, padded to a multiple of 32 entries, then the rows
 * without, padded likewise.  A padding entry repeats the last row of its class with bit 31 of the row set.  The level builds this once
 * per gf_smp_prepare; gf_smp_level_products_ex_f32 builds it per call (the backward products under skip_zero_grads walk it).  rows < 2^29.  Asynchronous on the context's stream. */
gf_status gf_smp_level_row_classes(gf_ctx *ctx, int rows, const int *trowf, int *lists);
/* The same lists as a fused 64-channel level of a model keeps them (live_only != 0): a row with none of bits 31 / 30 / 29 of its packed
 * word -- an EMPTY row: no data in any block of T, its O is exact zeros and nothing reads its gradients -- goes into NEITHER list, and
 * [1] counts the rows without bit 31 that are left.  lists: 4 + 2 (rows + 64) + 2 (rows / 1024 + 2) ints.  live_only = 0:
 * gf_smp_level_row_classes. */
gf_status gf_smp_level_row_classes_ex(gf_ctx *ctx, int rows, const int *trowf, int *lists, int live_only);
/* SMP_2D_ver5's level (gf_smp_config.steerable_2d = 5), its channel projections and weight gradients as stand-alone operators: the
 * level's own kernels and launches on caller-supplied operands, for per-row tests (tests/test_smp_2d_ver5_ops_gpu.py).  Device
 * pointers, fp32, asynchronous on the context's stream.  C = 1 .. 128 channels; K [C][2 C] = [K1 | K2]; sizes: nsizes entries of 3 C
 * floats (lambda1_s | lambda2_s | b_s), entry s - 1 for a node of s positions; row_cs [rows][2] = (column of the row, s); col_s [cols].
 *   rows, backward = 0: out[row] = LeakyReLU_alpha((lambda1_s . X[row]) K1^T + u[column of the row]),  X, out [rows][C], u [cols][C];
 *         backward = 1: out[row] = X[row] K1  (sizes, u, row_cs, cols, nsizes are not read and may be NULL / 0).
 *         max_workgroups = 0: the level's grid (no more workgroups than the device holds at once, striding over the 32-row tiles);
 *         > 0: at most that many, so that a small input strides as a large one does.
 *   cols, backward = 0: out[j] = (lambda2_s . in[j]) K2^T + b_s;   backward = 1: out[j] = in[j] K2  (sizes, col_s not read).
 *         Rows of `in` are ldin >= C floats apart (the level's backward reads cz out of its 4 C-wide column partials), out [cols][C].
 *   wgrad: dK [C][2 C] += (sum_rows dz^T (lambda1_s . S) | sum_cols cz^T (lambda2_s . col)): dz, S [rows][C]; cz (rows ldcz >= C floats
 *         apart), col [cols][C]; per half one partial image per 512 rows, folded in a fixed order (the images live in the context's
 *         workspace).
 * GF_ERR_INVALID before anything is launched: C outside 1 .. 128, rows / cols < 1, ldin / ldcz < C, and -- checked on the host, one
 * blocking copy of the tables per call -- a size outside 1 .. nsizes or (rows forward, wgrad) a column outside [0, cols).  The context
 * stays usable after a refusal. */
gf_status gf_smp_2d_ver5_rows_ex_f32(gf_ctx *ctx, int backward, int C, int rows, int cols, int nsizes, const float *K, const float *X,
                                     const float *sizes, const float *u, const int *row_cs, float alpha, int max_workgroups, float *out);
gf_status gf_smp_2d_ver5_cols_ex_f32(gf_ctx *ctx, int backward, int C, int cols, int nsizes, const float *K, const float *in, int ldin,
                                     const float *sizes, const int *col_s, float *out);
gf_status gf_smp_2d_ver5_wgrad_ex_f32(gf_ctx *ctx, int C, int rows, int cols, int nsizes, const float *dz, const float *S, const int *row_cs,
                                      const float *cz, int ldcz, const float *col, const int *col_s, const float *sizes, float *dK);
/* The softmax neighbourhood level (gf_smp_config.neighbourhood = 1, 2, 3), its kernels as stand-alone operators: the level's own kernels
 * and launchers on caller-supplied operands, for per-row tests (tests/test_smp_neighbourhood_ops_gpu.py).  Device pointers, fp32,
 * asynchronous on the context's stream.  H = 1 .. 128 channels, nV vertices, pairs != 0: RisiLayer2D (form 3), else the sum.
 * Lists are CSR: ptr long long [nV + 1] from 0, idx int members in [0, nV).  rounds = 0: the level's own vertices per workgroup;
 * > 0: that many rounds of a workgroup's 256 / G vertex slots (G = 8, 16, 32, 64: the lane group of H).
 *   fwd:      h[v] = softmax(W1 x[v] + W2 n[v]), W1 [H][FD], x [nV][FD], W2 [H][H] (NULL: level 0, no aggregate, n / A / Tt untouched);
 *             n[v] = sum_u hprev[u] over ptr / idx, or with pairs A Tt - sum_u hprev[u] Tprev[u], A = sum_u hprev[u], Tt = sum_u Tprev[u];
 *             pairs also stores A [nV][H], Tt [nV] and T[v] = sum_k h[v][k] (T at level 0 too).
 *   node_bwd: dh[v] <- dz = d h (1 - h) in place, d = dh[v], or dy[vmol[v]] Wout when dy is not NULL (the top level; vmol in [0, nMol));
 *             with W2: dn[v] = W2^T dz, and with pairs gTt[v] = dn[v] Tt[v], sA[v] = <dn[v], A[v]>.  W2 NULL: level 0, dz alone.
 *   gather_bwd: dhprev[w] = sum of dn[v] over the consumers v of w (the transposed list tptr / tidx); pairs:
 *             sum_v gTt[v] - Tprev[w] sum_v dn[v] + sum_v sA[v] - <sum_v dn[v], hprev[w]>.
 *   readout:  g[m] = sum of hL[v] over mol_ptr[m] <= v < mol_ptr[m + 1] (int [nMol + 1], within the nV rows), yhat = <W, g>,
 *             dy = yhat - target (target NULL: 0), loss = 0.5 dy^2 (NULL: not stored); then dW[c] += sum_m dy[m] g[m][c].
 * GF_ERR_INVALID before anything is launched: H outside 1 .. 128, nV / nMol / FD < 1, rounds < 0, a missing operand of the chosen
 * form, more than 160 KiB of LDS for (H, FD), and -- checked on the host, one blocking copy of the tables per call -- a list that does
 * not start at 0 or decreases, a member outside [0, nV), vmol outside [0, nMol), a mol_ptr that decreases or leaves the nV rows.  The
 * context stays usable after a refusal. */
gf_status gf_smp_neighbourhood_fwd_ex_f32(gf_ctx *ctx, int pairs, int H, int FD, int nV, int rounds, const float *W1, const float *x, const float *W2,
                                          const float *hprev, const float *Tprev, const long long *ptr, const int *idx, float *h, float *n, float *A,
                                          float *T, float *Tt);
gf_status gf_smp_neighbourhood_node_bwd_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const float *W2, const float *h, float *dh,
                                               const float *dy, const float *Wout, const int *vmol, int nMol, const float *A, const float *Tt,
                                               float *dn, float *gTt, float *sA);
gf_status gf_smp_neighbourhood_gather_bwd_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, const long long *tptr, const int *tidx, const float *dn,
                                                 const float *gTt, const float *sA, const float *hprev, const float *Tprev, float *dhprev);
gf_status gf_smp_neighbourhood_readout_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, const float *hL, const int *mol_ptr, const float *W,
                                              const float *target, float *g, float *yhat, float *loss, float *dy, float *dW);
/* The gated level's kernels (GRU_GCN_1D, GRU_GCN_2D and GRU_GCN_3D's cell: smp_level_gru.hip) as stand-alone operators through the level's
 * own launchers, for tests/test_smp_gru_ops_gpu.py.  Device pointers, fp32, asynchronous on the context's stream.  H = 1 .. 64 channels,
 * nV vertices, lists and rounds as above.  M6 = W_z, U_z, W_r, U_r, W_h, U_h back to back, M2 = W_g, U_g, [H][H] each.
 *   cell_fwd: aggregate 0: n[v] = sum_u hprev[u] over ptr / idx; 1: the pair form A Tt - sum_u hprev[u] Tprev[u], which also stores
 *             A [nV][H], Tt [nV] and T[v] = sum_k h[v][k]; 2: n is an INPUT (GRU_GCN_3D), ptr / idx / Tprev / A / T / Tt may be NULL and
 *             stay untouched.  With hp = hprev[v]: z = sigmoid(W_z n + U_z hp), r = sigmoid(W_r n + U_r hp), c = tanh(W_h n + U_h (r hp)),
 *             h[v] = (1 - z) hp + z c; h, n, z, r, c [nV][H].
 *   cell_bwd: from dh and the stored z, r, c: dzp = dh (c - hp) z (1 - z), dcp = dh z (1 - c^2), dq = U_h^T dcp, drp = dq hp r (1 - r),
 *             q = r hp, dn = W_z^T dzp + W_r^T drp + W_h^T dcp, direct = dh (1 - z) + dq r + U_z^T dzp + U_r^T drp; with pairs also
 *             gTt[v] = dn[v] Tt[v] and sA[v] = <dn[v], A[v]>.  dh_{l-1} = gf_smp_neighbourhood_gather_bwd_ex_f32 of dn (, gTt, sA) + direct.
 *   readout_fwd: s = sigmoid(W_g hL[v]), t = tanh(U_g hL[v]) [nV][H]; g[m] = tanh(sum of s t over mol_ptr[m] <= v < mol_ptr[m + 1])
 *             (an empty molecule: 0), yhat = <U, g>, dy = yhat - target (target NULL: 0), loss = 0.5 dy^2 (NULL: not stored).
 *   readout_bwd: dU[c] += sum_m dy[m] g[m][c]; with dg = dy[vmol[v]] U (1 - g^2): ds = dg t s (1 - s), dt = dg s (1 - t^2),
 *             dh[v] = W_g^T ds + U_g^T dt.
 * GF_ERR_INVALID before anything is launched: H outside 1 .. 64, nV / nMol < 1, rounds < 0, aggregate outside 0 .. 2, a missing operand
 * of the chosen form, and -- one blocking copy of the tables per call -- a list that does not start at 0 or decreases, a member outside
 * [0, nV), vmol outside [0, nMol), a mol_ptr that decreases or leaves the nV rows.  The context stays usable after a refusal. */
gf_status gf_smp_gru_cell_fwd_ex_f32(gf_ctx *ctx, int aggregate, int H, int nV, int rounds, const float *M6, const float *hprev, const float *Tprev,
                                     const long long *ptr, const int *idx, float *h, float *n, float *z, float *r, float *c, float *A, float *T,
                                     float *Tt);
gf_status gf_smp_gru_cell_bwd_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const float *M6, const float *hprev, const float *dh,
                                     const float *z, const float *r, const float *c, const float *A, const float *Tt, float *dzp, float *drp,
                                     float *dcp, float *q, float *dn, float *gTt, float *sA, float *direct);
gf_status gf_smp_gru_readout_fwd_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, int rounds, const float *M2, const float *U, const float *hL,
                                        const int *mol_ptr, const float *target, float *s, float *t, float *g, float *yhat, float *loss,
                                        float *dy);
gf_status gf_smp_gru_readout_bwd_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, int rounds, const float *M2, const float *U, const float *s,
                                        const float *t, const float *g, const float *dy, const int *vmol, float *ds, float *dt, float *dh,
                                        float *dU);
/* The same three kernels on TWO operand sets in one launch each (gf_smp_config.distance_channel: the vertex and the distance channel
 * of a level; blockIdx.y picks the set).  pairs, H, nV, rounds and the lists are shared; a set is the single-channel call's operands, with
 * an operand width FD of its own in fwd.  W2 (fwd, node_bwd) must be NULL in both sets or in neither; dy / vmol / nMol are shared.  The
 * validation is that of the single-channel entries, applied to both sets; set 0 gives the bits of the single-channel call. */
typedef struct gf_nbh_fwd_set {
    int FD;
    const float *W1, *x, *W2, *hprev, *Tprev;
    float *h, *n, *A, *T, *Tt;
} gf_nbh_fwd_set;
typedef struct gf_nbh_node_set {
    const float *W2, *h;
    float *dh;
    const float *Wout, *A, *Tt;
    float *dn, *gTt, *sA;
} gf_nbh_node_set;
typedef struct gf_nbh_gather_set {
    const float *dn, *gTt, *sA, *hprev, *Tprev;
    float *dhprev;
} gf_nbh_gather_set;
gf_status gf_smp_neighbourhood_fwd2_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const gf_nbh_fwd_set *sets, const long long *ptr,
                                           const int *idx);
gf_status gf_smp_neighbourhood_node_bwd2_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const gf_nbh_node_set *sets, const float *dy,
                                                const int *vmol, int nMol);
gf_status gf_smp_neighbourhood_gather_bwd2_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, const long long *tptr, const int *tidx,
                                                  const gf_nbh_gather_set *sets);
/* The distance channel's input rows (gf_smp_config.distance_channel) as a stand-alone operator, for tests/test_smp_distance_ops_gpu.py.
 * Device pointers: mol_ptr int [nMol + 1] (prefix sums of the vertex counts, from 0), nVertices int [nMol], distance = the molecules' V x V
 * matrices of doubles back to back, x_d float [mol_ptr[nMol]][M].  x_d[v] = the ascending sort of (float) distance[u][j], u = 0 .. V - 1 --
 * COLUMN j = v - mol_ptr[m] of molecule m -- and M - V zeros.  GF_ERR_INVALID before anything is launched (one blocking copy of the
 * operands per call): nMol or M below 1, M above 4096, a missing operand, a mol_ptr that does not start at 0 or disagrees with nVertices,
 * a molecule with fewer than 1 or more than M vertices, an entry that is not finite.  Blocking.  The context stays usable. */
gf_status gf_smp_distance_rows_ex_f32(gf_ctx *ctx, int nMol, int M, const int *mol_ptr, const int *nVertices, const double *distance,
                                      float *x_d);
/* The two read-outs of gf_smp_config.readout as stand-alone operators on caller-supplied operands (smp_level_readouts.hip;
 * tests/test_pair_gram_ops_gpu.py).  Device pointers, fp32.  H = 1 .. 128 channels, nV rows of hL.  pair_readout validates with one blocking
 * copy and then launches asynchronously on the context's stream; gram_readout is BLOCKING: a test operator that allocates its table of
 * matrix offsets for the length of the call, waits for the stream and frees it.
 *   pair_readout: graph_ptr int [2 nPairs + 1] (prefix sums of the graphs' vertex counts X_0, Y_0, X_1, .., from 0, within the nV rows);
 *             g[p] = [sum of hL over X_p | over Y_p] [2 H] in ascending vertex order, yhat[p] = <W, g[p]> (W [2 H]), dy = yhat - target (target
 *             NULL: 0), loss = 0.5 dy^2 (NULL: not stored); dW[c] += sum_p dy[p] g[p][c], folded over the pairs in a fixed order; dhL[v][c] =
 *             dy[pair(v)] W[side(v) H + c] for every vertex of a graph (dhL NULL: not written).  A graph may be empty.
 *   gram_readout: mol_ptr int [nMol + 1]; adj = the molecules' V x V matrices as floats, row-major, back to back; gram the same shape:
 *             gram[x][y] = <hL[x], hL[y]>, loss[m] = 0.5 sum (gram - adj)^2 (NULL: not stored), dhL[x] = sum_y (E[x][y] + E[y][x]) hL[y] with
 *             E = gram - adj (dhL NULL: not written).  One workgroup per molecule; every molecule needs 4 (V (H | 1) + V (V | 1) + 4) bytes
 *             of LDS within 160 KiB.
 * GF_ERR_INVALID before anything is launched: H outside 1 .. 128, nV / nPairs / nMol < 1, a missing operand, and -- checked on the host, one
 * blocking copy per call -- a list that does not start at 0, decreases or leaves the nV rows, a molecule beyond the LDS bound (named).  The
 * context stays usable after a refusal. */
gf_status gf_smp_pair_readout_ex_f32(gf_ctx *ctx, int H, int nV, int nPairs, const float *hL, const int *graph_ptr, const float *W,
                                     const float *target, float *g, float *yhat, float *loss, float *dy, float *dW, float *dhL);
gf_status gf_smp_gram_readout_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, const float *hL, const int *mol_ptr, const float *adj, float *gram,
                                     float *loss, float *dhL);
/* The covariant vertex level (gf_smp_config.covariant = 1, 2: CGCN_1D, CGCN_2D), its two network kernels as stand-alone operators on
 * caller-supplied operands (tests/test_cgcn_ops_gpu.py).  Device pointers, fp32, asynchronous on the context's stream.  form = 1 (the sum
 * aggregate) or 2 (RisiLayer2D); L = 0 .. 64 levels; M = 1 .. 75, the length of a vertex's vector and the side of F_l; nV vertices in nMol
 * molecules, molecule m = the vertices mol_ptr[m] .. mol_ptr[m + 1] - 1 (int [nMol + 1]; at most M each; a molecule may be empty).
 *   nb_ptr long long [nV + 1], nb_idx int: the column neighbour lists N(v) as GLOBAL vertex ids of v's own molecule, strictly ascending
 *             (the order the aggregate adds them in); nb_tptr / nb_tidx: the transposed lists { v : u in N(v) }, likewise.
 *   hop       unsigned char [nV][M]: hop[v][i] = the hop count sp[i][v] of position i < V (255: unreachable); position i of vertex v is
 *             inside the mask of level l where hop[v][i] <= l.  Entries i >= V are not read.
 *   s0 [nV]   the level-0 scalars <x[v], H>;  F [L][M][M] the stacked F_l, row-major;  target [nMol] or NULL (0).
 * forward:  h [L + 1][nV][M] = every h_l[v], n [L][nV][M] = every n_l[v] (l = 1 .. L at index l - 1), positions >= V written as zeros;
 *           g [nMol][M] the graph features, yhat [nMol] their component sums, loss [nMol] = 0.5 (yhat - target)^2 (NULL: not stored),
 *           dy [nMol] = yhat - target (NULL: not stored).  One launch, one workgroup per molecule; every sum in a fixed order.
 * backward: from h, n and dy [nMol] of a forward: dF [L][M][M] += the gradients of the F_l, ds0 [nV] = the gradients of the level-0 scalars.
 *           One launch over min(nMol, 256) chunks of ceil(nMol / chunks) consecutive molecules and one fold of the chunks' partial images in
 *           ascending order (the context's workspace holds them); dh_{l-1} is gathered over the transposed lists.  No float atomics: two
 *           calls give the same bits.
 * GF_ERR_INVALID before anything is launched: form, L, M, nV or nMol out of range, a missing operand, and -- checked on the host, one
 * blocking copy per call -- a table that does not start at 0, decreases or leaves its range, a molecule above M vertices (named), a
 * list entry outside its vertex's molecule (named).  The context stays usable after a refusal. */
gf_status gf_smp_covariant_forward_ex_f32(gf_ctx *ctx, int form, int L, int M, int nV, int nMol, const int *mol_ptr, const long long *nb_ptr,
                                          const int *nb_idx, const unsigned char *hop, const float *s0, const float *F, const float *target,
                                          float *h, float *n, float *g, float *yhat, float *loss, float *dy);
gf_status gf_smp_covariant_backward_ex_f32(gf_ctx *ctx, int form, int L, int M, int nV, int nMol, const int *mol_ptr, const long long *nb_ptr,
                                           const int *nb_idx, const long long *nb_tptr, const int *nb_tidx, const unsigned char *hop,
                                           const float *F, const float *h, const float *n, const float *dy, float *dF, float *ds0);
/* The third-order pool (gf_smp_config.neighbourhood = 6, 7), its two kernels as stand-alone operators on caller-supplied operands, for
 * per-vertex tests (tests/test_smp_third_order_ops_gpu.py).  Device pointers, fp32, asynchronous on the context's stream.  H = 1 .. 64
 * channels, nV vertices; lists are CSR: ptr long long [nV + 1] from 0, idx int members in [0, nV), tptr / tidx the transposed list
 * (the consumers of a source, ascending).
 *   fwd: n[v] [H] = the H largest of T[x, y, z] over the members hprev[u], u in the list of v, counted with the multiplicity of their
 *        class, ascending; sel[v] [H] = the canonical triple per rank, x | y << 8 | z << 16 with x <= y <= z.  A list of fewer than three
 *        members gives n = 0 and sel = -1.
 *   bwd: dhprev[w] [H] = sum over the consumers v of w, ascending, and their ranks r with sel[v][r] = (x, y, z), g = dn[v][r], of
 *        g D_w(y, z) into channel x, g D_w(x, z) into y, g D_w(x, y) into z; D_w(p, q) = (A_p - a_w[p]) (A_q - a_w[q]) - (B_pq - a_w[p] a_w[q])
 *        with A, B of v's members (recomputed from ptr / idx and hprev).  A source without a consumer gets 0.
 * GF_ERR_INVALID before anything is launched: H outside 1 .. 64, nV < 1, a missing operand, and -- checked on the host, one blocking copy
 * per call -- a list that does not start at 0 or decreases, a member outside [0, nV), a list longer than the LDS plan takes (474 members
 * at 64 channels), a sel entry that is neither -1 nor a triple x <= y <= z < H.  The context stays usable after a refusal. */
gf_status gf_smp_third_order_pool_fwd_ex_f32(gf_ctx *ctx, int H, int nV, const long long *ptr, const int *idx, const float *hprev, float *n,
                                             int *sel);
gf_status gf_smp_third_order_pool_bwd_ex_f32(gf_ctx *ctx, int H, int nV, const long long *ptr, const int *idx, const long long *tptr,
                                             const int *tidx, const float *hprev, const int *sel, const float *dn, float *dhprev);
/* The row-list GEMM level (gf_smp_config.matrix_form = 1, 2), its two products as stand-alone operators on caller-supplied operands, for
 * per-row tests (tests/test_rowlist_ops_gpu.py).  Device pointers, fp32, asynchronous on the context's stream.  The operand is
 *   A[r][slot * Cin + c] = sum over the entries e of row r with that slot of coef[e] * X[src[e]][c],      r < R, slot < slots, c < Cin,
 * given as a CSR list: ptr long long [R + 1] from 0, and per entry src in [0, nX) (X is [nX][Cin]), slot in [0, slots), coef (NULL: every
 * coefficient is 1); the entries of a row in ascending slot order.  A row may have no entries, a slot any number of them.
 *   product: out [R][N] = act(A B + bias), act = 0: none, 1: LeakyReLU(0.01); bias [N] or NULL.  transposed_b = 0: B is [slots Cin][N];
 *            1: B is the matrix of the forward product this one is the backward-data of, [slots][N][Cin], read transposed slot by slot
 *            (element (slot Cin + a, n) = B[(slot N + n) Cin + a]; one slot: the plain transpose).
 *   wgrad:   dB [slots Cin][N] += A^T dOut (dOut [R][N]) as a split over row chunks folded in ascending order; db [N] += the column sums
 *            of dOut when db is not NULL.  Uses the context's workspace.
 * GF_ERR_INVALID before anything is launched: a shape below 1, slots Cin or N above 65536, a missing operand, and -- checked on the host,
 * one blocking copy per call -- a list that does not start at 0 or decreases, more than 2^31 - 1 entries, a source row outside [0, nX), a
 * slot outside [0, slots), slots that decrease inside a row.  The context stays usable after a refusal. */
gf_status gf_smp_rowlist_product_ex_f32(gf_ctx *ctx, int transposed_b, int R, int slots, int Cin, int N, int nX, const long long *ptr,
                                        const int *src, const int *slot, const float *coef, const float *X, const float *B, const float *bias,
                                        int act, float *out);
gf_status gf_smp_rowlist_wgrad_ex_f32(gf_ctx *ctx, int R, int slots, int Cin, int N, int nX, const long long *ptr, const int *src,
                                      const int *slot, const float *coef, const float *X, const float *dOut, float *dB, float *db);
/* Host only (no device): what gf_smp_prepare derives from ONE molecule of a matrix_form configuration.  LCNN: order [V] and sequence
 * [V][nNeighbors] with V = max_nVertices (norm_adj is not written); GCN_MW: norm_adj = A-hat [V][V] in double (order, sequence are not
 * written).  GF_ERR_INVALID: a configuration gf_smp_create refuses, V outside 1 .. max_nVertices, a missing output, and an LCNN molecule
 * with V == max_nVertices one of whose vertices reaches fewer than nNeighbors vertices (see gf_smp_config.matrix_form). */
gf_status gf_smp_matrix_form_molecule_host(const gf_smp_config *cfg, int V, const int *adj, const double *feature, int *order, int *sequence,
                                           double *norm_adj);
/* Host only: one molecule of a covariant configuration (covariant = 1, 2) as gf_smp_prepare derives it.  lists int [V][M + 1], M =
 * max_nVertices: slot 0 = the size of N(v) = { u : adj[u][v] > 0 }, then its members in ascending order, -1 behind them; hop unsigned
 * char [V][M]: hop[v][i] = the hop count sp[i][v] (255: unreachable, or i beyond the molecule) -- position i of vertex v is inside the mask
 * of level l where hop[v][i] <= l; x (optional) double [V][nFeatures (nDepth + 1)], the shell sums.  GF_ERR_INVALID: a configuration
 * gf_smp_create would refuse (its message), covariant = 0, V outside 1 .. max_nVertices, a missing argument. */
gf_status gf_smp_covariant_molecule_host(const gf_smp_config *cfg, int V, const int *adj, const double *feature, int *lists, unsigned char *hop,
                                         double *x);
/* Device memory of the handle's buffer pool: bytes held by the current batch, and bytes the pool keeps in total (idle
 * blocks included).  Sizing aid for batch selection (GraphFlow has no counterpart: its tensors live in host `new[]`). */
gf_status gf_smp_device_bytes(const gf_smp *smp, size_t *in_use, size_t *reserved);
/* Introspection for tests: launches so far of the kernels a fused level takes when all its sources are single vertices (level 1 of
 * SMP_omega at 64 / 32 / 16 channels: one per size class in tables-forward, one in the backward gather); they run under the general
 * kernels' launch names.  GF_SMP_LEVEL1=0 keeps it where it is.  0 for a null handle. */
long long gf_smp_single_vertex_launches(const gf_smp *smp);
/* Introspection for tests: level passes so far, forward or backward, in which a fused 64-channel level neither stored nor read the
 * projected matrix O / dO of its empty rows (rows (a, b) with no data in any table block: no source covers them).  One per level and
 * direction where the call's kernels all mask those rows; GF_SMP_EMPTY_ROWS=0 (read per call) keeps it where it is.  0 for a null handle. */
long long gf_smp_empty_row_calls(const gf_smp *smp);
/* ... and the level's projected matrix as the last pass left it -- O = [O_loc | U] after a forward, dO = [dz | dU] after a backward of
 * the level -- copied to `out` (device, [rows][2 C] floats), asynchronously on the context's stream.  GF_ERR_INVALID unless the level's
 * last forward ran fused on the row-panel kernels (the compact layout) at the caller's own channel count (no padding). */
gf_status gf_smp_level_projected_f32(gf_smp *smp, int level, float *out);
/* Host-pointer mode of the driver (what graphflow_amd/host/SMP_omega_hip.h uses): the handle owns the model -- a device
 * parameter buffer and its gradient.  Wherever the entry points of this section take `params` / `grads`, NULL selects the
 * handle-owned buffers.  gf_smp_forward_host runs gf_smp_forward on them and returns per-molecule results as doubles
 * (targets NULL: predict / Feature only; loss is 0.5 (y - t)^2 per molecule, SquaredLoss.h:45-53).  Blocking. */
gf_status gf_smp_parameters_upload(gf_smp *smp, const float *host_params);
gf_status gf_smp_parameters_download(gf_smp *smp, float *host_params, float *host_grads);
gf_status gf_smp_forward_host(gf_smp *smp, const double *targets, double *predict, double *loss, double *graph_feature);
/* Optimiser step of SMP_omega::BatchLearn (GraphFlow/SMP_omega.h:820-821 -> Adam::Learn(alpha, nBatch), Adam.h:106-133,
 * including its per-element advance of the bias-correction powers): params -= ..., from grads = the batch SUM written by
 * gf_smp_backward (all-reduced over ranks first in data-parallel runs; nBatch is then the GLOBAL batch).  The moment
 * buffers live in the handle and survive gf_smp_prepare.  Device pointers. */
gf_status gf_smp_adam_step(gf_smp *smp, float *params, const float *grads, double learning_rate, int nBatch);
gf_status gf_smp_adam_reset(gf_smp *smp);   /* zeroes the moment buffers (Adam and Momentum) and Adam's element counter */
/* Momentum::Learn(learning_rate, nBatch) (GraphFlow/Momentum.h:64-71), the optimiser of SMP_2D_ver6-8
 * (SMP_2D_ver6.h:204, :593): m = gamma m + learning_rate * grads / nBatch, params -= m. */
gf_status gf_smp_momentum_step(gf_smp *smp, float *params, const float *grads, double learning_rate, int nBatch, double gamma);
/* sgd->Learn(learning_rate, nBatch) for any of the reference's five optimisers over the same flat vector -- what a reference user gets by
 * changing the type of the model's `sgd` member.  All arithmetic in double on fp32 storage, each expression in the reference's order
 * (g = gradient / nBatch is a division); a state value the reference reads back after storing it is read back as stored (fp32).
 *   kind 0  Adam       gf_smp_adam_step's launch, bit for bit
 *   kind 1  Momentum   gf_smp_momentum_step's launch, bit for bit (gamma)
 *   kind 2  SGD        SGD::Learn(lr, nBatch), SGD.h:44-50: p -= lr * g / nBatch.  No state.
 *   kind 3  AdaMax     AdaMax::Learn(alpha, nBatch), AdaMax.h:97-122: beta1_t *= beta1 once per call (a host double in the handle); per
 *                      registered block b (gf_smp_config_param_blocks): first_order = beta1 first_order + (1 - beta1) g, infinity_norm[b] =
 *                      max(beta2 infinity_norm[b], max_j |g_j|), p -= alpha / (1 - beta1_t) * first_order / infinity_norm[b].
 *                      A block whose gradient is all zero while its norm is still 0 divides 0 by 0 in the reference, and here: the
 *                      block's parameters become NaN (and stay NaN); no other block is touched.  Per-size blocks of sizes a batch never
 *                      shows hit it -- in the class as well.
 *   kind 4  AdaDelta   AdaDelta::Learn(alpha, nBatch), AdaDelta.h:90-112: E[g^2], E[dx^2] per element; learning_rate is not read.
 * nBatch = 1 is Learn(alpha) for kinds 2 to 4 (the overloads differ by a division by 1).  The two fp32 state buffers are the ones Adam and
 * Momentum use, so the handle remembers the kind of its last step (the older step calls and gf_smp_fit record theirs and never refuse):
 * a different kind here is GF_ERR_INVALID until gf_smp_adam_reset, which also clears AdaMax's norms and beta1_t.  NULL cfg, a kind
 * outside 0 .. 4 and nBatch <= 0 are GF_ERR_INVALID. */
typedef struct {
    int kind;              /* 0 Adam, 1 Momentum, 2 SGD, 3 AdaMax, 4 AdaDelta: gf_smp_fit_config.optimiser's numbering */
    int nBatch;
    double learning_rate;
    double gamma;          /* Momentum */
    double beta1, beta2;   /* AdaMax; 0, 0 = 0.9, 0.999 (AdaMax.h:26-29) */
    double rho, epsilon;   /* AdaDelta; 0, 0 = 0.95, 1e-6 (AdaDelta.h:26-28) */
} gf_optim_config;
gf_status gf_smp_optimiser_step(gf_smp *smp, float *params, const float *grads, const gf_optim_config *cfg);
/* L1Regularization (L1Regularization.h:39-67; sign() is 0 for |p| < 1e-8) and L2Regularization (L2Regularization.h:39-58) over every
 * registered parameter: *value_host = lambda * sum |p| (norm 1) or lambda * sum p^2 (norm 2), summed in double in a fixed two-stage shape
 * (the same bits on every run), and grads[i] += times * (lambda sign(p_i) | 2 lambda p_i): `times` = how often the class's backward()
 * would have run since the gradient was last zeroed, the batch size for a BatchLearn step.  Blocking.  The fit loops do not regularise. */
gf_status gf_smp_regularise(gf_smp *smp, const float *params, float *grads, int norm, double lambda, int times, double *value_host);
/* The classes' CacheParameters (GraphFlow/CacheParameters.h:45-59): a device-to-device copy of the flat parameter buffer into
 * (snapshot) or out of (rollback) a cache the handle owns, allocated by the first snapshot.  params NULL: the handle-owned model.
 * Values only -- Momentum's velocity, Adam's moments and its element counter stay as they are, as in the classes.  Rollback before any
 * snapshot of the handle is GF_ERR_INVALID.  Asynchronous on the context's stream. */
gf_status gf_smp_parameters_snapshot(gf_smp *smp, const float *params);
gf_status gf_smp_parameters_rollback(gf_smp *smp, float *params);
/* gf_smp_forward_host for EVERY handle kind but a physics tower: the arrays are per sample -- a pair for readout = 1, a molecule
 * otherwise -- and a feature row is gf_smp_feature_width wide (2 nChanels for the pair and distance handles, max_nVertices for the
 * covariant ones).  A Gram handle (readout = 2) takes NULL targets, predict and graph_feature and returns the per-molecule loss.
 * gf_smp_forward_host itself keeps its refusals.  Blocking. */
gf_status gf_smp_forward_host_samples(gf_smp *smp, const double *targets, double *predict, double *loss, double *graph_feature);
/* gf_smp_gram to a HOST array of doubles (the molecules back to back, V_m^2 values each).  Blocking. */
gf_status gf_smp_gram_host(gf_smp *smp, double *out);
/* The iterative training calls every model class of the reference has, on the prepared batch:
 *   kind 0  BatchLearn(nBatch, molecule, target, nIterations, learning_rate, epsilon)      (GraphFlow/SMP_omega.h:827-874, GCN_1D.h:347-392)
 *           cache; first = second = loss; per iteration: reverse sweep, Learn(lr, nBatch), loss; loss > second: restore, lr *= 0.5,
 *           leave when lr < 1e-6; else second = loss, cache.  epsilon is not read.
 *   kind 1  Learn(molecule, target, nIterations, learning_rate, epsilon)                   (SMP_omega.h:876-922, GCN_1D.h:394-438)
 *           a batch of ONE sample (else GF_ERR_INVALID); first loss < epsilon: return (loss, loss) at once; per iteration: reverse sweep,
 *           Learn(lr) -- for Adam the overload that advances the bias-correction powers once per CALL (Adam.h:77-105), not per element --,
 *           error; error < epsilon: leave (the step stays); error >= best: restore, lr = max(0.5 lr, 1e-6); else best = error, cache.
 * "loss" is the sum of the per-sample losses of a forward, added in double in ascending sample order on the device and read back (8
 * bytes, one blocking copy per iteration); a classifier's is its LogLoss value (at most 0) under the same comparisons, as in the
 * reference.  lr and every comparison live on the host in double (graphflow_amd/csrc/smp_fit_policy.h).  The passes are gf_smp_forward
 * / gf_smp_backward / gf_smp_adam_step / gf_smp_momentum_step, in the order a caller would issue them; after a restore the loop runs a
 * forward before the next reverse sweep (and before it returns), so the handle is left forwarded at the parameters it is left with. */
typedef struct {
    int kind;        /* 0: the BatchLearn overload, 1: Learn */
    int optimiser;   /* 0: Adam, 1: Momentum with `gamma`, 2: SGD, 3: AdaMax, 4: AdaDelta (the classes' default constants) */
    int nIterations;
    double learning_rate, epsilon, gamma;
} gf_smp_fit_config;
typedef struct {
    double first, second;   /* the pair the class returns */
    int iterations, accepted, rejected;   /* iterations run; steps kept; steps restored */
    int left_early;         /* a break (kind 0: lr < 1e-6, kind 1: error < epsilon) or kind 1's immediate return */
    double learning_rate;   /* the rate the loop ended with */
} gf_smp_fit_report;
/* params / grads: device pointers, or both NULL for the handle-owned model; targets: device, one per sample (NULL on a Gram handle);
 * decisions (optional, host, nIterations bytes): per iteration run 1 = kept, 2 = restored, 3 = restored and left (kind 0),
 * 4 = left on error < epsilon (kind 1).  gf_smp_fit_host: the handle-owned model with host targets.  Blocking. */
gf_status gf_smp_fit(gf_smp *smp, float *params, float *grads, const float *targets, const gf_smp_fit_config *cfg,
                     gf_smp_fit_report *report, unsigned char *decisions);
gf_status gf_smp_fit_host(gf_smp *smp, const double *targets, const gf_smp_fit_config *cfg, gf_smp_fit_report *report,
                          unsigned char *decisions);
/* The loop's loss sum as a stand-alone operator, for tests/test_fit_gpu.py: *sum (host) = the n device floats of `loss` added as doubles
 * in ascending order -- the bits of a host loop `total += loss[i]` -- by the loop's own kernel.  1 <= n < 2^31.  Blocking. */
gf_status gf_smp_loss_sum_f32(gf_ctx *ctx, const float *loss, size_t n, double *sum);
/* SMP_omega::weights_initialization (SMP_omega.h:334-338; GraphFlow.h:1297-1306) into a HOST buffer of
 * gf_smp_param_count floats, drawing from rand() in the reference's order: same srand() -> same initial weights. */
gf_status gf_smp_uniform_init_host(const gf_smp_config *cfg, float *params);
/* ... of a classifier (SMP_2D_ver6_classification.h:256-259): sgd->params holds Vector*, so W[nClass][C] is drawn by
 * uniform_init(Vector*) with the divisor 10 * nClass * C.  Host only. */
gf_status gf_smp_classifier_uniform_init_host(const gf_smp_config *cfg, int nClass, float *params);
/* Text checkpoints interchangeable with SMP_omega::save_model / load_model (GraphFlow/SMP_omega.h:1033-1055):
 * whitespace-separated values in the flat parameter order above.  `params` is a device pointer.  Blocking. */
gf_status gf_smp_save_model(const gf_smp *smp, const float *params, const char *path);
gf_status gf_smp_load_model(gf_smp *smp, float *params, const char *path);
gf_status gf_smp_prepare_molecule_host(const gf_smp_config *cfg, int V, const int *adj, const double *feature,
                                       int *phi_out, double *wl_out);  /* host only; phi_out [L+1][V][cap+1], slot 0 = size */
int       gf_smp_receptive_field(const gf_smp *smp, int mol, int level, int v, int *out, int capacity);
/* Introspection for parity checks against the reference's per-level state: f_l[v] of molecule `mol` as [s][s][C] floats
 * (level[l]->f[v]->value after forward(), SMP_omega.h:667-669) and its reduced adjacency [s][s] (level[l]->adj[v], :556-581),
 * copied to HOST buffers.  Return the element count, or -1 (bad argument, capacity too small, nothing forwarded).  Blocking. */
long long gf_smp_read_activation(gf_smp *smp, int mol, int level, int v, float *host_out, size_t capacity);
long long gf_smp_read_reduced_adjacency(gf_smp *smp, int mol, int level, int v, float *host_out, size_t capacity);
gf_status gf_smp_level_sizes(const gf_smp *smp, int level, long long *nodes, long long *rows, long long *ppos);
/* sum of the receptive-field sizes s over the level's nodes: the (node, neighbour) pairs = promoted tensors of the level
 * (SMP_omega.h:641-647), and the rows of the per-(node, x) tables of the fused level; -1 on a bad argument */
long long gf_smp_level_pairs(const gf_smp *smp, int level);
/* Rows (a, b) of the level whose promoted slab row is not structurally zero -- vertex b lies inside the receptive field of a's
 * source (the selection matrices of SMP_omega.h:461-474 have a 1 in that column) -- out of gf_smp_level_sizes' `rows`.  The fused
 * level neither writes, reads nor back-propagates the other rows' S_ab / T6 table blocks; the bench prices its kernels with it. */
long long gf_smp_level_present_rows(const gf_smp *smp, int level);
/* ... and the rows (b, c) that SOME source covers (both vertices inside one source's field): the others' S_bc / T10 blocks are
 * structural zeros as well.  Equal to `rows` where the handle keeps no row flags (the flags exist for the channel counts the
 * row-panel kernels serve: models computed at 32 or 64 channels, i.e. every nChanels <= 64 through gf_smp_create's padding).
 * Both calls are introspection for tests and the bench: the first call after a prepare blocks on a device-to-host copy (the
 * result is then cached until the next prepare), and neither may run concurrently with gf_smp_prepare / gf_smp_destroy on the
 * SAME handle (they read the tables prepare replaces).  Other handles of the context are unaffected. */
long long gf_smp_level_covered_rows(const gf_smp *smp, int level);

/* RisiContraction_18_dropout inside a physics tower (SMP_sigma_pairgraphs.h:248-265, :632-651): masks[(l-1) * nVertices + gv] =
 * kept-slice bits of the contraction of global vertex gv (molecules back to back) at level l, drawn by the caller in the
 * reference's order (gf_smp_model_forward does); scale 1 in train mode, nKept / 18 with every bit set in test mode.  NULL: off. */
gf_status gf_smp_dropout_masks(gf_smp *smp, const unsigned *masks, float scale);
/* Adam::Learn(learning_rate, nBatch) (GraphFlow/Adam.h:106-133) on any flat device buffer with caller-owned moment buffers;
 * element i uses the bias-correction powers beta^(elements_before + i + 1), as the reference's per-element advance gives. */
gf_status gf_adam_step_f32(gf_ctx *ctx, float *params, const float *grads, float *m, float *v, size_t n, double learning_rate,
                           int nBatch, unsigned long long elements_before);
/* gf_smp_optimiser_step's kinds 2 to 4 on any flat device buffer with caller-owned state (other kinds: GF_ERR_INVALID).  state0 / state1
 * (device, n floats): AdaMax's first_order / unused, AdaDelta's E[g^2] / E[dx^2]; SGD reads neither.  AdaMax also takes its blocks --
 * block_offsets_host: nBlocks + 1 strictly ascending offsets from 0 to n, on the HOST --, block_norms (device, nBlocks doubles:
 * infinity_norm) and *beta1_t_inout (host; 1.0 before the first step), which the call advances. */
gf_status gf_optimiser_step_f32(gf_ctx *ctx, const gf_optim_config *cfg, float *params, const float *grads, size_t n,
                                const size_t *block_offsets_host, int nBlocks, float *state0, float *state1, double *block_norms,
                                double *beta1_t_inout);
/* gf_smp_regularise on any flat device buffers.  norm 1 | 2, times >= 0.  Blocking. */
gf_status gf_regularise_f32(gf_ctx *ctx, const float *params, float *grads, size_t n, int norm, double lambda, int times,
                            double *value_host);

/* ---- the `_physics` / `_pairgraphs` models as one handle ------------------------------------------------------
 * nTowers 1: SMP_omega_physics (GraphFlow/SMP_omega_physics.h:29-606) -- SMP_beta_physics with max_receptive_field =
 *            max_nVertices; head = one hidden layer of nTotal / 2 units (:229-238).
 * nTowers 2: SMP_omega_pairgraphs / SMP_beta_pairgraphs (GraphFlow/SMP_omega_pairgraphs.h:81-730): a graph and its partner (e.g.
 *            its line graph) through two towers with their own weights, level features concatenated level by level (:699-704),
 *            head = two hidden layers (:330-345).  nKept > 0: SMP_sigma_pairgraphs (RisiContraction_18_dropout keeping nKept
 *            slices; masks drawn with rand() in the reference's order in train mode, all slices x nKept / 18 in test mode).
 * params / grads: flat device buffers in the class's registration order -- physics H, (K_l, b_l)..., W1, W2 (:254-262);
 * pairgraphs H_1, H_2, (K1_l, b1_l, K2_l, b2_l)..., W1, W2, W3 (SMP_omega_pairgraphs.h:361-375).  grads = the batch SUM.
 * prepare: host pointers as gf_smp_prepare, one set per tower (the second set NULL for nTowers 1).
 * nContractions = 4: SMP_gamma_physics / SMP_gamma_pairgraphs (GraphFlow/SMP_gamma_physics.h, SMP_gamma_pairgraphs.h): the same
 *            models with RisiContraction_4 and K_l = [4 C_{l-1}][C_l]; receptive fields, halving channels, read-out of every level,
 *            heads, registration order and weights_initialization unchanged (use_coulomb is inert in the reference: nothing to pass).
 *            The towers compute at their own widths, on the rectangular gamma level of smp_level_gamma.hip where every width is at
 *            most 64 channels and every field at most 64 positions (otherwise, and under gf_smp_model_set_fused(0), op by op).
 *            0 (or an aggregate initialiser that stops before the field) means 18; other values, and nKept > 0 with 4, are refused. */
typedef struct gf_smp_model gf_smp_model;
typedef struct {
    int nTowers, nLevels, nChanels, max_receptive_field;
    int nFeatures[2];
    int nKept;   /* 0: RisiContraction_18; 1..18: RisiContraction_18_dropout */
    int nContractions;   /* 0 or 18: the `_omega` / `_beta` / `_sigma` models; 4: the `_gamma` ones */
    /* first_order = 1: SMP_theta_physics (nTowers 1) / SMP_theta_pairgraphs (nTowers 2) -- towers of gf_smp_config.first_order levels,
     * K_l = [2 C_{l-1}][C_l], per-size (lambda1, lambda2, b) blocks of max_nVertices entries in front of every K_l; heads, feature rows and
     * the interleaving of two towers' parameters as in the other models.  max_nVertices is per tower (SMP_theta_pairgraphs.h:31:
     * max_nVertices_1 / _2; [1] = 0 means [0]).  nContractions and nKept must be 0.  Zero: the models above. */
    int first_order, max_nVertices[2];
    /* ccn_1d = 1: CCN_1D (GraphFlow/CCN_1D.h), the first-order covariant compositional network on a pair of graphs: SMP_theta_pairgraphs with
     *   - the widths C_0 = nChanels, C_l = max(int(ceil(C_{l-1} * nChanels_decay)), 16) in both towers (the product in double, :200, :217),
     *   - the head nTotal -> max(int(ceil(nTotal * decay)), 16) -> max(int(ceil(that * decay)), 16) -> 1 (:352-353),
     *   - every vertex's feature row divided by its L1 norm before level 0 (:439-448); gf_smp_model_prepare does it on the host and refuses
     *     a row of zeros (0 / 0 in the class) with GF_ERR_INVALID, naming sample, tower and vertex.
     * Fields, cap, children, per-size blocks, read-out, registration order (H_1, H_2; per level tower 1's max_nVertices[0] size entries and
     * K1_l, then tower 2's; W1, W2, W3), weights_initialization, Adam and the multiplicity of dlambda are SMP_theta_pairgraphs'.
     * Required, else GF_ERR_INVALID before anything is allocated: nTowers = 2, first_order = 1, nKept = nContractions = 0, nChanels >= 16,
     * 0 < nChanels_decay <= 1, max_receptive_field <= both max_nVertices.  Zero (an initialiser that stops before the fields): the models
     * above, nChanels_decay is not read. */
    int ccn_1d;
    double nChanels_decay;
} gf_smp_model_config;
gf_status gf_smp_model_create(gf_ctx *ctx, const gf_smp_model_config *cfg, gf_smp_model **out);
/* host only: the parameter count gf_smp_model_create gives the configuration, 0 for one it refuses */
size_t    gf_smp_model_config_param_count(const gf_smp_model_config *cfg);
/* gf_smp_config_param_blocks for a composite model: H of every tower; per level, tower by tower, the level's blocks; the head's W1, W2
 * (, W3) (SMP_omega_pairgraphs.h:361-375, CCN_1D.h:381-403).  Host only. */
size_t    gf_smp_model_config_param_blocks(const gf_smp_model_config *cfg, size_t *offsets, size_t capacity);
gf_status gf_smp_model_destroy(gf_smp_model *model);
size_t    gf_smp_model_param_count(const gf_smp_model *model);
gf_status gf_smp_model_set_mode(gf_smp_model *model, int train);   /* SMP_sigma_pairgraphs::setMode (:139-149); default train */
/* gf_smp_set_fused on every tower (1, the default: the fused levels where the shape allows; 0: op by op) */
gf_status gf_smp_model_set_fused(gf_smp_model *model, int on);
gf_status gf_smp_model_prepare(gf_smp_model *model, int nMol, const int *nVertices1, const int *adj1, const double *feature1,
                               const int *nVertices2, const int *adj2, const double *feature2);
gf_status gf_smp_model_forward(gf_smp_model *model, const float *params, const float *targets, float *predict, float *loss);
gf_status gf_smp_model_backward(gf_smp_model *model, const float *params, float *grads, int accumulate);
gf_status gf_smp_model_uniform_init_host(const gf_smp_model *model, float *host_params);
/* host-pointer mode (graphflow_amd/host/SMP_physics_hip.h): the handle owns parameters, gradients and Adam moments; NULL
 * params / grads in the two calls above select them */
gf_status gf_smp_model_parameters_upload(gf_smp_model *model, const float *host_params);
gf_status gf_smp_model_parameters_download(gf_smp_model *model, float *host_params, float *host_grads);
gf_status gf_smp_model_forward_host(gf_smp_model *model, const double *targets, double *predict, double *loss);
gf_status gf_smp_model_adam_step(gf_smp_model *model, double learning_rate, int nBatch);
/* gf_smp_optimiser_step / gf_smp_regularise on the composite handle's flat vector (NULL params / grads: the handle-owned model).  Kind 0
 * leaves the bits of gf_smp_model_adam_step; kind 1 (Momentum) is available here although no composite class uses it.  The composite
 * handle has no reset call: it keeps the kind of its first step. */
gf_status gf_smp_model_optimiser_step(gf_smp_model *model, float *params, const float *grads, const gf_optim_config *cfg);
gf_status gf_smp_model_regularise(gf_smp_model *model, const float *params, float *grads, int norm, double lambda, int times,
                                  double *value_host);
/* gf_smp_parameters_snapshot / _rollback and gf_smp_fit / gf_smp_fit_host for the composite handle, over the whole registration-order
 * vector.  The composite classes train with Adam: optimiser = 1 is GF_ERR_UNSUPPORTED (2, 3 and 4 are accepted).  With device pointers the Adam moments are the
 * handle's (those of gf_smp_model_adam_step). */
gf_status gf_smp_model_parameters_snapshot(gf_smp_model *model, const float *params);
gf_status gf_smp_model_parameters_rollback(gf_smp_model *model, float *params);
gf_status gf_smp_model_fit(gf_smp_model *model, float *params, float *grads, const float *targets, const gf_smp_fit_config *cfg,
                           gf_smp_fit_report *report, unsigned char *decisions);
gf_status gf_smp_model_fit_host(gf_smp_model *model, const double *targets, const gf_smp_fit_config *cfg, gf_smp_fit_report *report,
                                unsigned char *decisions);

#ifdef __cplusplus
}
#endif
#endif /* GF_HIP_H_INCLUDED */
