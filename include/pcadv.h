/*
 * pcadv — MI355X-native (gfx950) PointNet adversarial-training hot path.
 *
 * C ABI of libpcadv.so.  Plain pointers and sizes only: every pointer is HIP
 * device memory owned by the caller (the library never allocates, frees or
 * retains a pointer past the call), every call is enqueued on `stream` without
 * a host sync and is safe to capture into a hipGraph.  Return value: PCADV_OK
 * or a negative error code; pcadv_last_error() then describes it
 * (thread-local).  No C++ exception crosses this boundary.
 *
 * Reference interfaces replaced (paths relative to the reference repo root,
 * YiruS/Adversarial_Learning_on_PointClouds):
 *   pcadv_feat_fwd / pcadv_feat_bwd  <- PointNetfeat.forward + autograd
 *                                       (models/pointnet.py:81-137; called from
 *                                        PointNetCls.forward :197-203)
 *   pcadv_conv_max_fwd               <- Conv1d(128->1024,1) + torch.max(dim=2)
 *                                       (models/pointnet.py:89,128-130; STN3d/STNkd
 *                                        :19,30-31 with relu before the max)
 *   pcadv_linear_fwd / _bwd          <- nn.Linear / 1x1 Conv1d on Bx Cx1 with
 *                                       ReLU / LeakyReLU(0.2) / Dropout
 *                                       (models/pointnet.py:191-202,
 *                                        models/discriminator.py:30-51)
 *   pcadv_adam                       <- torch.optim.Adam step
 *                                       (train_classification.py:110-122,
 *                                        utils/trainer.py:558-559)
 *   pcadv_gemm / _gemm_wgrad / _colsum / _conv_max_x3 / _row_ce
 *                                    <- PointNetSeg.forward + autograd + the
 *                                       per-point CrossEntropyLoss
 *                                       (models/pointnet.py:261-317,
 *                                        utils/trainer.py:310-400)
 *   pcadv_adv_step                   <- one iteration of utils/trainer.py:run_training
 *                                       (:426-559) incl. the losses of
 *                                       train_classification.py:199-200 and
 *                                       make_D_label (utils/utils.py:22-31)
 *
 * Layouts: point clouds are B x N x 3 f32 exactly as PointNetCls receives them
 * (no transpose copy); activations are point-major [cloud][point][channel];
 * weights are the reference's [out][in] (Conv1d [out,in,1] reinterpreted).
 * Parameters of the fused step live in one flat f32 buffer per network in
 * state_dict order (offsets below).
 */
#ifndef PCADV_H
#define PCADV_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCADV_OK 0
#define PCADV_EINVAL (-1)
#define PCADV_EHIP (-2)

#define PCADV_ACT_NONE 0
#define PCADV_ACT_RELU 1
#define PCADV_ACT_LRELU 2 /* LeakyReLU(negative_slope=0.2), discriminator.py:39 */

/* channel widths of the cls generator (models/pointnet.py:86-89,191-193) */
#define PCADV_C1 64
#define PCADV_C2 64
#define PCADV_C3 128
#define PCADV_C4 1024

/* flat parameter layout of PointNetCls(k=40) in state_dict order */
enum {
  PCADV_G_CONV1_W = 0, PCADV_G_CONV1_B = 192,
  PCADV_G_CONV2_W = 256, PCADV_G_CONV2_B = 4352,
  PCADV_G_CONV3_W = 4416, PCADV_G_CONV3_B = 12608,
  PCADV_G_CONV4_W = 12736, PCADV_G_CONV4_B = 143808,
  PCADV_G_FC1_W = 144832, PCADV_G_FC1_B = 669120,
  PCADV_G_FC2_W = 669632, PCADV_G_FC2_B = 800704,
  PCADV_G_FC3_W = 800960, PCADV_G_FC3_B = 811200,
  PCADV_G_NUMEL = 811240
};
/* flat parameter layout of DeepConvDiscNet(40, 1) in state_dict order */
enum {
  PCADV_D_CONV1_W = 0, PCADV_D_CONV1_B = 20480,
  PCADV_D_CONV2_W = 20992, PCADV_D_CONV2_B = 152064,
  PCADV_D_CONV3_W = 152320, PCADV_D_CONV3_B = 217856,
  PCADV_D_CONV4_W = 218112, PCADV_D_CONV4_B = 234496,
  PCADV_D_CONV5_W = 234560, PCADV_D_CONV5_B = 238656,
  PCADV_D_FC_W = 238720, PCADV_D_FC_B = 238784,
  PCADV_D_NUMEL = 238785
};

const char* pcadv_last_error(void);
/* 11: pcadv_split_bf3 and pcadv_gemm_b3 (version 9's weight planes split three
 * ways once per step: bitwise pcadv_gemm's result, measured slower) removed;
 * nothing else changes. */
int pcadv_abi_version(void);

/* ---- PointNetfeat (feature_transform=False) -------------------------------
 * pts [C][N][3]; w1 [64][3], w2 [64][64], w3 [128][64], w4 [1024][128] + biases.
 * One fused pass (conv1..conv4 + max): writes x3 [C][N][128] (post-ReLU conv3
 * output, read by the backward), gmax [C][1024] (x_global, pointnet.py:129-130,
 * an exact f32 dot product) and gidx [C][1024] (argmax over points, first index
 * on ties as torch.max on CPU).  conv1/conv2 are computed in f32, conv3 as six
 * bf16 split products (f32-level); conv4 screens the points with three bf16
 * MFMAs per product (|err| <= ~3 2^-16 sum|x w|) and re-evaluates the top two
 * points of every channel in exact f32, ranked by those values. */
size_t pcadv_feat_fwd_workspace_bytes(int C, int N);
int pcadv_feat_fwd(const float* pts, int C, int N,
                   const float* w1, const float* b1, const float* w2, const float* b2,
                   const float* w3, const float* b3, const float* w4, const float* b4,
                   float* x3, float* gmax, int32_t* gidx,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

/* pcadv_feat_fwd in bf16 mode (BASELINE configs[1]'s "bf16"): conv3 and conv4
 * multiply bf16-rounded operands with f32 accumulation (one MFMA product each);
 * gmax is the winner's bf16-product value (low 6 bits of its screening key
 * dropped), gidx its point (first index on equal keys).  conv1/conv2 stay f32
 * (the backward's recompute of x1/x2 is bitwise).  x3 is stored as bf16
 * [C][N][128] (2 bytes per element, the rounding conv4 applies to it; ABI
 * version 10): pcadv_feat_bwd takes it widened to f32. */
int pcadv_feat_fwd_bf16(const float* pts, int C, int N,
                        const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, const float* w4, const float* b4,
                        void* x3, float* gmax, int32_t* gidx,
                        void* workspace, size_t workspace_bytes, hipStream_t stream);

/* The second launch of pcadv_feat_fwd alone: conv4 (128 -> 1024, no ReLU) +
 * torch.max over the points (models/pointnet.py:128-130) of given conv3
 * activations x3 [C][N][128] -> gmax, gidx [C][1024]; precision 0 = f32-level
 * (as pcadv_feat_fwd), 1 = bf16 over an f32 x3, 2 = bf16 over a bf16 x3 (as
 * pcadv_feat_fwd_bf16 runs it on the x3 it stores; ABI version 10). */
int pcadv_conv4_max(const void* x3, int C, int N, const float* w4, const float* b4,
                    float* gmax, int32_t* gidx, int precision, hipStream_t stream);

/* Bytes of workspace pcadv_feat_bwd needs for C clouds of N points. */
size_t pcadv_feat_bwd_workspace_bytes(int C, int N);

/* Autograd of pcadv_feat_fwd: dgmax [C][1024] -> dw1..db4 (overwritten).
 * The max-pool backward is sparse (each channel's gradient goes to its argmax
 * point), equal to torch's MaxBackward for unique maxima; conv1/conv2 outputs
 * of the points that receive gradient are recomputed from pts. */
int pcadv_feat_bwd(const float* dgmax, const int32_t* gidx, const float* pts, int C, int N,
                   const float* w1, const float* b1, const float* w2, const float* b2,
                   const float* w3, const float* w4, const float* x3,
                   float* dw1, float* db1, float* dw2, float* db2,
                   float* dw3, float* db3, float* dw4, float* db4,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Generic 1x1-conv (K=128 -> O, O % 128 == 0) + max over points.
 * relu_before_max=1 for the T-Nets (pointnet.py:30-31,63-64).  O = 1024 runs
 * on the fused forward's k_conv4_max (split-product screen, every winner
 * re-evaluated in exact f32; with the ReLU, an all-negative channel's argmax
 * is point 0, as torch.max over the zeros gives); other O on an f32 kernel. */
int pcadv_conv_max_fwd(const float* x, int C, int N, int K, const float* w, const float* b,
                       int O, int relu_before_max, float* gmax, int32_t* gidx,
                       hipStream_t stream);

/* ---- point-wise layers: the feature-transform path --------------------------
 * (PointNetCls(feature_transform=True): PointNetfeat conv1/conv2/conv3 with the
 * STNkd(64) transform, models/pointnet.py:46-79,109-122.)  Rows are points,
 * point-major [M][C].
 *
 * pcadv_pw_fwd: y[M][O] = act(x[M][K] W^T + b) (b may be NULL), K in {3, 64,
 * 128}, O % 32 == 0, act NONE/RELU.  W is the Conv1d weight [O][K], or with
 * w_kmajor=1 a [K][O] matrix (y = x T: the feature-transform bmm,
 * pointnet.py:120-121); rows_per_w > 0 (a multiple of 64) uses one matrix per
 * rows_per_w rows (one per cloud, W + cloud * O * K). */
int pcadv_pw_fwd(const float* x, int M, int K, const float* w, const float* b, int O, int act,
                 int w_kmajor, int rows_per_w, float* y, hipStream_t stream);

/* pcadv_pw_chain: n consecutive pcadv_pw_fwd layers in ONE launch (layer i's
 * input is layer i-1's output, layer 0's is x[M][K]); every layer's y is
 * written, bitwise what the per-layer pcadv_pw_fwd calls write.  Instantiated
 * for the feature-transform extractor (models/pointnet.py:115-122, :57-60):
 * K = 3 -> 64, 64, 64, 128 (conv1, conv2, STNkd conv1, STNkd conv2) and
 * K = 64 -> 64, 128 (x2 T, conv3); other shapes return PCADV_EINVAL. ABI 9. */
#define PCADV_PW_CHAIN_MAX 4
typedef struct pcadv_pw_layer {
  const float* w; /* [O][K] Conv1d weight, or [K][O] with w_kmajor = 1 */
  const float* b; /* bias [O] or NULL */
  float* y;       /* output [M][O] */
  int O;
  int act;        /* PCADV_ACT_NONE / PCADV_ACT_RELU */
  int w_kmajor;
  int rows_per_w; /* 0, or a multiple of 64: one matrix per rows_per_w rows */
} pcadv_pw_layer;
int pcadv_pw_chain(const float* x, int M, int K, const pcadv_pw_layer* layers, int n,
                   hipStream_t stream);

/* dx[M][K] (+)= (dy * act'(y)) W  (y = that layer's output; O in {64, 128},
 * K % 32 == 0); accumulate=1 adds into dx. */
int pcadv_pw_bwd_data(const float* dy, const float* y, int act, int M, int O, const float* w,
                      int K, int w_kmajor, int rows_per_w, float* dx, int accumulate,
                      hipStream_t stream);

/* dW = sum over rows of (dy * act'(y))^T x and db (NULL: skipped), per group
 * of rows_per_group rows (0: all rows; a multiple of 128 dividing M): dw holds
 * M / rows_per_group matrices, [O][K] or with dw_kmajor=1 [K][O] (dT of the
 * bmm).  O in {64, 128}, K in {3, 64, 128} (K = 3: O = 64, [O][K]).
 * Deterministic (fixed-order reduction over 128-row slabs in the workspace). */
size_t pcadv_pw_bwd_weight_workspace_bytes(int M, int O, int K);
int pcadv_pw_bwd_weight(const float* dy, const float* y, int act, const float* x, int M, int O,
                        int K, int rows_per_group, int dw_kmajor, float* dw, float* db,
                        void* workspace, size_t workspace_bytes, hipStream_t stream);

/* The deferred form of pcadv_pw_bwd_weight (rows_per_group = 0, dw [O][K]):
 * pcadv_pw_bwd_weight with dw = db = NULL writes only the per-slab partial sums
 * into its workspace; pcadv_pw_wgrad_finish then sums the slabs of up to 8
 * such weight gradients (each job: that call's workspace, M, O, K, and the
 * dw / db to write) in ONE launch, bitwise the per-call sums.  The
 * feature-transform step's backward finishes its five parameter gradients
 * this way.  ABI version 8. */
typedef struct pcadv_pw_wgrad_job {
  const void* slabs;
  int M, O, K;
  float* dw;
  float* db;
} pcadv_pw_wgrad_job;
int pcadv_pw_wgrad_finish(const pcadv_pw_wgrad_job* jobs, int njobs, hipStream_t stream);

/* Backward of pcadv_conv_max_fwd: each channel's gradient goes to its argmax
 * point (times [gmax > 0] when gmax_relu is given: the ReLU before the max of
 * the T-Nets, pointnet.py:30-31,63-64).  dw [O][K], db [O] (may be NULL), dx
 * [C][N][K] (NULL: skipped; rows of points without hits are written as 0).
 * dx_relu (ABI 8): x is the ReLU output of the layer below and dx is stored
 * as that layer's pre-activation gradient, dx * [x > 0], so the layer's
 * backward reads no activations for its mask. */
int pcadv_conv_max_bwd(const float* dgmax, const int32_t* gidx, const float* gmax_relu,
                       const float* x, int C, int N, int K, const float* w, int O, float* dw,
                       float* db, float* dx, int dx_relu, hipStream_t stream);

/* feature_transform_regularizer (pointnet.py:345-353): norms[b] =
 * ||T_b T_b^T - I||_F and *reg = mean_b norms[b]; backward dT = *grad_reg *
 * (2 / (B norms[b])) (T T^T - I) T, and 0 for a cloud with norms[b] = 0 (as
 * torch.norm's backward).  k <= 64. */
int pcadv_tnet_reg_fwd(const float* T, int B, int k, float* norms, float* reg,
                       hipStream_t stream);
int pcadv_tnet_reg_bwd(const float* T, int B, int k, const float* grad_reg, float* dT,
                       hipStream_t stream);
/* The regulariser of a training step in two launches (ABI 9): norms and
 * *reg as pcadv_tnet_reg_fwd, dT += pcadv_tnet_reg_bwd's gradient (the bmm's
 * dT accumulated in place; a cloud with norm 0 leaves its dT untouched), and
 * *step_count += 1 when given, once per call (the fused feature-transform cls
 * step advances its count there on every call, ahead of its Adam). */
int pcadv_tnet_reg_step(const float* T, int B, int k, float* norms, float* reg,
                        const float* grad_reg, float* dT, int32_t* step_count,
                        hipStream_t stream);

/* ---- linear / 1x1 conv on B x C x 1 ----------------------------------------
 * y[M][Nout] = act(s * (x[M][K] w[Nout][K]^T + b)), where s is the dropout
 * scale: drop_mask[M][Nout] in {0,1} times 1/(1-drop_p) when drop_mask is
 * non-NULL, else a device Philox draw keyed by (rng_seed, *rng_step) when
 * rng_step is non-NULL, else 1.  K % 4 == 0.  add_identity_k > 0 (with
 * Nout == k*k) adds the flattened k x k identity after the activation: the
 * T-Net output transform (STNkd fc3 + iden, models/pointnet.py:70-77). */
int pcadv_linear_fwd(const float* x, const float* w, const float* b, float* y,
                     int M, int Nout, int K, int act,
                     const float* drop_mask, const int32_t* rng_step, uint64_t rng_seed,
                     float drop_p, int add_identity_k, hipStream_t stream);

/* Backward of pcadv_linear_fwd.  dz = dy * act'(y) * s (y = the forward output).
 * dx[M][K] = dz w (skipped when dx is NULL); dw[Nout][K] = sum over the first
 * m_w rows of dz^T x, db[Nout] likewise (skipped when dw is NULL). */
int pcadv_linear_bwd(const float* dy, const float* y, int act,
                     const float* drop_mask, const int32_t* rng_step, uint64_t rng_seed,
                     float drop_p, const float* x, const float* w,
                     float* dx, float* dw, float* db, int M, int m_w, int Nout, int K,
                     hipStream_t stream);

/* ---- dense point-wise GEMM engine: the segmentation net ---------------------
 * (PointNetSeg, models/pointnet.py:261-317; run_training_pointnet_seg,
 * utils/trainer.py:310-400.)  Rows are points (point-major [B*N][C]); f32
 * operands are split to bf16 hi + lo and multiplied as three bf16 MFMA products
 * with f32 accumulation (relative error <= ~1.2e-5 of sum|a b| over a sum
 * whose terms' errors average out; one product alone can be off by up to
 * 3 * 2^-16 = 4.6e-5 of |a b|, so reductions shorter than K = 16 always take
 * the six-product form below).
 *
 * pcadv_gemm: C[m][n] (+)= sum_k A[m][k] B[n][k] (+ bias[n] + bias_rows[m /
 * rows_per_group][n]), ReLU optional.  A[m][k] = a[m*lda + k] (ta = 0) or
 * a[k*lda + m] (ta = 1, only with tb = 1); B[n][k] = b[n*ldb + k] (tb = 0: a
 * weight [out][in], the forward) or b[k*ldb + n] (tb = 1: dX = dZ W).
 * accumulate = 1 adds into C.  cmask (nullable, stored like C with stride ldm)
 * then zeroes C where cmask <= 0: the producer of a data gradient applies the
 * relu' of the layer below, so every consumer reads dZ = dY relu'(Y) already
 * masked.  precise = 1 multiplies six products of hi/mid/lo splits instead
 * (f32-level accuracy; the gradients); K < 16 does so whatever precise says.  c_hi / c_lo (nullable, bf16, row
 * stride ldcp): the epilogue also writes C's hi / lo planes, the operand form
 * pcadv_gemm_bf2 stages without splitting.
 * Requirements: lda >= K (ta = 0) or M (ta = 1), ldb >= K (tb = 0) or N
 * (tb = 1), ldc >= N, ldm >= N; float-aligned pointers, any stride and any
 * N, K (16-B loads are used where an operand is 16-B aligned with a stride
 * % 4 == 0 and no vector straddles an edge, dword loads elsewhere: the same
 * values either way); bias [N] and bias_rows [ceil(M / rows_per_group)][N]
 * dense; every operand spans < 2 GB.  Output planes need N % 4 == 0,
 * ldcp >= N, ldcp % 4 == 0, 8-B aligned planes, and C, bias, bias_rows and
 * cmask 16-B aligned with ldc % 4 == 0 and ldm % 4 == 0; they are not
 * available on the few-row form (ta = 0, M <= 32: exact f32 FMAs on the
 * vector ALUs instead of MFMAs, the same epilogue). */
int pcadv_gemm(const float* a, int64_t lda, int ta, const float* b, int64_t ldb, int tb,
               float* c, int64_t ldc, int M, int N, int K, const float* bias,
               const float* bias_rows, int rows_per_group, int relu, int accumulate,
               const float* cmask, int64_t ldm, int precise, void* c_hi, void* c_lo, int64_t ldcp,
               hipStream_t stream);

/* The forward GEMM with both operands given as bf16 hi / lo planes (A [M][K],
 * B [N][K], the 2-way splits of f32 matrices made once by their producers:
 * hi = bf16(v), lo = bf16(v - hi)); bitwise the result pcadv_gemm computes
 * from the f32 matrices (precise = 0), without re-splitting every tile.
 * K % 16, lda % 8, ldb % 8, lda >= K, ldb >= K, 16-B aligned planes (any M,
 * N; row strides above K allowed); the output planes as for pcadv_gemm. */
int pcadv_gemm_bf2(const void* a_hi, const void* a_lo, int64_t lda, const void* b_hi,
                   const void* b_lo, int64_t ldb, float* c, int64_t ldc, void* c_hi, void* c_lo,
                   int64_t ldcp, int M, int N, int K, const float* bias, const float* bias_rows,
                   int rows_per_group, int relu, int accumulate, const float* cmask, int64_t ldm,
                   hipStream_t stream);
/* f32 [rows][cols] (stride ld) -> its bf16 hi / lo planes (stride ldo). */
int pcadv_split_bf2(const float* x, int64_t ld, int rows, int cols, void* hi, void* lo,
                    int64_t ldo, hipStream_t stream);

/* Weight gradient dw[o][k] (row stride ldo) (+)= sum over `rows` points of
 * dz[p][o] x[p][k]: six-product (f32-level) GEMM over fixed-order slabs of the
 * point axis.  db (nullable) (+)= the column sums of dz (the bias gradient);
 * gsum (nullable, needs rows_per_group > 0 dividing rows) = the sums of dz over
 * each group of rows_per_group rows ([rows / rows_per_group][O], overwritten:
 * fc1's per-cloud sums).  Both come from the staged dz, no second pass.
 * rows_per_group (0 = one group) also sets the slab plan, so pass the same
 * value to the workspace query.  ldz >= O, ldx >= Kin, ldo >= Kin, any
 * alignment of dz and x; the workspace 16-B aligned; db and gsum each may be
 * NULL; accumulate applies to dw and db. */
size_t pcadv_gemm_wgrad_workspace_bytes(int rows, int O, int Kin, int rows_per_group);
int pcadv_gemm_wgrad(const float* dz, int64_t ldz, const float* x, int64_t ldx, int rows, int O,
                     int Kin, float* dw, int64_t ldo, float* db, float* gsum, int rows_per_group,
                     int accumulate, void* workspace, size_t workspace_bytes, hipStream_t stream);
/* Descriptor forms of pcadv_gemm_wgrad's and pcadv_gemm's arguments, for the
 * split / paired entry points below.  A descriptor is read during the call
 * only: the library keeps neither it nor any pointer in it. */
typedef struct pcadv_wgrad_desc {
  const float* dz; int64_t ldz; const float* x; int64_t ldx;
  int rows, O, Kin; float* dw; int64_t ldo; float* db; float* gsum;
  int rows_per_group, accumulate; void* workspace; size_t workspace_bytes;
} pcadv_wgrad_desc;
typedef struct pcadv_gemm_desc {
  const float* a; int64_t lda; int ta; const float* b; int64_t ldb; int tb;
  float* c; int64_t ldc; int M, N, K; const float* bias; const float* bias_rows;
  int rows_per_group, relu, accumulate; const float* cmask; int64_t ldm; int precise;
  void* c_hi; void* c_lo; int64_t ldcp;
} pcadv_gemm_desc;
/* pcadv_gemm_wgrad split in two calls, so that one launch can finish the slab
 * sums of many weight gradients (the seg backward's launch count, not its
 * values: bitwise pcadv_gemm_wgrad).
 * pcadv_gemm_wgrad_slabs enqueues w's slab GEMM into w->workspace (and, when
 * w->gsum is given, the per-group sums and db now); when g is non-null it also
 * enqueues the GEMM g (a data gradient: pcadv_gemm's arguments), and where both
 * have the engine's pairable forms (g: ta = 0, tb = 1, either precision, M > 32,
 * operands vectorisable: 16-B aligned rows, VEC >= 2) the two run as ONE launch, their workgroups side by side, each output bitwise its
 * own launch's; a g of another form is enqueued on its own.  g must not write
 * anything w reads or writes, nor read anything w writes (both may read the same dz).
 * pcadv_wgrad_finish then enqueues the remaining dw (and db) sums of n such
 * weight gradients in one launch (more launches above 16).  Between the two
 * calls the caller keeps dw, db and the workspaces alive and untouched; nothing
 * is held by the library, so a caller that abandons a backward between them
 * simply drops its descriptors. */
int pcadv_gemm_wgrad_slabs(const pcadv_wgrad_desc* w, const pcadv_gemm_desc* g,
                           hipStream_t stream);
int pcadv_wgrad_finish(const pcadv_wgrad_desc* w, int n, hipStream_t stream);
/* Weight gradient over a few rows in exact f32 (rows in order):
 * dw0[o][k] (+)= sum_{b < B} s[b][o] x0[b][k] for k < K0, and the same with
 * x1 / K1 / dw1 when x1 is given, in one launch (fc1's per-cloud columns). */
int pcadv_wgrad_small(const float* s, int64_t lds, int B, int O, const float* x0, int64_t ldx0,
                      int K0, float* dw0, const float* x1, int64_t ldx1, int K1, float* dw1,
                      int64_t ldo, int accumulate, hipStream_t stream);

/* Column sums (bias gradients): out[n] (+)= sum_m x[m][n] [ymask[m][n] > 0];
 * pcadv_group_colsum writes one row of sums per rows_per_group rows (M %
 * rows_per_group == 0; out [M / rows_per_group][N] dense, overwritten).
 * ymask nullable; ld, ldm >= N, any alignment. */
size_t pcadv_colsum_workspace_bytes(int M, int N);
int pcadv_colsum(const float* x, const float* ymask, int64_t ld, int64_t ldm, int M, int N,
                 float* out, int accumulate, void* workspace, size_t workspace_bytes,
                 hipStream_t stream);
int pcadv_group_colsum(const float* x, const float* ymask, int64_t ld, int64_t ldm, int M, int N,
                       int rows_per_group, float* out, hipStream_t stream);

/* conv + (ReLU) + max over the Npts points of each of C clouds (conv6 + the
 * global max, pointnet.py:301-303): gmax [C][O], gidx [C][O] (first index on
 * ties of the f32 values; with relu the pooled value is relu(max)).  A screened
 * GEMM keeps per-128-point-tile top-2 candidates; the winner (and the
 * runner-up on near-ties) is re-evaluated as an f32 dot product of x and w.
 * K % 32 == 0, ldx % 4 == 0, ldx >= K, x and w ([O][K] dense) 16-B aligned;
 * any C, Npts, O; b nullable. */
size_t pcadv_conv_max_x3_workspace_bytes(int C, int Npts, int O);
int pcadv_conv_max_x3(const float* x, int64_t ldx, int C, int Npts, int K, const float* w,
                      const float* b, int O, int relu, float* gmax, int32_t* gidx,
                      void* workspace, size_t workspace_bytes, hipStream_t stream);
/* The same with the screened GEMM staging x and w from their bf16 hi / lo
 * planes (x still given in f32 for the exact re-evaluation): ldxp % 8 == 0,
 * ldxp >= K, w's planes [O][K] dense, all four planes 16-B aligned. */
int pcadv_conv_max_bf2(const float* x, int64_t ldx, const void* x_hi, const void* x_lo,
                       int64_t ldxp, int C, int Npts, int K, const float* w, const void* w_hi,
                       const void* w_lo, const float* b, int O, int relu, float* gmax,
                       int32_t* gidx, void* workspace, size_t workspace_bytes,
                       hipStream_t stream);
/* Its backward: g' = dgmax [gmax > 0]; dw [O][K] and db [O] overwritten
 * (each nullable on its own: db is formed with or without dw), dx rows
 * (stride lddx, nullable, K <= 512) accumulated: deterministic.  relu_x = 1
 * masks the dx additions by [x > 0] (x the output of a ReLU layer: the
 * gradient leaves already multiplied by its relu').  K % 4 == 0, ldx % 4 == 0,
 * lddx % 4 == 0, O <= 4096, gidx in [0, Npts); x, w, dw ([O][K] dense) and dx
 * 16-B aligned. */
int pcadv_conv_max_x3_bwd(const float* dgmax, const float* gmax, const int32_t* gidx,
                          const float* x, int64_t ldx, int C, int Npts, int O, int K,
                          const float* w, float* dw, float* db, float* dx, int64_t lddx,
                          int relu_x, hipStream_t stream);

/* ---- data path: HDF5-free dataset reader -------------------
 * Replaces h5py's f['data'][:, 0:npts, :], f['label'][:], f['pid'][:, 0:npts]
 * in dataset/modelNetData.py:43-47 and dataset/shapeNetData.py:176-181 (host
 * code; no HDF5 library).  pcadv_h5_info: rank, dims[<= 8] and the stored type
 * (PCADV_H5_F32 / _F64, or PCADV_H5_INT / _UINT | byte size << 4).
 * pcadv_h5_read: the whole dataset converted to f32 or int64 (row-major), the
 * second dimension cut to its first keep1 entries when 0 < keep1 < dims[1]. */
#define PCADV_H5_F32 1
#define PCADV_H5_F64 2
#define PCADV_H5_INT 3
#define PCADV_H5_UINT 4
#define PCADV_H5_OUT_F32 0
#define PCADV_H5_OUT_I64 1
int pcadv_h5_info(const char* path, const char* name, int* rank, int64_t* dims, int* dtype);
int pcadv_h5_read(const char* path, const char* name, int out_type, int64_t keep1, void* out,
                  size_t out_bytes);

/* Batch assembly on the device: out[b] = src[idx[b]][0:npts] (+ jitter), with
 * src [n_src][src_npts][3] resident in HBM (the whole split), labels
 * src_lab [n_src][lab_width] and part ids src_seg [n_src][src_npts] (both
 * nullable) gathered alongside.  Jitter (dataset/modelNetData.py:80-91):
 * + clip(sigma * z, -clip, clip) per coordinate (sigma = 0: none), z from
 * `noise` ([B][npts][3] f64 standard normals, computed in f64 like numpy) or,
 * when noise is NULL, Philox normals keyed by (seed, *step, point), the point
 * of batch row b counted as row rng_row0 + b (0 for a one-process loader; a
 * data-parallel rank r holding rows [rB, rB + B) of each global batch passes
 * rB, so the ranks jitter exactly as one loader of the global batch would;
 * ABI version 6).  Indices must lie in [0, n_src) (checked by the caller;
 * out-of-range rows are left untouched). */
int pcadv_gather_clouds(const float* src, int64_t n_src, int npts, int src_npts,
                        const int64_t* idx, int B, const int64_t* src_lab, int lab_width,
                        const int64_t* src_seg, double sigma, double clip, const double* noise,
                        uint64_t seed, const int32_t* step, float* out, int64_t* out_lab,
                        int64_t* out_seg, int64_t rng_row0, hipStream_t stream);

/* pcadv_gather_clouds for a graph-replayed loader: batch k = *cursor of the
 * epoch order `order` (int64, k * B + b -> source cloud), so a captured graph
 * gathers a new batch on every replay with no host copy; the caller advances
 * *cursor and *step (pcadv_iter_epilogue) and rewrites `order` at each epoch
 * (DeviceCloudLoader.index_batches' order). */
int pcadv_gather_clouds_at(const float* src, int64_t n_src, int npts, int src_npts,
                           const int64_t* order, const int32_t* cursor, int B,
                           const int64_t* src_lab, int lab_width, const int64_t* src_seg,
                           double sigma, double clip, uint64_t seed, const int32_t* step,
                           float* out, int64_t* out_lab, int64_t* out_seg, int64_t rng_row0,
                           hipStream_t stream);

/* Several graph-fed loaders' pcadv_gather_clouds_at in ONE launch (the
 * training iteration's GT and no-GT batches, trainer.py): job k is exactly the
 * arguments of one pcadv_gather_clouds_at call, and its output is bitwise that
 * call's.  1 <= njobs <= 4.  ABI version 7. */
typedef struct pcadv_gather_job {
  const float* src;
  int64_t n_src;
  int npts, src_npts;
  const int64_t* order;
  const int32_t* cursor;
  int B;
  const int64_t* src_lab;
  int lab_width;
  const int64_t* src_seg;
  double sigma, clip;
  uint64_t seed;
  const int32_t* step;
  float* out;
  int64_t* out_lab;
  int64_t* out_seg;
  int64_t rng_row0;
} pcadv_gather_job;
int pcadv_gather_clouds_multi(const pcadv_gather_job* jobs, int njobs, hipStream_t stream);

/* The adversarial segmentation steps' packed input in ONE launch, from a GT and
 * a no-GT ShapeNet split (both jobs: the same B and npts, lab_width 1, each its
 * own order / cursor / seed / step / sigma / clip / rng_row0; their out,
 * out_lab and out_seg fields are not read):
 *   pts [2B][npts][3]: rows [0, B) the GT job's batch, rows [B, 2B) the no-GT
 *     job's, each half bitwise what pcadv_gather_clouds_at writes for that job;
 *   cls [2B][1][C] f32: the one-hot of each cloud's class id, every element
 *     written (no clearing launch needed); 1 <= C <= 64;
 *   seg [B][npts] int64: the GT job's part ids (the GT job must have src_seg,
 *     the no-GT job none).
 * A cloud index outside its split leaves that row of all three outputs as it
 * was.  Class ids must lie in [0, C) (checked once by the caller; an id outside
 * gives an all-zero row).  An addition to ABI version 11. */
int pcadv_gather_seg_pair(const pcadv_gather_job* gt, const pcadv_gather_job* nogt, int C,
                          float* pts, float* cls, int64_t* seg, hipStream_t stream);

/* The end of a graph-replayed training iteration (trainer.py): counters[i] += 1
 * for i < ncounters (<= 64: loaders' RNG steps and batch cursors), and, when
 * ring is given, losses[0..nl) (nl <= 32) into slot (*ring_count % slots) of the [slots][nl]
 * loss ring, then *ring_count += 1 (the host reads the ring every `slots`
 * iterations instead of copying the losses out every iteration). */
int pcadv_iter_epilogue(int32_t* counters, int ncounters, const float* losses, int nl,
                        float* ring, int slots, int32_t* ring_count, hipStream_t stream);

/* CrossEntropyLoss over rows (the per-point segmentation loss, mean over M
 * points): *loss, and dlogits = scale * dL/dlogits (same stride ld >= ncls;
 * the padding columns are not written).  Any M and ncls; labels in [0, ncls);
 * the row maximum is subtracted before the exponentials. */
size_t pcadv_row_ce_workspace_bytes(int M);
int pcadv_row_ce(const float* logits, int64_t ld, const int64_t* labels, int M, int ncls,
                 float scale, float* loss, float* dlogits, void* workspace,
                 size_t workspace_bytes, hipStream_t stream);

/* Evaluation metrics of one batch on the device (the trainers' test passes,
 * evaluate.py): for logits [M][ncls] (row stride ld >= ncls, 2 <= ncls <= 64)
 * and labels int64 [M] (each in [0, ncls)), per row the argmax (the FIRST index
 * on exact ties, as np.argmax / torch.max on the host) into pred (optional)
 * and the row's cross entropy; per call, into the caller-owned device
 * accumulator acc[4] (zeroed by the caller before a pass):
 *   acc[0] += number of rows with pred == label,
 *   acc[1] += the f32 mean of the M rows' cross entropy (what loss.item() gives),
 *   acc[2] += M,   acc[3] += 1.
 * The mean is a fixed-order sum (no floating-point atomics): two runs on the
 * same inputs leave the same bits.
 * rows_per_group = N > 0 (M % N == 0) adds the mean part IoU of each group
 * (cloud) g of N rows (utils/metric.py:19-30): its category is
 * group_cat[g * cat_stride], whose parts are the labels [cat_parts[2c],
 * cat_parts[2c] + cat_parts[2c + 1]) (device table [ncat][2], at most 8 parts);
 * a part in neither the labels nor the predictions counts 1, the others
 * |gt & pred| / |gt | pred| in f64, summed in part order and divided by the
 * part count: bitwise the host's np.mean.  The IoU goes to iou_out[base + g]
 * and the category to cat_out[base + g], base = *cursor * (M / N) (cursor: a
 * device int32, NULL for 0), so a replayed graph writes each batch's records
 * at its own place.  A category outside [0, ncat) gives a NaN record.
 * Calls sharing acc or the workspace must be ordered on one stream. */
size_t pcadv_row_eval_workspace_bytes(int M);
int pcadv_row_eval(const float* logits, int64_t ld, const int64_t* labels, int M, int ncls,
                   int32_t* pred, int rows_per_group, const int64_t* group_cat,
                   int64_t cat_stride, const int32_t* cat_parts, int ncat,
                   const int32_t* cursor, double* iou_out, int32_t* cat_out, double* acc,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- Adam (torch.optim.Adam semantics, amsgrad=False, weight_decay=0) ------
 * step_count: device int32, incremented by this call (t = *step_count + 1). */
int pcadv_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
               int64_t n, int32_t* step_count, float lr, float beta1, float beta2,
               float eps, hipStream_t stream);

/* out = [a; b] (na + nb floats) and, when inc_counter is not NULL,
 * *inc_counter += 1: the feature-transform step's first launch, its GT and
 * no-GT batches as one 2B-cloud input (PointNetCls runs on each,
 * utils/trainer.py:467,490) and the iteration's step number advanced for the
 * device draws and pcadv_adam2.  ABI version 8. */
int pcadv_concat2(const float* a, int64_t na, const float* b, int64_t nb, float* out,
                  int32_t* inc_counter, hipStream_t stream);

/* Two Adam updates of one iteration in one launch (segment 1 may be empty,
 * n1 = 0), each with its own learning rate, at the step number *step_count
 * that the iteration already advanced (pcadv_adv_step part 3): t =
 * *step_count, not incremented.  The feature-transform step's optimizer.step()
 * + optimizer_D.step() (utils/trainer.py:558-559).  ABI version 8. */
int pcadv_adam2(float* p0, const float* g0, float* m0, float* v0, int64_t n0, float lr0,
                float* p1, const float* g1, float* m1, float* v1, int64_t n1, float lr1,
                const int32_t* step_count, float beta1, float beta2, float eps,
                hipStream_t stream);

/* ---- the fused adversarial step (utils/trainer.py:426-559) -------------------
 * B clouds of N points per loader.  Stochastic inputs: when drop_mask_gt /
 * drop_mask_nogt ([B][256] {0,1}) or soft_gt / soft_nogt ([B]) are NULL they are
 * drawn on device from Philox keyed by (rng_seed, *step_count), so a captured
 * graph draws fresh values each replay. */
typedef struct pcadv_adv_args {
  int B, N;
  /* inputs */
  const float* pts_gt;      /* [B][N][3] */
  const int64_t* labels;    /* [B] class ids in [0,40) */
  const float* pts_nogt;    /* [B][N][3] */
  const float* drop_mask_gt, * drop_mask_nogt;
  const float* soft_gt, * soft_nogt;
  /* generator: flat params / grads / Adam moments (PCADV_G_NUMEL floats) */
  float* g_param, * g_grad, * g_m, * g_v;
  /* discriminator (PCADV_D_NUMEL floats) */
  float* d_param, * d_grad, * d_m, * d_v;
  int32_t* step_count;      /* device: completed steps (shared by both Adams) */
  float lr_g, lr_d, beta1, beta2, eps;
  float lambda_cls, lambda_adv, drop_p;
  uint64_t rng_seed;
  int apply_adam;           /* 0: stop after the gradients (parity tests) */
  /* outputs */
  float* losses;            /* [4]: loss_cls, loss_adv, loss_D_gt, loss_D_nogt
                               ([6] with semi: + loss_semi, kept ratio) */
  float* logits;            /* [2B][40] or NULL */
  /* scratch */
  void* workspace;
  size_t workspace_bytes;
  /* run_training_semi (utils/trainer.py:611-847, :716-743): when semi != 0 the
   * generator loss gains lambda_semi * CrossEntropyLoss(ignore_index=255) of
   * the no-GT logits against their own argmax, the clouds with
   * D(log_softmax(pred_nogt)) <= semi_th ignored (no term when all are) */
  int semi;
  float lambda_semi, semi_th;
  /* 0: the whole step.  A data-parallel step may split it so the gradients
   * that are final early are all-reduced while the feature backward runs:
   * 1 = forward, losses, discriminator and head backward (every gradient
   *     except the generator's conv1..conv4, g_grad[0, PCADV_G_FC1_W));
   * 2 = the feature backward (those conv1..conv4 gradients; and both Adam
   *     updates when apply_adam) on the state part 1 left in the workspace;
   * 3 = part 1 from fc1 on, over the caller's features (feat_* below);
   *     pcadv_cls_step takes 0 or 3 (ABI 9: its head on given features). */
  int part;
  /* feature forward precision: 0 = f32-level (default), 1 = bf16 (as
   * pcadv_feat_fwd_bf16, x3 kept in bf16 for the feature backward; the head,
   * the discriminator and every backward stay f32 arithmetic).  ABI version 5;
   * the bf16 x3 since version 10. */
  int precision;
  /* Data parallelism (ABI version 6): rank rng_rank of rng_world (<= 1: one
   * process) holding GT rows [rank B, rank B + B) and no-GT rows [rank B,
   * rank B + B) of the rng_world B-cloud global batches.  The device-drawn
   * dropout masks and soft D labels are keyed by those global rows, so with
   * the same rng_seed and step count the ranks draw exactly the slices of the
   * one-process step on the global batch (the dropout row of no-GT row j is
   * rng_world B + j, as in the one-process [GT; no-GT] batch). */
  int rng_rank, rng_world;
  /* The graph-replayed training iteration's epilogue (pcadv_iter_epilogue:
   * epi_counters[0..epi_ncounters) += 1, losses[0..epi_nl) into slot
   * (*epi_ring_count % epi_slots) of the [epi_slots][epi_nl] ring, then
   * *epi_ring_count += 1) run by the step's last launch instead of a launch of
   * its own; epi_ncounters = 0 and epi_ring = NULL: none.  Not with part = 1.
   * pcadv_adv_step and pcadv_cls_step.  ABI version 7. */
  int32_t* epi_counters;
  int epi_ncounters;
  float* epi_ring;
  int epi_slots, epi_nl;
  int32_t* epi_ring_count;
  /* The step's input batches gathered by its first launch (the feature
   * forward's point loads) instead of a pcadv_gather_clouds_multi launch
   * before the step: job 0 fills pts_gt (and, with src_lab, the label rows
   * `labels` points into), job 1 pts_nogt (the adversarial step; the cls step
   * takes job 0 only).  Each job as pcadv_gather_clouds_at (device jitter, no
   * part ids) with out = the step's input buffer: bitwise that gather's
   * batch.  ngather = 0: none.  ABI version 7. */
  const pcadv_gather_job* gather;
  int ngather;
  /* A generator whose feature extractor runs outside the step (the
   * feature-transform generator, PointNetCls(feature_transform=True), built
   * from the point-wise kernels): part = 3 runs part 1's work from fc1 on
   * (fc1..fc3 + dropout, log_softmax / CE, the three discriminator passes with
   * their BCE terms, D's gradients, the head backward) on the caller's pooled
   * features feat_gmax [2B][1024] (GT clouds first) and writes dL/dgmax to
   * feat_dgmax [2B][1024].  No gather, epilogue or Adam, and *step_count is
   * NOT advanced: the caller's first launch advances it (pcadv_concat2), its
   * extractor's backward and Adam (pcadv_adam2) follow.  NULL for parts 0-2.
   * ABI version 8. */
  const float* feat_gmax;
  float* feat_dgmax;
} pcadv_adv_args;

size_t pcadv_adv_step_workspace_bytes(int B, int N);
int pcadv_adv_step(const pcadv_adv_args* args, hipStream_t stream);

/* A test and diagnostic view of the step's workspace (an addition to ABI 11;
 * nothing existing changes): the byte offsets, from args->workspace, of the
 * arrays pcadv_adv_step and pcadv_cls_step called with the same (B, N) leave
 * there, and `total` = pcadv_adv_step_workspace_bytes(B, N).  The layout is
 * private to the library and may change with any build: read it through this
 * call, never by a copy of the offsets (as x_out of pcadv_pwdisc_backward, a
 * view for tests, not an interface to compute on).  All arrays are f32,
 * row-major.  With C = 2B generator rows (GT clouds first; the cls step uses
 * rows [0, B) only) and R = 3B discriminator rows ([D(lsm_gt); D(lsm_nogt);
 * the adversarial pass on lsm_nogt again]):
 *   h1 [C][512], h2 [C][256]   fc1 / fc2 outputs (after ReLU and dropout)
 *   logits, dlogits [C][40]    fc3 output (when args->logits is NULL) and dL/dlogits
 *   dh2 [C][256], dh1 [C][512] dL/d(fc2 / fc1 pre-activation): each data gradient
 *                              is stored as the dz of the layer below
 *   dgmax [C][1024]            dL/d(pooled features) (parts 0..2; part 3 writes
 *                              args->feat_dgmax instead)
 *   din [R][40]                the discriminator's input rows (log_softmax)
 *   d1 [R][512], d2, d3 [R][256]   D conv1..conv3 outputs
 *   dd1 [R][512], dd2, dd3 [R][256] dL/d(conv1..conv3 pre-activation); rows
 *                              [0, 2B) carry the D loss, rows [2B, 3B) the
 *                              generator's adversarial loss
 *   a4 [2B][64]                D conv4 output, rows [0, 2B) ONLY
 *   z4, z5 [2B][64]            dL/d(conv4 / conv5 pre-activation), rows [0, 2B)
 *                              ONLY (the rows D's weight gradients sum over)
 *   mask [C][256]              the {0,1} dropout mask of fc2 (given or drawn)
 *   dout [R]                   the D logits
 *   rowloss [B]                the cls step's CE_r / B
 * The adversarial step leaves rowloss untouched, the cls step everything from
 * din to dout but mask.  Returns PCADV_EINVAL for B outside [1, 256], N < 1 or
 * out NULL. */
typedef struct {
  size_t h1, h2, logits, dlogits, dh2, dh1, dgmax;
  size_t din, d1, d2, d3, dd3, dd2, dd1;
  size_t z4, z5, a4, mask, dout, rowloss, total;
} pcadv_step_ws_layout;
int pcadv_adv_step_workspace_layout(int B, int N, pcadv_step_ws_layout* out);

/* The two Adam updates of pcadv_adv_step alone (optimizer.step() and
 * optimizer_D.step(), trainer.py:558-559), for a step that ran with
 * apply_adam = 0 and whose gradients were then all-reduced across ranks.
 * Uses the step counter already advanced by that pcadv_adv_step.  args->part
 * selects the parameters (Adam is elementwise, so parts 1 + 2 equal part 0
 * bitwise): 0 = all; 1 = those whose gradients part 1 of the step finalises
 * (g_param[PCADV_G_FC1_W, PCADV_G_NUMEL) and all of D), so they can update
 * while the conv1..conv4 bucket is still being all-reduced; 2 = the rest
 * (g_param[0, PCADV_G_FC1_W)). */
int pcadv_adv_step_adam(const pcadv_adv_args* args, hipStream_t stream);

/* One iteration of run_training_pointnet_cls (utils/trainer.py:222-268,
 * feature_transform=False; BASELINE configs[1]): PointNetCls forward on the B
 * clouds of pts_gt (labels), loss = lambda_cls * CrossEntropyLoss, backward,
 * and (apply_adam) the generator's Adam step.  Uses the generator fields of
 * pcadv_adv_args (pts_nogt, d_*, soft_*, lambda_adv, semi ignored);
 * drop_mask_gt optional (else device-drawn); losses[0] = CE; workspace as
 * pcadv_adv_step_workspace_bytes(B, N).  part = 3 (ABI 9): the head alone on
 * the caller's pooled features feat_gmax [B][1024] (fc1 .. the CE, and back to
 * feat_dgmax = dL/dgmax and the head's gradients), for the feature-transform
 * generator's step whose extractor runs outside.  Part 3 does not touch
 * *step_count: the head's dropout draws read it as it stands (the count of
 * the completed calls), and the caller advances it afterwards (the fused
 * feature-transform step in its pcadv_tnet_reg_step launch, on every call,
 * with or without Adam) and runs Adam at the advanced count. */
int pcadv_cls_step(const pcadv_adv_args* args, hipStream_t stream);

/* ---- PointwiseDiscNet of the adversarial segmentation step -----------------
 * (models/discriminator.py:53-79, utils/trainer.py:849-1026, run_training_seg.)
 * Additions to ABI 10 (nothing existing changes).
 *
 * logits [n0 + n1][ncls] point-major (row stride ld), 2 <= ncls <= 64.  Rows
 * [0, n0) are the GT clouds' points and enter D through transform t0, rows
 * [n0, n0 + n1) the no-GT clouds' through t1 (the reference: softmax and
 * log_softmax, trainer.py:901,914).  w[i] / b[i]: conv1..conv4 ([64][ncls],
 * [64][64], [64][64], [128][64]; conv2..conv4 16-B aligned).
 *
 * pcadv_pwdisc_forward, one launch: out[row] = max over the 128 channels of
 * relu(conv4(..relu(conv1(x)))) on exact f32 MFMAs in k order, argc[row] its
 * channel (the first on ties).  With losses != NULL also the iteration's
 * three BCE-with-logits terms:
 *   losses[0] = loss_adv = mean over the no-GT rows against label 1,
 *   losses[2] = 0.5 mean over the GT rows against soft labels of U(0.7, 1.05),
 *   losses[3] = 0.5 mean over the no-GT rows against soft labels of U(0, 0.305),
 *   losses[1] = loss_D = losses[2] + losses[3],
 * and their derivatives dout_d[n0 + n1] (loss_D's) and dout_adv[n1]
 * (loss_adv's, optional).  The labels, one per point (make_D_label(random=
 * True)), are soft0[n0] / soft1[n1] or, where those are NULL, drawn from Philox
 * keyed by (rng_seed, *step_count, row); soft_out[n0 + n1] (optional) receives
 * them.  The sums run in a fixed order (no floating-point atomics).  The first
 * 256 bytes of the workspace are a ticket that must be zero when a forward
 * with losses starts and is zero again when it ends: zero the workspace once.
 *
 * pcadv_pwdisc_backward, one launch and a fixed-order finish: recomputes
 * x1..x3 (the forward's bits), routes the gradient to channel argc (none for a
 * row whose out is 0) and writes dw[i] / db[i] = the gradients of
 * sum_row dout_d[row] out[row], and, with dlogits and dout_adv given, the
 * gradient of lambda_adv sum_j dout_adv[j] out[n0 + j] with respect to the
 * no-GT rows' logits (through transform t1) into rows [n0, n0 + n1) of
 * dlogits (row stride ldd; the other rows are not touched).  Reads out, argc.
 * x_out (optional, [3][n0 + n1][64]) receives the recomputed x1..x3, whose signs
 * are the ReLU masks the backward used (tests).
 *
 * max_workgroups: 0, or a cap on the persistent grids (tests).  The workspace
 * (pcadv_pwdisc_workspace_bytes(n0 + n1, max_workgroups)) is shared by the two. */
#define PCADV_PWD_NONE 0
#define PCADV_PWD_SOFTMAX 1
#define PCADV_PWD_LOG_SOFTMAX 2
typedef struct pcadv_pwdisc_args {
  const float* logits;
  int64_t ld;
  int ncls, n0, n1, t0, t1;
  const float* w[4];
  const float* b[4];
  float* out;
  int32_t* argc;
  float* losses;
  const float* soft0;
  const float* soft1;
  float* soft_out;
  uint64_t rng_seed;
  const int32_t* step_count;
  float* dout_d;
  float* dout_adv;
  float lambda_adv;
  float* dw[4];
  float* db[4];
  float* dlogits;
  int64_t ldd;
  int max_workgroups;
  void* workspace;
  size_t workspace_bytes;
  float* x_out;
} pcadv_pwdisc_args;
size_t pcadv_pwdisc_workspace_bytes(int64_t rows, int max_workgroups);
int pcadv_pwdisc_forward(const pcadv_pwdisc_args* args, hipStream_t stream);
int pcadv_pwdisc_backward(const pcadv_pwdisc_args* args, hipStream_t stream);

/* ---- The semi-supervised term of run_training_seg_semi ----------------------
 * (utils/trainer.py:1999-2024.)  Additions to ABI 10 (nothing existing changes).
 *
 * logits [M][ncls] (row stride ld >= ncls, 2 <= ncls <= 64) are the no-GT
 * rows' predictions, d_out [M] D's raw per-point output on them.  Row r is
 * KEPT iff !(d_out[r] <= semi_th) (a value equal to the threshold is ignored,
 * as semi_ignore_mask = D_out <= semi_TH does).  Its pseudo-label is the FIRST
 * index of the row's maximum (torch.argmax); labels_out (optional, int32 [M])
 * receives it for a kept row and 255 for an ignored one.  With K kept rows:
 *   *loss = (1/K) sum over kept rows of (logsumexp(row) - max(row)), 0 if K = 0
 *           (CrossEntropyLoss(ignore_index=255) of the rows against their own
 *           argmax; the reference logs 0 when every point is ignored),
 *   dlogits[r][c] += scale / K (softmax(row)[c] - [c == label])  on kept rows,
 *   *kept_out = K (optional, int32).
 * The gradient is ADDED (row stride ldd >= ncls): the no-GT rows already hold
 * the adversarial term's gradient.  Ignored rows, columns >= ncls, and
 * everything when K = 0 are not written at all.  K and the loss are summed in a
 * fixed order (no floating-point atomics): the same inputs leave the same bits.
 * Two launches, no host synchronisation; every workspace slot is written before
 * it is read in each call, so the workspace needs no zeroing, ever.  Calls
 * sharing a workspace must be ordered on one stream. */
size_t pcadv_row_semi_ce_workspace_bytes(int M);
int pcadv_row_semi_ce(const float* logits, int64_t ld, const float* d_out, int M, int ncls,
                      float semi_th, float scale, float* dlogits, int64_t ldd,
                      int32_t* labels_out, float* loss, int32_t* kept_out, void* workspace,
                      size_t workspace_bytes, hipStream_t stream);

/* ---- StackDiscNet of run_training_seg_stack ----------------------------------
 * (models/discriminator.py:139-175, utils/trainer.py:1028-1216.)
 * Additions to ABI 11 (nothing existing changes).
 *
 * The layout of pcadv_pwdisc_args: logits [n0 + n1][ncls] (row stride ld,
 * 2 <= ncls <= 64), rows [0, n0) through transform t0 and rows [n0, n0 + n1)
 * through t1 (the reference: softmax and log_softmax, trainer.py:1082,1095).
 * w[i] / b[i]: conv1..conv4 as there, and conv5 ([num_shapes][1], [num_shapes];
 * 2 <= num_shapes <= 32).  The activations are LeakyReLU(0.2).
 *
 * pcadv_stackdisc_forward, one launch, per row:
 *   m        = max over the 128 channels of lrelu(conv4(..lrelu(conv1(x)))),
 *              exact f32 MFMAs in k order; argc its channel (first on ties),
 *   S[s]     = w5[s] m + b5[s]          (shape_logits [n0 + n1][num_shapes], optional),
 *   d_out    = out / (out + 1), out = logsumexp_s S (less the row maximum).
 * With losses != NULL (5 floats) also, BCE as torch's binary_cross_entropy
 * (-(y max(log x, -100) + (1 - y) max(log(1 - x), -100)), derivative
 * (x - y) / max(x (1 - x), 1e-12), any real label y):
 *   losses[0] = loss_adv = mean over the no-GT rows of BCE(d_out, 1),
 *   losses[2] = 0.5 mean over the GT rows against soft labels of U(0.7, 1.05),
 *   losses[3] = 0.5 mean over the no-GT rows against soft labels of U(0, 0.305),
 *   losses[1] = loss_D = losses[2] + losses[3],
 *   losses[4] = loss_D_shape = mean over the GT rows of CrossEntropy(S,
 *               shape_label[row / pts_per_cloud]), unscaled,
 *   dm_d[n0 + n1]  = d(loss_D + lambda_disc_shape loss_D_shape) / dm,
 *   dm_adv[n1]     = d loss_adv / dm (optional),
 *   dw[4] / db[4]  = conv5's gradients of loss_D + lambda_disc_shape loss_D_shape,
 *   *bad_rows      = the number of rows whose d_out is not in [0, 1] (NaN
 *                    included; torch's BCELoss raises there).  Written by every
 *                    forward with losses; such rows' loss and derivative values
 *                    are unspecified, and nothing faults.
 * The soft labels are soft0 / soft1 or drawn with pcadv_pwdisc_forward's Philox
 * keys (rng_seed, *step_count, row): the same labels for the same seed.  n0 must
 * be a multiple of pts_per_cloud; shape_label holds n0 / pts_per_cloud int32
 * (a label outside [0, num_shapes) selects no class).  All sums run in a fixed
 * order.  The workspace's first 256 bytes are the ticket, as above.
 *
 * pcadv_stackdisc_backward, one launch and the fixed-order finish: recomputes
 * x1..x3, routes a unit gradient from channel argc through the masks
 * (y > 0 ? 1 : 0.2, the arg-max channel's own mask on m included; no row is
 * dead) and writes dw[0..3] / db[0..3] = the gradients of sum_row dm_d[row]
 * m[row], and with dlogits and dm_adv the gradient of lambda_adv sum_j
 * dm_adv[j] m[n0 + j] through t1 into rows [n0, n0 + n1) of dlogits.  Reads m,
 * argc; x_out as in pcadv_pwdisc_backward. */
typedef struct pcadv_stackdisc_args {
  const float* logits;
  int64_t ld;
  int ncls, n0, n1, t0, t1;
  const float* w[5];
  const float* b[5];
  int num_shapes;
  const int32_t* shape_label;
  int pts_per_cloud;
  float lambda_disc_shape;
  float* m;
  int32_t* argc;
  float* d_out;
  float* shape_logits;
  float* losses;
  const float* soft0;
  const float* soft1;
  float* soft_out;
  uint64_t rng_seed;
  const int32_t* step_count;
  float* dm_d;
  float* dm_adv;
  int32_t* bad_rows;
  float lambda_adv;
  float* dw[5];
  float* db[5];
  float* dlogits;
  int64_t ldd;
  int max_workgroups;
  void* workspace;
  size_t workspace_bytes;
  float* x_out;
} pcadv_stackdisc_args;
size_t pcadv_stackdisc_workspace_bytes(int64_t rows, int max_workgroups);
int pcadv_stackdisc_forward(const pcadv_stackdisc_args* args, hipStream_t stream);
int pcadv_stackdisc_backward(const pcadv_stackdisc_args* args, hipStream_t stream);

/* ---- The semi-supervised term of the stacked loops ---------------------------
 * (run_training_seg_stack_semi, run_training_seg_stack_regulization_semi:
 * utils/trainer.py:1516-1530, 1747-1761.)  Additions to ABI 11 (nothing
 * existing changes; pcadv_stackdisc_args is as above).
 *
 * pcadv_stackdisc_forward_semi is pcadv_stackdisc_forward (the same launch
 * count, every output above the same bits) with the term's scan in the same
 * kernel.  losses must not be NULL.  A no-GT row is KEPT iff
 * !(d_out[row] <= semi_th), with the d_out value the call stores (equality is
 * ignored, a NaN is kept).  With K kept rows:
 *   *loss_semi = (1/K) sum over kept rows of (logsumexp(row) - max(row)) of the
 *                row's raw logits, 0 if K = 0 (n1 = 0 included),
 *   *kept      = K (int32).
 * The row term is log1p of the exp sum over the classes other than the first
 * maximum; the workgroups' sums are f64, combined in workgroup order: no
 * floating-point atomics, the same inputs leave the same bits.  The workspace is
 * pcadv_stackdisc_workspace_bytes'; nothing needs zeroing between calls.
 *
 * pcadv_row_semi_apply is pcadv_row_semi_ce's gradient pass for a caller that
 * holds K on the device: one launch, no workspace.  logits [M][ncls] (row
 * stride ld), d_out [M], *kept = K.  With K > 0,
 *   dlogits[r][c] += scale / K (softmax(row)[c] - [c == label])
 * on the rows with !(d_out[r] <= semi_th), label the FIRST index of the row's
 * maximum: the bits pcadv_row_semi_ce adds for the same K.  labels_out
 * (optional, int32 [M]) is written for every row: the label of a kept row, 255
 * for an ignored one; with K <= 0 no row counts as kept (every label 255) and
 * nothing else is written.  Ignored rows and columns >= ncls are never written.
 * 16-byte accesses where both bases and strides allow. */
typedef struct pcadv_stackdisc_semi {
  float semi_th;
  float* loss_semi;
  int32_t* kept;
} pcadv_stackdisc_semi;
int pcadv_stackdisc_forward_semi(const pcadv_stackdisc_args* args, const pcadv_stackdisc_semi* semi,
                                 hipStream_t stream);
int pcadv_row_semi_apply(const float* logits, int64_t ld, const float* d_out, int M, int ncls,
                         float semi_th, float scale, const int32_t* kept, float* dlogits,
                         int64_t ldd, int32_t* labels_out, hipStream_t stream);

/* ---- T-Net glue of the regularised seg generator ----------------------------
 * (PointNetSeg_regulization, models/pointnet.py:205-259;
 * run_training_seg_stack_regulization, utils/trainer.py:1218-1429.)  Additive
 * to ABI 11.  Rows are points, point-major; C clouds of Npts points each (any
 * C, Npts >= 0; zero rows: no launch); k in {3, 128}; T [C][k][k] dense.  Every
 * sum runs in a fixed order (no atomics): results are bitwise reproducible.
 * k = 128 on exact f32 MFMAs, k = 3 on VALU FMAs.
 *
 * pcadv_cloud_xform_fwd: y[c][n][j] = sum_i x[c][n][i] T[c][i][j]; x has row
 * stride ldx >= k, y row stride ldy >= k (floats). */
int pcadv_cloud_xform_fwd(const float* x, int64_t ldx, const float* T, float* y, int64_t ldy,
                          int C, int Npts, int k, hipStream_t stream);

/* Its backward from dy (row stride lddy), x and T:
 *   dT[c][i][j] (+)= sum_n x[c][n][i] dy[c][n][j]   (NULL: skipped; accumulate=1 adds)
 *   dx[c][n][i] += (sum_j dy[c][n][j] T[c][i][j] + add[c][n][i]) * [x[c][n][i] > 0 if relu_x]
 * dx (NULL: skipped) has row stride lddx and always accumulates; add is a
 * dense [C*Npts][k] addend or NULL (a second consumer's gradient of x, summed
 * before the one mask).  With dx and k = 128, T must be 16-byte aligned. */
int pcadv_cloud_xform_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                          const float* T, float* dT, int accumulate, float* dx, int64_t lddx,
                          const float* add, int relu_x, int C, int Npts, int k,
                          hipStream_t stream);

/* MSELoss()(T T^T, I) per batch (utils/trainer.py:1280-1281,1301-1302): the
 * first B0 clouds are group 0, the other C - B0 group 1 (B0 = C: one group,
 * loss[1] = 0).  loss[g] = sum over the group's clouds and i, j of
 * (T T^T - I)^2 / (B_g k^2); dT[c] += scale (4 / (B_g k^2)) (T_c T_c^T - I) T_c
 * (dT NULL: loss only; an element whose gradient is 0 is not written, so
 * T = I leaves dT bitwise as it was).  k = 3 or a multiple of 4 up to 128;
 * 1 <= B0 <= C; workspace: 4 C floats. */
int pcadv_tnet_mse_reg(const float* T, int C, int B0, int k, float scale, float* loss, float* dT,
                       float* workspace, hipStream_t stream);

/* ---- The dual discriminator of run_training_seg_dual ------------------------
 * (BaseDiscNet / PointDiscNet / ShapeDiscNet, models/discriminator.py:82-137;
 * utils/trainer.py:2123-2382.)  Additive to ABI 11.  The nets' wide layers run
 * on pcadv_gemm (precise = 1, no activation) and pcadv_gemm_wgrad, the shape
 * head on pcadv_conv_max_x3 (relu = 0: LeakyReLU is increasing, so it commutes
 * with the max and keeps the arg-max) and pcadv_linear_*; these entries are
 * what the engine lacks.  Every sum runs in a fixed order (no atomics).
 *
 * pcadv_dual_input: x0[r][0..ncls) (dense, [n0 + n1][ncls]) = transform t0 of
 * logits row r < n0, t1 of the other rows (PCADV_PWD_*; row stride ld,
 * 2 <= ncls <= 64).  pcadv_dual_input_bwd: its backward on n rows of one
 * transform t: from x0 (the transform's OUTPUT rows) and dx0 (both dense
 * [n][ncls]) into dlogits (row stride ldd; columns >= ncls are not written). */
int pcadv_dual_input(const float* logits, int64_t ld, int ncls, int64_t n0, int64_t n1, int t0,
                     int t1, float* x0, hipStream_t stream);
int pcadv_dual_input_bwd(const float* x0, const float* dx0, int ncls, int64_t n, int t,
                         float* dlogits, int64_t ldd, hipStream_t stream);

/* LeakyReLU(0.2) in place over n floats, and its derivative applied to a data
 * gradient: d[i] *= (y[i] > 0 ? 1 : 0.2), y the activation's OUTPUT (slope 0.2
 * at exactly 0, as the backward of torch's in-place LeakyReLU). */
int pcadv_lrelu_fwd(float* y, int64_t n, hipStream_t stream);
int pcadv_lrelu_bwd(float* d, const float* y, int64_t n, hipStream_t stream);

/* PointDiscNet's tail on y [n0 + n1][C] (its last layer's output after the
 * LeakyReLU; C % 4 == 0, 16-B aligned): out[row] = max over the C channels,
 * argc[row] its channel (the first on ties).  With losses != NULL (4 floats)
 * also the three BCE-with-logits terms exactly as pcadv_pwdisc_forward defines
 * them (losses[0] = loss_adv, [1] = loss_D_point = [2] + [3]), the labels
 * soft0 / soft1 or drawn with the same Philox keys (rng_seed, *step_count,
 * row), dout_d [n0 + n1], dout_adv [n1] (optional), and the top gradients of
 * the backward chains, one-hot at argc times the winner's LeakyReLU slope:
 *   dz_d   [n0 + n1][C] (optional) = dout_d[row] slope,
 *   dz_adv [n1][C]      (optional) = lambda_adv dout_adv[j] slope.
 * max_workgroups: 0, or a cap on the grid (tests).  The workspace needs no
 * zeroing. */
typedef struct pcadv_dual_tail_args {
  const float* y;
  int C;
  int64_t n0, n1;
  float* out;
  int32_t* argc;
  float* losses;
  const float* soft0;
  const float* soft1;
  float* soft_out;
  uint64_t rng_seed;
  const int32_t* step_count;
  float* dout_d;
  float* dout_adv;
  float lambda_adv;
  float* dz_d;
  float* dz_adv;
  int max_workgroups;
  void* workspace;
  size_t workspace_bytes;
} pcadv_dual_tail_args;
size_t pcadv_dual_point_tail_workspace_bytes(int64_t rows);
int pcadv_dual_point_tail(const pcadv_dual_tail_args* args, hipStream_t stream);

/* Plain SGD over a flat range (torch.optim.SGD without momentum, dampening or
 * weight decay): p[i] -= lr g[i]; with acc != NULL first acc[i] += g[i] and the
 * update takes acc[i] (a .grad that is never cleared: PointDiscNet's in
 * run_training_seg_dual).  Any n and alignment (16-B stores where p, g and acc
 * are 16-B aligned); product and difference rounded separately. */
int pcadv_sgd(float* p, const float* g, float* acc, int64_t n, float lr, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCADV_H */
