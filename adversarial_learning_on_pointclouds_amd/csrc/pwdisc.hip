// PointwiseDiscNet (models/discriminator.py:53-79) fused for the adversarial
// segmentation step (utils/trainer.py:849-1026): per point a softmax /
// log_softmax of the generator's logits, conv1..conv4 + ReLU (ncls -> 64 -> 64
// -> 64 -> 128) on the exact f32 MFMA, the max over the 128 channels and the
// three BCE-with-logits terms of the iteration; the backward recomputes x1..x3
// and forms every weight gradient and the no-GT rows' input gradient.
//
// Tiles of 64 points, persistent workgroups of 4 waves.  Every MFMA runs in k
// order (mfma_rows_x_wt), and the backward calls the same device functions as
// the forward, so its recomputed activations (and ReLU masks) are the forward's
// bits.  No floating-point atomics: the loss terms and the weight-gradient
// slabs are summed in a fixed order.
//
// StackDiscNet (models/discriminator.py:139-175, run_training_seg_stack) shares
// all of it: the layer functions and the backward are templates on the
// activation (ReLU here, LeakyReLU(0.2) there), and k_stk_fwd adds conv5, the
// logsumexp, out / (out + 1), the BCE and shape terms and conv5's gradients
// behind the channel max (second half of this file).
#include <cmath>
#include <type_traits>

#include "common.h"

namespace pcadv {

namespace {

constexpr int PD_T = 256;     // threads per workgroup
constexpr int PD_ROWS = 64;   // points per tile
constexpr int PD_S = S64;     // LDS row stride of the 64-wide buffers
constexpr int PD_S4 = S128;   // ... of conv4's 128-wide output
constexpr int PD_FWD_WG = 512;  // default persistent grids: 2 (forward) and 1
constexpr int PD_BWD_WG = 256;  // (backward) workgroups per CU (LDS bound)

// one workgroup's weight-gradient slab (floats): dW1 padded to K = 64
constexpr int SL_W1 = 0, SL_W2 = 4096, SL_W3 = 8192, SL_W4 = 12288;
constexpr int SL_B1 = 20480, SL_B2 = 20544, SL_B3 = 20608, SL_B4 = 20672;
constexpr int SL_N = 20800;
constexpr size_t WS_HEAD = 256;  // the ticket, alone on its line

struct PwdNet {
  const float* logits;
  long long ld;
  int ncls, n0, n1, t0, t1;
  const float* w[4];
  const float* b[4];
};

struct PwdFwdOut {
  float* out;
  int32_t* argc;
  float* losses;        // [4] or NULL: no loss terms
  const float* soft0;   // explicit labels (parity mode) or NULL: drawn here
  const float* soft1;
  float* soft_out;      // optional: the labels used
  uint64_t seed;
  const int32_t* step;
  float* dout_d;
  float* dout_adv;
  unsigned* ticket;
  float* partial;       // [ntiles][3]
};

struct PwdBwdArgs {
  const float* out;
  const int32_t* argc;
  const float* dout_d;
  const float* dout_adv;  // NULL: no input gradient
  float lambda_adv;
  float* dlogits;
  long long ldd;
  float* slabs;
  float* x_out;  // optional [3][M][64]: the recomputed x1..x3 (tests)
};

// The transformed input tile x0 [64][64] (columns >= ncls and rows >= M zero):
// four lanes per row, column c = q + 4 i.  The row max and the exp sum combine
// the four lanes' partials by xor shuffles (commutative: every lane holds the
// same bits), in one fixed order.
// SEMI (k_stk_fwd<true>): es receives the row's sum of exp(x - max) over the
// classes OTHER than the first maximum (semi.hip's sm_row), so that the row's
// pseudo-label loss logsumexp - max = log1p(es) does not cancel on a confident
// row; the same value in the row's four lanes.
template <bool SEMI>
__device__ __forceinline__ void pwd_load_x0_t(const PwdNet& p, int r0, int tid, float* x0,
                                              float& es) {
  const int row = tid >> 2, q = tid & 3;
  const long long g = (long long)r0 + row;
  const bool in = g < (long long)p.n0 + p.n1;
  const int tr = g < p.n0 ? p.t0 : p.t1;
  const float* src = p.logits + (size_t)(in ? g : 0) * p.ld;
  float v[16];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = q + 4 * i;
    const bool ok = in && c < p.ncls;
    v[i] = ok ? src[c] : -INFINITY;
    mx = fmaxf(mx, v[i]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 1));
  mx = fmaxf(mx, __shfl_xor(mx, 2));
  if (!in) mx = 0.f;
  float e[16];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    e[i] = (in && q + 4 * i < p.ncls) ? expf(v[i] - mx) : 0.f;
    s += e[i];
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  if constexpr (SEMI) {
    int bi = 64;  // the first class at the maximum: the lane's, then the row's
#pragma unroll
    for (int i = 15; i >= 0; --i)
      if (v[i] == mx) bi = q + 4 * i;
    bi = min(bi, __shfl_xor(bi, 1));
    bi = min(bi, __shfl_xor(bi, 2));
    es = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) es += q + 4 * i != bi ? e[i] : 0.f;
    es += __shfl_xor(es, 1);
    es += __shfl_xor(es, 2);
  }
  const float lg = logf(s);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = q + 4 * i;
    float y = v[i];
    if (tr == PCADV_PWD_SOFTMAX) y = e[i] / s;
    if (tr == PCADV_PWD_LOG_SOFTMAX) y = (v[i] - mx) - lg;
    x0[row * PD_S + c] = (in && c < p.ncls) ? y : 0.f;
  }
}
__device__ __forceinline__ void pwd_load_x0(const PwdNet& p, int r0, int tid, float* x0) {
  float es;
  pwd_load_x0_t<false>(p, r0, tid, x0, es);
}

// B fragments of W [O][ldw] for output columns [oc, oc + 32), k < kmax (zero
// past it: conv1's ncls columns padded to the MFMA's K = 64)
template <bool PAD>
__device__ __forceinline__ void pwd_frags(const float* __restrict__ w, int ldw, int kmax, int oc,
                                          int lane, f32x4 (&bf)[8]) {
  const int r = lane & 31, h = lane >> 5;
  const float* row = w + (size_t)(oc + r) * ldw;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    if constexpr (PAD) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 8 * g + 4 * h + j;
        bf[g][j] = k < kmax ? row[k] : 0.f;
      }
    } else {
      bf[g] = *reinterpret_cast<const f32x4*>(row + 8 * g + 4 * h);
    }
  }
}

// B fragments of the transposed product dz W (W [64][ldw]): output columns
// [oc, oc + 32) of W's columns (zero from ncols on), k over W's 64 rows
__device__ __forceinline__ void pwd_frags_t(const float* __restrict__ w, int ldw, int ncols, int oc,
                                            int lane, f32x4 (&bf)[8]) {
  const int r = lane & 31, h = lane >> 5;
  const bool ok = oc + r < ncols;
  const float* col = w + (ok ? oc + r : 0);
#pragma unroll
  for (int g = 0; g < 8; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[g][j] = ok ? col[(size_t)(8 * g + 4 * h + j) * ldw] : 0.f;
}

// one 64 -> 64 layer + activation (ReLU, or the stacked discriminator's
// LeakyReLU(0.2)) of the tile: wave = (row tile wave >> 1, column tile wave & 1)
template <int ACT>
__device__ __forceinline__ void pwd_layer64(const float* in, float* out, const f32x4 (&bf)[8],
                                            float bias, int wave, int lane) {
  const int r = lane & 31, oc = 32 * (wave & 1), rt = wave >> 1;
  f32x16 acc = {};
  acc = mfma_rows_x_wt<64>(in + 32 * rt * PD_S, PD_S, bf, acc, lane);
#pragma unroll
  for (int e = 0; e < 16; ++e)
    out[(32 * rt + acc_row(e, lane)) * PD_S + oc + r] = act_fwd(acc[e] + bias, ACT);
}

// x0 -> x1 -> x2 -> x3 (each [64][PD_S]); the caller has synchronised after
// writing x0.  Ends with a barrier: x3 is readable by every wave.
template <int ACT>
__device__ __forceinline__ void pwd_chain3(const PwdNet& p, float* x0, float* x1, float* x2,
                                           float* x3, int wave, int lane) {
  const int r = lane & 31, oc = 32 * (wave & 1);
  f32x4 bf[8];
  pwd_frags<true>(p.w[0], p.ncls, p.ncls, oc, lane, bf);
  pwd_layer64<ACT>(x0, x1, bf, p.b[0][oc + r], wave, lane);
  pwd_frags<false>(p.w[1], 64, 64, oc, lane, bf);
  __syncthreads();
  pwd_layer64<ACT>(x1, x2, bf, p.b[1][oc + r], wave, lane);
  pwd_frags<false>(p.w[2], 64, 64, oc, lane, bf);
  __syncthreads();
  pwd_layer64<ACT>(x2, x3, bf, p.b[2][oc + r], wave, lane);
  __syncthreads();
}

// conv4 + activation of the tile x3 into y4 [64][PD_S4] (wave = 32 of the 128
// channels, both row tiles), a barrier, then the max over the channels, first
// index on ties: 4 lanes x 32 channels per row (row = tid >> 2).  All four
// lanes of a row end with the same (best, bi).
template <int ACT>
__device__ __forceinline__ void pwd_conv4_max(const PwdNet& p, const float* x3, float* y4, int tid,
                                              float& best, int& bi) {
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31;
  {
    f32x4 bf[8];
    pwd_frags<false>(p.w[3], 64, 64, 32 * wave, lane, bf);
    const float bias = p.b[3][32 * wave + r];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 acc = {};
      acc = mfma_rows_x_wt<64>(x3 + 32 * t * PD_S, PD_S, bf, acc, lane);
#pragma unroll
      for (int e = 0; e < 16; ++e)
        y4[(32 * t + acc_row(e, lane)) * PD_S4 + 32 * wave + r] = act_fwd(acc[e] + bias, ACT);
    }
  }
  __syncthreads();
  const int row = tid >> 2, q = tid & 3;
  const float* y = &y4[row * PD_S4 + 32 * q];
  best = y[0];
  bi = 32 * q;
#pragma unroll 8
  for (int c = 1; c < 32; ++c) {
    const float v = y[c];
    if (beats(v, best)) { best = v; bi = 32 * q + c; }
  }
#pragma unroll
  for (int m = 1; m < 4; m <<= 1) {
    const float ov = __shfl_xor(best, m);
    const int oi = __shfl_xor(bi, m);
    const bool up = q & m;  // this lane holds the higher channels
    const float lo_v = up ? ov : best, hi_v = up ? best : ov;
    const int lo_i = up ? oi : bi, hi_i = up ? bi : oi;
    const bool t = beats(hi_v, lo_v);
    best = t ? hi_v : lo_v;
    bi = t ? hi_i : lo_i;
  }
}

struct PwdFwdLds {
  alignas(16) float xa[PD_ROWS * PD_S];
  alignas(16) float xb[PD_ROWS * PD_S];
  alignas(16) float y4[PD_ROWS * PD_S4];
  float lt[3][PD_ROWS];
  int last;
};

__global__ void __launch_bounds__(PD_T, 2) k_pwd_fwd(PwdNet p, PwdFwdOut o, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PwdFwdLds& L = *reinterpret_cast<PwdFwdLds*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long M = (long long)p.n0 + p.n1;
  uint32_t stepv = 0;
  if (o.losses && o.step) stepv = (uint32_t)*o.step;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * PD_ROWS;
    pwd_load_x0(p, r0, tid, L.xa);
    __syncthreads();
    // xa -> xb -> xa -> xb
    pwd_chain3<ACT_RELU>(p, L.xa, L.xb, L.xa, L.xb, wave, lane);
    {
      const int row = tid >> 2, q = tid & 3;
      float best;
      int bi;
      pwd_conv4_max<ACT_RELU>(p, L.xb, L.y4, tid, best, bi);
      const long long g = (long long)r0 + row;
      if (q == 0) {
        float l0 = 0.f, l1 = 0.f, l2 = 0.f;
        if (g < M) {
          o.out[g] = best;
          o.argc[g] = bi;
          if (o.losses) {
            // make_D_label(random=True), one label per point (utils/utils.py:22-31)
            const float z = best;
            const float sg = 1.f / (1.f + expf(-z));
            const float sp = log1pf(expf(-fabsf(z)));
            if (g < p.n0) {
              const float y0 = o.soft0 ? o.soft0[g]
                                       : 0.7f + 0.35f * rng_uniform(o.seed, stepv, RNG_LABEL_GT,
                                                                    (uint32_t)g);
              l1 = fmaxf(z, 0.f) - z * y0 + sp;
              o.dout_d[g] = 0.5f * (sg - y0) / (float)p.n0;
              if (o.soft_out) o.soft_out[g] = y0;
            } else {
              const long long j = g - p.n0;
              const float y1 = o.soft1 ? o.soft1[j]
                                       : 0.305f * rng_uniform(o.seed, stepv, RNG_LABEL_NOGT,
                                                              (uint32_t)j);
              l2 = fmaxf(z, 0.f) - z * y1 + sp;
              l0 = fmaxf(z, 0.f) - z + sp;  // against label 1 (the generator's term)
              o.dout_d[g] = 0.5f * (sg - y1) / (float)p.n1;
              if (o.dout_adv) o.dout_adv[j] = (sg - 1.f) / (float)p.n1;
              if (o.soft_out) o.soft_out[g] = y1;
            }
          }
        }
        L.lt[0][row] = l0;
        L.lt[1][row] = l1;
        L.lt[2][row] = l2;
      }
    }
    __syncthreads();
    if (o.losses && wave == 0) {
      const float a0 = wave_sum(L.lt[0][lane]), a1 = wave_sum(L.lt[1][lane]),
                  a2 = wave_sum(L.lt[2][lane]);
      if (lane == 0) {
        o.partial[3 * (size_t)tile + 0] = a0;
        o.partial[3 * (size_t)tile + 1] = a1;
        o.partial[3 * (size_t)tile + 2] = a2;
      }
    }
    // the next tile's x0 goes to xa (last read before conv4's barrier), lt is
    // rewritten after three more barriers
  }
  if (!o.losses) return;
  // the last workgroup to arrive sums the tiles' terms in tile order (whichever
  // workgroup that is, the order and so the bits are the same)
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const unsigned t = atomicAdd(o.ticket, 1u);
    L.last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!L.last || wave != 0) return;
  __threadfence();
  float a[3] = {0.f, 0.f, 0.f};
  for (int t = lane; t < ntiles; t += 64)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      a[k] += __uint_as_float(__hip_atomic_load(
          reinterpret_cast<const unsigned*>(o.partial) + 3 * (size_t)t + k, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = wave_sum(a[k]);
  if (lane == 0) {
    const float adv = p.n1 ? a[0] / (float)p.n1 : 0.f;
    const float dgt = p.n0 ? 0.5f * (a[1] / (float)p.n0) : 0.f;
    const float dng = p.n1 ? 0.5f * (a[2] / (float)p.n1) : 0.f;
    o.losses[0] = adv;        // loss_adv
    o.losses[1] = dgt + dng;  // loss_D
    o.losses[2] = dgt;
    o.losses[3] = dng;
    *o.ticket = 0u;  // ready for the next launch
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
struct PwdBwdLds {
  alignas(16) float x[4][PD_ROWS * PD_S];  // x0..x3
  alignas(16) float da[PD_ROWS * PD_S];    // unit gradients, alternating
  alignas(16) float db[PD_ROWS * PD_S];
  float sv[PD_ROWS];  // D's dout of the row (0: dead row or past the end)
  float av[PD_ROWS];  // lambda_adv dout_adv (no-GT rows)
  int ac[PD_ROWS];    // argc, -1 for a dead row
};

// acc += (s dz)^T x over the tile's rows in row order: 32 x 32 (o, k) tile
__device__ __forceinline__ f32x16 pwd_wgrad(const float* dz, const float* sv, const float* x,
                                            int o0, int k0, f32x16 acc, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll 8
  for (int t = 0; t < 32; ++t) {
    const int row = 2 * t + h;
    acc = mfma32(dz[row * PD_S + o0 + r] * sv[row], x[row * PD_S + k0 + r], acc);
  }
  return acc;
}

// the data gradient of one layer: out = (in W) masked by the activation's
// derivative at y (relu: 1 / 0, leaky relu: 1 / 0.2; y = NULL: none)
template <int ACT>
__device__ __forceinline__ void pwd_dgrad(const float* in, float* out, const float* y,
                                          const f32x4 (&bf)[8], int wave, int lane) {
  const int r = lane & 31, oc = 32 * (wave & 1), rt = wave >> 1;
  f32x16 acc = {};
  acc = mfma_rows_x_wt<64>(in + 32 * rt * PD_S, PD_S, bf, acc, lane);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = (32 * rt + acc_row(e, lane)) * PD_S + oc + r;
    if constexpr (ACT == ACT_RELU)
      out[i] = (!y || y[i] > 0.f) ? acc[e] : 0.f;
    else
      out[i] = (!y || y[i] > 0.f) ? acc[e] : 0.2f * acc[e];
  }
}

// The whole backward of a row is linear in one scalar, so one unit chain per
// row (gradient 1 at channel argc) serves both uses: the weight gradients scale
// it by D's dout (sv), the no-GT rows' input gradient by lambda_adv dout_adv.
// ACT_LRELU (the stacked discriminator): no row is dead, every mask is 1 / 0.2,
// and the arg-max channel's own mask on out scales the row's two scalars.
template <int ACT>
__global__ void __launch_bounds__(PD_T, 1) k_pwd_bwd(PwdNet p, PwdBwdArgs a, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PwdBwdLds& L = *reinterpret_cast<PwdBwdLds*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31;
  const long long M = (long long)p.n0 + p.n1;
  const int wo = 32 * (wave >> 1), wk = 32 * (wave & 1);  // this wave's (o, k) tile
  f32x16 g1 = {}, g2 = {}, g3 = {}, g4a = {}, g4b = {};
  float bsum = 0.f;  // wave 0: db3, wave 1: db2, wave 2: db1 (lane = channel)
  float b4sum = 0.f;  // waves 2, 3: db4 of channel tid - 128
  const bool want_dx = a.dlogits && a.dout_adv;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * PD_ROWS;
    pwd_load_x0(p, r0, tid, L.x[0]);
    if (tid < PD_ROWS) {
      const long long g = (long long)r0 + tid;
      const bool pos = g < M && a.out[g] > 0.f;
      // relu'(0) = 0: a dead row gets nothing; a leaky row gets 0.2 of it
      const bool live = ACT == ACT_RELU ? pos : g < M;
      const float top = (ACT == ACT_RELU || pos) ? 1.f : 0.2f;
      L.sv[tid] = live ? top * a.dout_d[g] : 0.f;
      L.av[tid] =
          (live && want_dx && g >= p.n0) ? top * (a.lambda_adv * a.dout_adv[g - p.n0]) : 0.f;
      L.ac[tid] = live ? (a.argc[g] & 127) : -1;  // a channel of conv4 whatever the buffer holds
    }
    __syncthreads();
    pwd_chain3<ACT>(p, L.x[0], L.x[1], L.x[2], L.x[3], wave, lane);
    if (a.x_out) {  // uniform over the grid
#pragma unroll 4
      for (int j = 0; j < PD_ROWS * 64 / PD_T; ++j) {
        const int e = tid + PD_T * j, row = e >> 6, k = e & 63;
        const long long g = (long long)r0 + row;
        if (g < M)
          for (int l = 0; l < 3; ++l)
            a.x_out[((size_t)l * M + g) * 64 + k] = L.x[l + 1][row * PD_S + k];
      }
    }
    // conv4: the gradient reaches channel argc only.  dW4 += onehot(argc) s x3
    {
      const int o = 32 * wave + r, h = lane >> 5;
#pragma unroll 8
      for (int t = 0; t < 32; ++t) {
        const int row = 2 * t + h;
        const float av = L.ac[row] == o ? L.sv[row] : 0.f;
        g4a = mfma32(av, L.x[3][row * PD_S + r], g4a);
        g4b = mfma32(av, L.x[3][row * PD_S + 32 + r], g4b);
      }
    }
    if (wave >= 2) {
      const int c = tid - 128;
      for (int row = 0; row < PD_ROWS; ++row) b4sum += L.ac[row] == c ? L.sv[row] : 0.f;
    }
    // unit dz3 = W4[argc] relu'(x3)
#pragma unroll
    for (int j = 0; j < PD_ROWS * 64 / PD_T; ++j) {
      const int e = tid + PD_T * j, row = e >> 6, k = e & 63;
      const int c = L.ac[row];
      if constexpr (ACT == ACT_RELU) {
        L.da[row * PD_S + k] = (c >= 0 && L.x[3][row * PD_S + k] > 0.f) ? p.w[3][c * 64 + k] : 0.f;
      } else {
        const float w = c >= 0 ? p.w[3][c * 64 + k] : 0.f;
        L.da[row * PD_S + k] = L.x[3][row * PD_S + k] > 0.f ? w : 0.2f * w;
      }
    }
    f32x4 bf[8];
    pwd_frags_t(p.w[2], 64, 64, wk, lane, bf);
    __syncthreads();
    // conv3
    g3 = pwd_wgrad(L.da, L.sv, L.x[2], wo, wk, g3, lane);
    if (wave == 0)
      for (int row = 0; row < PD_ROWS; ++row) bsum += L.sv[row] * L.da[row * PD_S + lane];
    pwd_dgrad<ACT>(L.da, L.db, L.x[2], bf, wave, lane);
    pwd_frags_t(p.w[1], 64, 64, wk, lane, bf);
    __syncthreads();
    // conv2
    g2 = pwd_wgrad(L.db, L.sv, L.x[1], wo, wk, g2, lane);
    if (wave == 1)
      for (int row = 0; row < PD_ROWS; ++row) bsum += L.sv[row] * L.db[row * PD_S + lane];
    pwd_dgrad<ACT>(L.db, L.da, L.x[1], bf, wave, lane);
    __syncthreads();
    // conv1
    g1 = pwd_wgrad(L.da, L.sv, L.x[0], wo, wk, g1, lane);
    if (wave == 2)
      for (int row = 0; row < PD_ROWS; ++row) bsum += L.sv[row] * L.da[row * PD_S + lane];
    const bool dx_tile = want_dx && (long long)r0 + PD_ROWS > p.n0;  // uniform over the workgroup
    if (dx_tile) {
      pwd_frags_t(p.w[0], p.ncls, p.ncls, wk, lane, bf);
      pwd_dgrad<ACT>(L.da, L.db, nullptr, bf, wave, lane);
    }
    __syncthreads();
    if (dx_tile) {  // through the input transform, written to the no-GT rows only
      const int row = tid >> 2, q = tid & 3;
      const long long g = (long long)r0 + row;
      const float s = L.av[row];
      float dy[16], y[16];
      float sum = 0.f, dot = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = q + 4 * i;
        dy[i] = c < p.ncls ? L.db[row * PD_S + c] * s : 0.f;
        y[i] = L.x[0][row * PD_S + c];
        sum += dy[i];
        dot += dy[i] * y[i];
      }
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      dot += __shfl_xor(dot, 1);
      dot += __shfl_xor(dot, 2);
      if (g >= p.n0 && g < M) {
        float* dst = a.dlogits + (size_t)g * a.ldd;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int c = q + 4 * i;
          float d = dy[i];
          if (p.t1 == PCADV_PWD_LOG_SOFTMAX) d = dy[i] - expf(y[i]) * sum;
          if (p.t1 == PCADV_PWD_SOFTMAX) d = y[i] * (dy[i] - dot);
          if (c < p.ncls) dst[c] = d;
        }
      }
    }
    __syncthreads();  // x[0], sv and the gradient buffers are free for the next tile
  }
  float* slab = a.slabs + (size_t)blockIdx.x * SL_N;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int ro = acc_row(e, lane);
    slab[SL_W1 + (wo + ro) * 64 + wk + r] = g1[e];
    slab[SL_W2 + (wo + ro) * 64 + wk + r] = g2[e];
    slab[SL_W3 + (wo + ro) * 64 + wk + r] = g3[e];
    slab[SL_W4 + (32 * wave + ro) * 64 + r] = g4a[e];
    slab[SL_W4 + (32 * wave + ro) * 64 + 32 + r] = g4b[e];
  }
  if (wave == 0) slab[SL_B3 + lane] = bsum;
  if (wave == 1) slab[SL_B2 + lane] = bsum;
  if (wave == 2) slab[SL_B1 + lane] = bsum;
  if (wave >= 2) slab[SL_B4 + tid - 128] = b4sum;
}

struct PwdGrads {
  float* dw[4];
  float* db[4];
};

// the slabs summed in workgroup order
__global__ void __launch_bounds__(256) k_pwd_bwd_finish(const float* __restrict__ slabs, int nslabs,
                                                        int ncls, PwdGrads g) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= SL_N) return;
  float s = 0.f;
  for (int i = 0; i < nslabs; ++i) s += slabs[(size_t)i * SL_N + e];
  if (e < SL_W2) {
    const int o = e >> 6, k = e & 63;
    if (k < ncls) g.dw[0][o * ncls + k] = s;
  } else if (e < SL_W3) {
    g.dw[1][e - SL_W2] = s;
  } else if (e < SL_W4) {
    g.dw[2][e - SL_W3] = s;
  } else if (e < SL_B1) {
    g.dw[3][e - SL_W4] = s;
  } else if (e < SL_B2) {
    g.db[0][e - SL_B1] = s;
  } else if (e < SL_B3) {
    g.db[1][e - SL_B2] = s;
  } else if (e < SL_B4) {
    g.db[2][e - SL_B3] = s;
  } else {
    g.db[3][e - SL_B4] = s;
  }
}

// ---------------------------------------------------------------------------
// StackDiscNet (models/discriminator.py:139-175): the same four layers with
// LeakyReLU(0.2), then per point S[s] = w5[s] m + b5[s], out = logsumexp_s S,
// d_out = out / (out + 1), and run_training_seg_stack's BCE and shape terms
// (utils/trainer.py:1097-1150).  Everything after m is a function of that one
// scalar, so the backward is k_pwd_bwd<ACT_LRELU> on dm_d / dm_adv.
// ---------------------------------------------------------------------------
constexpr int SK_MAXS = 32;            // shape classes (the reference: 16)
constexpr int SK_NTERM = 8;            // adv, D's GT part, its no-GT part, CE, bad rows
constexpr int SK_NP = SK_NTERM + 2 * SK_MAXS;  // one workgroup's partial sums
// per-row columns of the tile's scratch (the free x buffer): dL/dS, m, the terms
constexpr int SK_CM = SK_MAXS, SK_CT = SK_MAXS + 1;

struct StkFwdOut {
  const float* w5;
  const float* b5;
  int S;
  const int32_t* shape_label;
  int ppc;
  float lambda_shape;
  float* m;
  int32_t* argc;
  float* d_out;
  float* shape_logits;  // optional [M][S]
  float* losses;        // [5] or NULL: no loss terms
  const float* soft0;
  const float* soft1;
  float* soft_out;
  uint64_t seed;
  const int32_t* step;
  float* dm_d;
  float* dm_adv;
  float* dw5;
  float* db5;
  int32_t* bad_rows;
  unsigned* ticket;
  float* partial;  // [SK_NP][gridDim.x]
};

// torch's binary_cross_entropy: the logs clamped at -100, the derivative's
// denominator at 1e-12.  x outside [0, 1] (a log of a negative number) gives a
// clamped NaN, never a fault; the row is counted in bad_rows.
__device__ __forceinline__ float stk_bce(float lx, float l1x, float y) {
  return -(y * lx + (1.f - y) * l1x);
}

// The semi-supervised term's scan (run_training_seg_stack_semi, utils/trainer.py:
// 1516-1530) in the forward's row lanes: a no-GT row is kept iff !(d_out <=
// th), its loss is log1p(es) (pwd_load_x0_t).  Per workgroup the kept count and
// the loss sum (f64) run in tile order into term rows 5..7 of the partials (the
// count's bits, the sum as an f32 pair hi + lo), and the last workgroup sums
// them in workgroup order with the other terms: K is on the device before the
// backward runs, so the gradient needs one launch (pcadv_row_semi_apply).
struct StkSemi {
  float th;
  float* loss;
  int32_t* kept;
};
constexpr int SK_TK = 5, SK_THI = 6, SK_TLO = 7;  // the scan's term rows

// SEMI = false is the plain forward (sm is not read).
template <bool SEMI>
__global__ void __launch_bounds__(PD_T, 2) k_stk_fwd(PwdNet p, StkFwdOut o, int ntiles, StkSemi sm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PwdFwdLds& L = *reinterpret_cast<PwdFwdLds*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long M = (long long)p.n0 + p.n1;
  const int S = o.S;
  double ssum = 0.0;  // SEMI, wave 0: the kept rows' loss sum and count over the tiles
  int skept = 0;
  uint32_t stepv = 0;
  if (o.losses && o.step) stepv = (uint32_t)*o.step;
  // wave 0's sums over this workgroup's tiles, in tile order: lane c < 32 holds
  // db5[c], lane 32 + c dw5[c]; every lane the five terms
  float gsum = 0.f, tsum[4] = {0.f, 0.f, 0.f, 0.f};
  int nbad = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = tile * PD_ROWS;
    float es = 0.f;
    pwd_load_x0_t<SEMI>(p, r0, tid, L.xa, es);
    __syncthreads();
    pwd_chain3<ACT_LRELU>(p, L.xa, L.xb, L.xa, L.xb, wave, lane);  // xa is free from here
    {
      const int row = tid >> 2, q = tid & 3;
      float best;
      int bi;
      pwd_conv4_max<ACT_LRELU>(p, L.xb, L.y4, tid, best, bi);
      const long long g = (long long)r0 + row;
      const bool in = g < M;
      // conv5 and the logsumexp less the row maximum: lane q holds s = q + 4 j
      float sv[SK_MAXS / 4], wv[SK_MAXS / 4], e[SK_MAXS / 4];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < SK_MAXS / 4; ++j) {
        const int s = q + 4 * j;
        const bool ok = s < S;
        wv[j] = ok ? o.w5[s] : 0.f;
        sv[j] = ok ? wv[j] * best + o.b5[s] : -INFINITY;
        mx = fmaxf(mx, sv[j]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 1));
      mx = fmaxf(mx, __shfl_xor(mx, 2));
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < SK_MAXS / 4; ++j) {
        e[j] = q + 4 * j < S ? expf(sv[j] - mx) : 0.f;
        sum += e[j];
      }
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      const float out = mx + logf(sum);
      const float x = out / (out + 1.f);
      if (in) {
        if (q == 0) {
          o.m[g] = best;
          o.argc[g] = bi;
          o.d_out[g] = x;
        }
        if (o.shape_logits) {
#pragma unroll
          for (int j = 0; j < SK_MAXS / 4; ++j)
            if (q + 4 * j < S) o.shape_logits[(size_t)g * S + q + 4 * j] = sv[j];
        }
      }
      if (o.losses) {  // uniform over the grid
        float t_adv = 0.f, t_gt = 0.f, t_ng = 0.f, t_ce = 0.f, t_bad = 0.f;
        float ds[SK_MAXS / 4];
#pragma unroll
        for (int j = 0; j < SK_MAXS / 4; ++j) ds[j] = 0.f;
        if (in) {
          const float inv = 1.f / sum;
          const float lx = fmaxf(logf(x), -100.f), l1x = fmaxf(log1pf(-x), -100.f);
          const float den = fmaxf(x * (1.f - x), 1e-12f);
          const float dxdo = 1.f / ((out + 1.f) * (out + 1.f));
          t_bad = (x >= 0.f && x <= 1.f) ? 0.f : 1.f;
          float gd, lam = 0.f;
          int lab = -1;
          if (g < p.n0) {
            // make_D_label(random=True), one label per point (utils/utils.py:22-31)
            const float y0 = o.soft0 ? o.soft0[g]
                                     : 0.7f + 0.35f * rng_uniform(o.seed, stepv, RNG_LABEL_GT,
                                                                  (uint32_t)g);
            t_gt = stk_bce(lx, l1x, y0);
            gd = 0.5f * ((x - y0) / den) * dxdo / (float)p.n0;
            lab = o.shape_label[g / o.ppc];
            lam = o.lambda_shape / (float)p.n0;
            if (o.soft_out && q == 0) o.soft_out[g] = y0;
          } else {
            const long long jr = g - p.n0;
            const float y1 = o.soft1 ? o.soft1[jr]
                                     : 0.305f * rng_uniform(o.seed, stepv, RNG_LABEL_NOGT,
                                                            (uint32_t)jr);
            t_ng = stk_bce(lx, l1x, y1);
            t_adv = stk_bce(lx, l1x, 1.f);  // against label 1 (the generator's term)
            gd = 0.5f * ((x - y1) / den) * dxdo / (float)p.n1;
            if (o.soft_out && q == 0) o.soft_out[g] = y1;
          }
          float pw = 0.f, dmd = 0.f, slab = 0.f;
#pragma unroll
          for (int j = 0; j < SK_MAXS / 4; ++j) {
            const int s = q + 4 * j;
            const float pj = e[j] * inv;
            const bool hit = s == lab;
            if (s < S) ds[j] = gd * pj + lam * (pj - (hit ? 1.f : 0.f));
            if (hit && s < S) slab = sv[j];
            pw += pj * wv[j];
            dmd += ds[j] * wv[j];
          }
          pw += __shfl_xor(pw, 1);
          pw += __shfl_xor(pw, 2);
          dmd += __shfl_xor(dmd, 1);
          dmd += __shfl_xor(dmd, 2);
          slab += __shfl_xor(slab, 1);
          slab += __shfl_xor(slab, 2);
          if (g < p.n0) t_ce = out - slab;  // CrossEntropyLoss(S, shape label) of the row
          if (q == 0) {
            o.dm_d[g] = dmd;
            if (g >= p.n0 && o.dm_adv)
              o.dm_adv[g - p.n0] = ((x - 1.f) / den) * dxdo * pw / (float)p.n1;
          }
        }
        float* sc = L.xa + row * PD_S;
#pragma unroll
        for (int j = 0; j < SK_MAXS / 4; ++j) sc[q + 4 * j] = ds[j];
        if (q == 0) {
          sc[SK_CM] = in ? best : 0.f;
          sc[SK_CT + 0] = t_adv;
          sc[SK_CT + 1] = t_gt;
          sc[SK_CT + 2] = t_ng;
          sc[SK_CT + 3] = t_ce;
          sc[SK_CT + 4] = t_bad;
          if constexpr (SEMI) {
            const bool keep = in && g >= p.n0 && !(x <= sm.th);  // the x stored as d_out[g]
            sc[SK_CT + 5] = keep ? log1pf(es) : 0.f;
            sc[SK_CT + 6] = keep ? 1.f : 0.f;
          }
        }
      }
    }
    if (o.losses) {
      __syncthreads();  // the scratch rows are written, y4 is read for the last time
      {  // each wave sums a quarter of the rows in row order, wave 0 the quarters
        const int c = lane & (SK_MAXS - 1);
        const bool wgt = lane >= SK_MAXS;
        float a = 0.f;
#pragma unroll 4
        for (int row = 16 * wave; row < 16 * wave + 16; ++row) {
          const float v = L.xa[row * PD_S + c];
          a += wgt ? v * L.xa[row * PD_S + SK_CM] : v;
        }
        L.y4[tid] = a;
      }
      float t5[5];
      if (wave == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) t5[k] = wave_sum(L.xa[lane * PD_S + SK_CT + k]);
        if constexpr (SEMI) {
          ssum += (double)wave_sum(L.xa[lane * PD_S + SK_CT + 5]);
          skept += (int)wave_sum(L.xa[lane * PD_S + SK_CT + 6]);
        }
      }
      __syncthreads();  // the next tile's x0 goes to xa
      if (wave == 0) {
        gsum += ((L.y4[lane] + L.y4[64 + lane]) + L.y4[128 + lane]) + L.y4[192 + lane];
#pragma unroll
        for (int k = 0; k < 4; ++k) tsum[k] += t5[k];
        nbad += (int)t5[4];
      }
      // y4 is written again after three more barriers
    }
  }
  if (!o.losses) return;
  const int G = gridDim.x;
  if (wave == 0) {
    o.partial[(size_t)(SK_NTERM + lane) * G + blockIdx.x] = gsum;
    if (lane < 4) o.partial[(size_t)lane * G + blockIdx.x] = tsum[lane];
    if (lane == 4) o.partial[(size_t)4 * G + blockIdx.x] = __int_as_float(nbad);
    if constexpr (SEMI) {
      const float hi = (float)ssum;
      if (lane == SK_TK) o.partial[(size_t)SK_TK * G + blockIdx.x] = __int_as_float(skept);
      if (lane == SK_THI) o.partial[(size_t)SK_THI * G + blockIdx.x] = hi;
      if (lane == SK_TLO) o.partial[(size_t)SK_TLO * G + blockIdx.x] = (float)(ssum - (double)hi);
    }
  }
  // the last workgroup to arrive sums the workgroups' terms in workgroup order
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const unsigned t = atomicAdd(o.ticket, 1u);
    L.last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!L.last) return;  // uniform over the workgroup
  __threadfence();
  // Sum k of the 4 + 2 S (the four terms, db5, dw5) belongs to wave k & 3: each
  // lane adds every 64th workgroup's value, all of a wave's sums in one pass so
  // that their loads are in flight together, then a butterfly.
  const unsigned* part = reinterpret_cast<const unsigned*>(o.partial);
  constexpr int KU = (4 + 2 * SK_MAXS) / 4;
  const int nsum = 4 + 2 * S;
  float acc[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) acc[u] = 0.f;
  for (int t = lane; t < G; t += 64) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = wave + 4 * u;
      // partial's row: terms 0..3, db5[j] at SK_NTERM + j, dw5[j] at SK_NTERM + 32 + j
      const int row = k < 4 ? k : k - 4 < S ? SK_NTERM + k - 4 : SK_NTERM + SK_MAXS + (k - 4 - S);
      if (k < nsum)
        acc[u] += __uint_as_float(__hip_atomic_load(part + (size_t)row * G + t, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT));
    }
  }
  float* fin = &L.lt[0][0];  // 4 + 2 S <= 68 sums
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int k = wave + 4 * u;
    const float v = wave_sum(acc[u]);
    if (k < nsum && lane == 0) fin[k] = v;
  }
  int bad = 0;
  if (wave == 0) {
    for (int t = lane; t < G; t += 64)
      bad += (int)__hip_atomic_load(part + (size_t)4 * G + t, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
    bad = wave_sum(bad);
  }
  if constexpr (SEMI) {
    if (wave == 1) {  // the workgroups' counts and loss sums, lane-strided then a butterfly
      int K = 0;
      double tot = 0.0;
      for (int t = lane; t < G; t += 64) {
        K += (int)__hip_atomic_load(part + (size_t)SK_TK * G + t, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
        const float hi = __uint_as_float(__hip_atomic_load(
            part + (size_t)SK_THI * G + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const float lo = __uint_as_float(__hip_atomic_load(
            part + (size_t)SK_TLO * G + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        tot += (double)hi + (double)lo;
      }
      K = wave_sum(K);
      tot = wave_sum(tot);
      if (lane == 0) {
        *sm.loss = K > 0 ? (float)(tot / (double)K) : 0.f;
        *sm.kept = K;
      }
    }
  }
  __syncthreads();
  if (tid < 2 * S) (tid < S ? o.db5 : o.dw5)[tid < S ? tid : tid - S] = fin[4 + tid];
  if (tid == 0) {
    const float* term = fin;
    const float adv = p.n1 ? term[0] / (float)p.n1 : 0.f;
    const float dgt = p.n0 ? 0.5f * (term[1] / (float)p.n0) : 0.f;
    const float dng = p.n1 ? 0.5f * (term[2] / (float)p.n1) : 0.f;
    o.losses[0] = adv;        // loss_adv
    o.losses[1] = dgt + dng;  // loss_D
    o.losses[2] = dgt;
    o.losses[3] = dng;
    o.losses[4] = p.n0 ? term[3] / (float)p.n0 : 0.f;  // loss_D_shape, unscaled
    *o.bad_rows = bad;
    *o.ticket = 0u;  // ready for the next launch
  }
}

int pwd_tiles(long long rows) { return (int)((rows + PD_ROWS - 1) / PD_ROWS); }
int pwd_grid(int ntiles, int max_wg, int dflt) {
  const int cap = max_wg > 0 ? max_wg : dflt;
  return ntiles < cap ? ntiles : cap;
}

// The workspace of either discriminator: the ticket alone on its line, the
// forward's partial sums (pwdisc: three per tile; stackdisc: SK_NP per forward
// workgroup), then one weight-gradient slab per backward workgroup.
struct PwdWs {
  size_t partial_bytes, bytes;
  unsigned* ticket(void* ws) const { return reinterpret_cast<unsigned*>(ws); }
  float* partial(void* ws) const {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + WS_HEAD);
  }
  float* slabs(void* ws) const {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + WS_HEAD + partial_bytes);
  }
};
PwdWs pwd_ws(long long rows, int max_wg, bool stack) {
  if (rows < 1) return {0, 0};
  const int nt = pwd_tiles(rows);
  const size_t np = stack ? (size_t)pwd_grid(nt, max_wg, PD_FWD_WG) * SK_NP : (size_t)nt * 3;
  const size_t pb = (np * 4 + 255) / 256 * 256;
  return {pb, WS_HEAD + pb + (size_t)pwd_grid(nt, max_wg, PD_BWD_WG) * SL_N * 4};
}

float* pwd_row_out(const pcadv_pwdisc_args* a) { return a->out; }
float* pwd_row_out(const pcadv_stackdisc_args* a) { return a->m; }

// The fields the two args structs share.  pcadv_stackdisc_args adds num_shapes
// and conv5, whose [S][1] weight is read by scalars (no alignment asked).
template <typename A>
int pwd_check(const A* a, const char* what, PwdNet& p) {
  constexpr bool STACK = std::is_same_v<A, pcadv_stackdisc_args>;
  constexpr int NL = STACK ? 5 : 4;
  PC_REQUIRE(a, "%s: args is NULL", what);
  PC_REQUIRE(a->ncls >= 2 && a->ncls <= 64, "%s: ncls = %d, expected 2..64", what, a->ncls);
  if constexpr (STACK)
    PC_REQUIRE(a->num_shapes >= 2 && a->num_shapes <= SK_MAXS,
               "%s: num_shapes = %d, expected 2..%d", what, a->num_shapes, SK_MAXS);
  PC_REQUIRE(a->n0 >= 0 && a->n1 >= 0 && (long long)a->n0 + a->n1 >= 1 &&
                 (long long)a->n0 + a->n1 <= 0x7fffffffLL - PD_ROWS,
             "%s: row counts n0 = %d, n1 = %d", what, a->n0, a->n1);
  PC_REQUIRE(a->ld >= a->ncls, "%s: row stride ld = %lld < ncls = %d", what, (long long)a->ld,
             a->ncls);
  PC_REQUIRE(a->t0 >= 0 && a->t0 <= 2 && a->t1 >= 0 && a->t1 <= 2,
             "%s: transforms (%d, %d): PCADV_PWD_NONE / _SOFTMAX / _LOG_SOFTMAX", what, a->t0,
             a->t1);
  PC_REQUIRE(a->max_workgroups >= 0, "%s: max_workgroups = %d", what, a->max_workgroups);
  PC_REQUIRE(a->logits && pwd_row_out(a) && a->argc, "%s: logits, %s and argc are required", what,
             STACK ? "m" : "out");
  for (int i = 0; i < NL; ++i) {
    PC_REQUIRE(a->w[i] && a->b[i], "%s: conv%d's weight and bias are required", what, i + 1);
    PC_REQUIRE(i == 0 || i == 4 || ((uintptr_t)a->w[i] & 15) == 0,
               "%s: conv%d's weight is not 16-B aligned", what, i + 1);
    if (i < 4) {
      p.w[i] = a->w[i];
      p.b[i] = a->b[i];
    }
  }
  p.logits = a->logits;
  p.ld = a->ld;
  p.ncls = a->ncls;
  p.n0 = a->n0;
  p.n1 = a->n1;
  p.t0 = a->t0;
  p.t1 = a->t1;
  return PCADV_OK;
}

template <typename K>
int pwd_lds(K kernel, size_t bytes, const char* what) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: %zu bytes of LDS refused", what, bytes);
    return PCADV_EHIP;
  }
  return PCADV_OK;
}

// What a forward with losses asks of either struct beyond its own outputs:
// a step counter for drawn labels and the workspace.
template <typename A>
int pwd_check_losses(const A* a, const char* what, const PwdWs& ws) {
  const bool drawn = (a->n0 > 0 && !a->soft0) || (a->n1 > 0 && !a->soft1);
  PC_REQUIRE(!drawn || a->step_count, "%s: device-drawn labels need step_count", what);
  PC_REQUIRE(a->workspace && a->workspace_bytes >= ws.bytes, "%s: workspace of %zu bytes, need %zu",
             what, a->workspace_bytes, ws.bytes);
  return PCADV_OK;
}

// The backward of both: k_pwd_bwd<ACT> on b (its slabs set here) and the
// fixed-order finish into a's dw[0..3] / db[0..3].
template <int ACT, typename A>
int pwd_launch_bwd(const A* a, const char* what, const PwdNet& p, PwdBwdArgs b, const PwdWs& ws,
                   hipStream_t s) {
  constexpr const char* kname = ACT == ACT_RELU ? "k_pwd_bwd" : "k_pwd_bwd<lrelu>";
  PwdGrads g;
  for (int i = 0; i < 4; ++i) {
    PC_REQUIRE(a->dw[i] && a->db[i], "%s: conv%d's gradients are required", what, i + 1);
    g.dw[i] = a->dw[i];
    g.db[i] = a->db[i];
  }
  PC_REQUIRE(!a->dlogits || a->ldd >= a->ncls, "%s: dlogits stride %lld < ncls", what,
             (long long)a->ldd);
  PC_REQUIRE(a->workspace && a->workspace_bytes >= ws.bytes, "%s: workspace of %zu bytes, need %zu",
             what, a->workspace_bytes, ws.bytes);
  b.argc = a->argc;
  b.lambda_adv = a->lambda_adv;
  b.dlogits = a->dlogits;
  b.ldd = a->ldd;
  b.x_out = a->x_out;
  b.slabs = ws.slabs(a->workspace);
  // one guard per instantiation, i.e. per kernel; see launch_pwdisc_fwd
  static int once = pwd_lds(k_pwd_bwd<ACT>, sizeof(PwdBwdLds), kname);
  if (once) return once;
  const int nt = pwd_tiles((long long)p.n0 + p.n1);
  const int grid = pwd_grid(nt, a->max_workgroups, PD_BWD_WG);
  hipLaunchKernelGGL(k_pwd_bwd<ACT>, dim3(grid), dim3(PD_T), sizeof(PwdBwdLds), s, p, b, nt);
  PC_HIP_CHECK_LAUNCH(kname);
  hipLaunchKernelGGL(k_pwd_bwd_finish, dim3((SL_N + 255) / 256), dim3(256), 0, s, b.slabs, grid,
                     a->ncls, g);
  PC_HIP_CHECK_LAUNCH("k_pwd_bwd_finish");
  return PCADV_OK;
}

}  // namespace

size_t pwdisc_workspace_bytes(long long rows, int max_wg) {
  return pwd_ws(rows, max_wg, false).bytes;
}
size_t stackdisc_workspace_bytes(long long rows, int max_wg) {
  return pwd_ws(rows, max_wg, true).bytes;
}

int launch_pwdisc_fwd(const pcadv_pwdisc_args* a, hipStream_t s) {
  const char* what = "pcadv_pwdisc_forward";
  PwdNet p;
  if (int rc = pwd_check(a, what, p)) return rc;
  const int nt = pwd_tiles((long long)a->n0 + a->n1);
  PwdFwdOut o = {};
  o.out = a->out;
  o.argc = a->argc;
  if (a->losses) {
    const PwdWs ws = pwd_ws((long long)a->n0 + a->n1, a->max_workgroups, false);
    PC_REQUIRE(a->dout_d, "%s: losses need dout_d", what);
    if (int rc = pwd_check_losses(a, what, ws)) return rc;
    o.losses = a->losses;
    o.soft0 = a->soft0;
    o.soft1 = a->soft1;
    o.soft_out = a->soft_out;
    o.seed = a->rng_seed;
    o.step = a->step_count;
    o.dout_d = a->dout_d;
    o.dout_adv = a->dout_adv;
    o.ticket = ws.ticket(a->workspace);
    o.partial = ws.partial(a->workspace);
  }
  // Once per process, as every launcher of this library does (set outside any
  // stream capture by the first eager call).  The attribute belongs to the
  // current device's copy of the kernel: a process that drives a second device
  // would have to set it there too (data parallelism runs one process per GPU).
  static int once = pwd_lds(k_pwd_fwd, sizeof(PwdFwdLds), "k_pwd_fwd");
  if (once) return once;
  hipLaunchKernelGGL(k_pwd_fwd, dim3(pwd_grid(nt, a->max_workgroups, PD_FWD_WG)), dim3(PD_T),
                     sizeof(PwdFwdLds), s, p, o, nt);
  PC_HIP_CHECK_LAUNCH("k_pwd_fwd");
  return PCADV_OK;
}

int launch_pwdisc_bwd(const pcadv_pwdisc_args* a, hipStream_t s) {
  const char* what = "pcadv_pwdisc_backward";
  PwdNet p;
  if (int rc = pwd_check(a, what, p)) return rc;
  PC_REQUIRE(a->dout_d, "%s: dout_d is required", what);
  PwdBwdArgs b;
  b.out = a->out;
  b.dout_d = a->dout_d;
  b.dout_adv = a->dout_adv;
  return pwd_launch_bwd<ACT_RELU>(a, what, p, b,
                                  pwd_ws((long long)a->n0 + a->n1, a->max_workgroups, false), s);
}

// pcadv_stackdisc_forward (semi NULL) and pcadv_stackdisc_forward_semi
int launch_stackdisc_fwd(const pcadv_stackdisc_args* a, const pcadv_stackdisc_semi* semi,
                         hipStream_t s) {
  const char* what = semi ? "pcadv_stackdisc_forward_semi" : "pcadv_stackdisc_forward";
  PwdNet p;
  if (int rc = pwd_check(a, what, p)) return rc;
  const int nt = pwd_tiles((long long)a->n0 + a->n1);
  PC_REQUIRE(a->d_out, "%s: d_out is required", what);
  if (semi) {
    PC_REQUIRE(a->losses, "%s: the scan runs with the loss terms: losses is required", what);
    PC_REQUIRE(semi->loss_semi && semi->kept, "%s: loss_semi and kept are required", what);
    PC_REQUIRE(((uintptr_t)semi->loss_semi & 3) == 0 && ((uintptr_t)semi->kept & 3) == 0,
               "%s: loss_semi and kept are not 4-B aligned", what);
  }
  StkFwdOut o = {};
  o.w5 = a->w[4];
  o.b5 = a->b[4];
  o.S = a->num_shapes;
  o.m = a->m;
  o.argc = a->argc;
  o.d_out = a->d_out;
  o.shape_logits = a->shape_logits;
  o.ppc = 1;
  if (a->losses) {
    const PwdWs ws = pwd_ws((long long)a->n0 + a->n1, a->max_workgroups, true);
    PC_REQUIRE(a->dm_d && a->dw[4] && a->db[4] && a->bad_rows,
               "%s: losses need dm_d, conv5's dw / db and bad_rows", what);
    if (a->n0 > 0) {
      PC_REQUIRE(a->shape_label && a->pts_per_cloud >= 1 && a->n0 % a->pts_per_cloud == 0,
                 "%s: the GT rows need shape_label and a pts_per_cloud (%d) that divides n0 = %d",
                 what, a->pts_per_cloud, a->n0);
      o.ppc = a->pts_per_cloud;
    }
    if (int rc = pwd_check_losses(a, what, ws)) return rc;
    o.shape_label = a->shape_label;
    o.lambda_shape = a->lambda_disc_shape;
    o.losses = a->losses;
    o.soft0 = a->soft0;
    o.soft1 = a->soft1;
    o.soft_out = a->soft_out;
    o.seed = a->rng_seed;
    o.step = a->step_count;
    o.dm_d = a->dm_d;
    o.dm_adv = a->dm_adv;
    o.dw5 = a->dw[4];
    o.db5 = a->db[4];
    o.bad_rows = a->bad_rows;
    o.ticket = ws.ticket(a->workspace);
    o.partial = ws.partial(a->workspace);
  }
  const dim3 grid(pwd_grid(nt, a->max_workgroups, PD_FWD_WG));
  if (semi) {
    const StkSemi sm = {semi->semi_th, semi->loss_semi, semi->kept};
    static int once_semi = pwd_lds(k_stk_fwd<true>, sizeof(PwdFwdLds), "k_stk_fwd<semi>");
    if (once_semi) return once_semi;
    hipLaunchKernelGGL(k_stk_fwd<true>, grid, dim3(PD_T), sizeof(PwdFwdLds), s, p, o, nt, sm);
    PC_HIP_CHECK_LAUNCH("k_stk_fwd<semi>");
    return PCADV_OK;
  }
  static int once = pwd_lds(k_stk_fwd<false>, sizeof(PwdFwdLds), "k_stk_fwd");  // see launch_pwdisc_fwd
  if (once) return once;
  hipLaunchKernelGGL(k_stk_fwd<false>, grid, dim3(PD_T), sizeof(PwdFwdLds), s, p, o, nt, StkSemi{});
  PC_HIP_CHECK_LAUNCH("k_stk_fwd");
  return PCADV_OK;
}

int launch_stackdisc_bwd(const pcadv_stackdisc_args* a, hipStream_t s) {
  const char* what = "pcadv_stackdisc_backward";
  PwdNet p;
  if (int rc = pwd_check(a, what, p)) return rc;
  PC_REQUIRE(a->dm_d, "%s: dm_d is required", what);
  PwdBwdArgs b;
  b.out = a->m;
  b.dout_d = a->dm_d;
  b.dout_adv = a->dm_adv;
  return pwd_launch_bwd<ACT_LRELU>(a, what, p, b,
                                   pwd_ws((long long)a->n0 + a->n1, a->max_workgroups, true), s);
}

}  // namespace pcadv
