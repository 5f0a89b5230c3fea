// The dual discriminator of run_training_seg_dual (models/discriminator.py:
// 82-137, utils/trainer.py:2123-2382): the kernels around the dense GEMM engine
// that BaseDiscNet / PointDiscNet / ShapeDiscNet need and the engine lacks.
//
//   pcadv_dual_input        softmax / log_softmax of the generator's rows (D's input)
//   pcadv_lrelu_fwd / _bwd  LeakyReLU(0.2) in place on a GEMM's output, and its
//                           derivative (from the activation OUTPUT: slope 0.2 at
//                           y <= 0, as torch's in-place LeakyReLU) on a data gradient
//   pcadv_dual_point_tail   per point the max / arg-max over PointDiscNet's
//                           channels, the three BCE-with-logits terms, their
//                           derivatives and the one-hot top gradients
//   pcadv_dual_input_bwd    the no-GT rows' dlogits through the input transform
//   pcadv_sgd               plain SGD on a flat range, optionally through a
//                           running gradient sum (PointDiscNet's never-cleared .grad)
//
// The wide layers themselves run on pcadv_gemm (precise = 1, no activation) and
// pcadv_gemm_wgrad, the shape head on pcadv_conv_max_x3 / pcadv_linear_*.
// Every sum here runs in a fixed order: no floating-point atomics, bitwise
// reproducible.  Max winners are taken on f32 values, the first index on ties.
#include <cmath>

#include "common.h"

namespace pcadv {

namespace {

constexpr int DD_T = 256;       // threads per workgroup
constexpr int DD_ROWS = 64;     // rows per tile of the tail
constexpr int DD_MAXC = 64;     // classes the input transform takes

// one thread per row: the row lives in registers-by-loop (ncls <= 64 reads, twice)
__global__ void __launch_bounds__(DD_T)
k_dd_input(const float* __restrict__ logits, long long ld, int ncls, long long n0, long long n1,
           int t0, int t1, float* __restrict__ x0) {
  const long long M = n0 + n1;
  for (long long g = (long long)blockIdx.x * DD_T + threadIdx.x; g < M;
       g += (long long)gridDim.x * DD_T) {
    const float* src = logits + g * ld;
    float* dst = x0 + g * ncls;
    const int tr = g < n0 ? t0 : t1;
    float mx = -INFINITY;
    for (int c = 0; c < ncls; ++c) mx = fmaxf(mx, src[c]);
    float s = 0.f;
    for (int c = 0; c < ncls; ++c) s += expf(src[c] - mx);
    const float lg = logf(s);
    for (int c = 0; c < ncls; ++c) {
      const float v = src[c];
      float y = v;
      if (tr == PCADV_PWD_SOFTMAX) y = expf(v - mx) / s;
      if (tr == PCADV_PWD_LOG_SOFTMAX) y = (v - mx) - lg;
      dst[c] = y;
    }
  }
}

// rows [0, n) of x0 (the transformed no-GT rows, dense [n][ncls]) and of dx0:
// the transform's backward into dlogits (row stride ldd, ncls columns written)
__global__ void __launch_bounds__(DD_T)
k_dd_input_bwd(const float* __restrict__ x0, const float* __restrict__ dx0, int ncls, long long n,
               int tr, float* __restrict__ dlogits, long long ldd) {
  for (long long g = (long long)blockIdx.x * DD_T + threadIdx.x; g < n;
       g += (long long)gridDim.x * DD_T) {
    const float* y = x0 + g * ncls;
    const float* dy = dx0 + g * ncls;
    float* d = dlogits + g * ldd;
    float sum = 0.f, dot = 0.f;
    for (int c = 0; c < ncls; ++c) {
      sum += dy[c];
      dot += dy[c] * y[c];
    }
    for (int c = 0; c < ncls; ++c) {
      float v = dy[c];
      if (tr == PCADV_PWD_LOG_SOFTMAX) v = dy[c] - expf(y[c]) * sum;
      if (tr == PCADV_PWD_SOFTMAX) v = y[c] * (dy[c] - dot);
      d[c] = v;
    }
  }
}

__global__ void __launch_bounds__(DD_T) k_dd_lrelu_fwd(float* __restrict__ y, long long n, int vec) {
  const long long i0 = (long long)blockIdx.x * DD_T + threadIdx.x;
  const long long stride = (long long)gridDim.x * DD_T;
  if (vec) {
    f32x4* y4 = reinterpret_cast<f32x4*>(y);
    const long long n4 = n >> 2;
    for (long long i = i0; i < n4; i += stride) {
      f32x4 v = y4[i];
      v.x = act_fwd(v.x, ACT_LRELU);
      v.y = act_fwd(v.y, ACT_LRELU);
      v.z = act_fwd(v.z, ACT_LRELU);
      v.w = act_fwd(v.w, ACT_LRELU);
      y4[i] = v;
    }
    for (long long i = (n4 << 2) + i0; i < n; i += stride) y[i] = act_fwd(y[i], ACT_LRELU);
  } else {
    for (long long i = i0; i < n; i += stride) y[i] = act_fwd(y[i], ACT_LRELU);
  }
}

__global__ void __launch_bounds__(DD_T)
k_dd_lrelu_bwd(float* __restrict__ d, const float* __restrict__ y, long long n, int vec) {
  const long long i0 = (long long)blockIdx.x * DD_T + threadIdx.x;
  const long long stride = (long long)gridDim.x * DD_T;
  if (vec) {
    f32x4* d4 = reinterpret_cast<f32x4*>(d);
    const f32x4* y4 = reinterpret_cast<const f32x4*>(y);
    const long long n4 = n >> 2;
    for (long long i = i0; i < n4; i += stride) {
      f32x4 v = d4[i];
      const f32x4 a = y4[i];
      v.x *= act_bwd(a.x, ACT_LRELU);
      v.y *= act_bwd(a.y, ACT_LRELU);
      v.z *= act_bwd(a.z, ACT_LRELU);
      v.w *= act_bwd(a.w, ACT_LRELU);
      d4[i] = v;
    }
    for (long long i = (n4 << 2) + i0; i < n; i += stride) d[i] *= act_bwd(y[i], ACT_LRELU);
  } else {
    for (long long i = i0; i < n; i += stride) d[i] *= act_bwd(y[i], ACT_LRELU);
  }
}

struct DdTail {
  const float* y;  // [n0 + n1][C], after LeakyReLU
  int C;
  long long n0, n1;
  float* out;
  int32_t* argc;
  int want_loss;
  const float* soft0;
  const float* soft1;
  float* soft_out;
  uint64_t seed;
  const int32_t* step;
  float* dout_d;
  float* dout_adv;
  float lambda_adv;
  float* dz_d;    // [n0 + n1][C] or NULL
  float* dz_adv;  // [n1][C] or NULL
  float* partial; // [ntiles][3]
};

// 16 lanes per row (four rows per wave); lane l holds channels 4 (l + 16 i) + j.
// The lanes' bests combine by xor shuffles under (greater value, then smaller
// index), a total order: every lane ends with the same winner.
__global__ void __launch_bounds__(DD_T) k_dd_tail(DdTail a, int ntiles) {
  __shared__ float lt[3][DD_ROWS];
  const int tid = threadIdx.x, l = tid & 15, rr = tid >> 4;  // rr: row within a 16-row pass
  const long long M = a.n0 + a.n1;
  uint32_t stepv = 0;
  if (a.want_loss && a.step) stepv = (uint32_t)*a.step;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    for (int pass = 0; pass < DD_ROWS / 16; ++pass) {
      const int row = pass * 16 + rr;
      const long long g = (long long)tile * DD_ROWS + row;
      const bool in = g < M;
      const float* src = a.y + (in ? g : 0) * a.C;
      float best = -INFINITY;
      int bi = 0x7fffffff;
      for (int c0 = 4 * l; c0 < a.C; c0 += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + c0);
        if (v.x > best) { best = v.x; bi = c0; }
        if (v.y > best) { best = v.y; bi = c0 + 1; }
        if (v.z > best) { best = v.z; bi = c0 + 2; }
        if (v.w > best) { best = v.w; bi = c0 + 3; }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      float l0 = 0.f, l1 = 0.f, l2 = 0.f, sd = 0.f, sa = 0.f;
      if (in && a.want_loss) {
        // make_D_label(random=True), one label per point (utils/utils.py:22-31)
        const float z = best;
        const float sg = 1.f / (1.f + expf(-z));
        const float sp = log1pf(expf(-fabsf(z)));
        const float slope = act_bwd(best, ACT_LRELU);
        if (g < a.n0) {
          const float y0 = a.soft0 ? a.soft0[g]
                                   : 0.7f + 0.35f * rng_uniform(a.seed, stepv, RNG_LABEL_GT,
                                                                (uint32_t)g);
          l1 = fmaxf(z, 0.f) - z * y0 + sp;
          const float dd = 0.5f * (sg - y0) / (float)a.n0;
          sd = dd * slope;
          if (l == 0) {
            a.dout_d[g] = dd;
            if (a.soft_out) a.soft_out[g] = y0;
          }
        } else {
          const long long j = g - a.n0;
          const float y1 = a.soft1 ? a.soft1[j]
                                   : 0.305f * rng_uniform(a.seed, stepv, RNG_LABEL_NOGT,
                                                          (uint32_t)j);
          l2 = fmaxf(z, 0.f) - z * y1 + sp;
          l0 = fmaxf(z, 0.f) - z + sp;  // against label 1 (the generator's term)
          const float dd = 0.5f * (sg - y1) / (float)a.n1;
          const float da = (sg - 1.f) / (float)a.n1;
          sd = dd * slope;
          sa = a.lambda_adv * da * slope;
          if (l == 0) {
            a.dout_d[g] = dd;
            if (a.dout_adv) a.dout_adv[j] = da;
            if (a.soft_out) a.soft_out[g] = y1;
          }
        }
      }
      if (in) {
        if (l == 0) {
          a.out[g] = best;
          a.argc[g] = bi;
        }
        if (a.want_loss) {
          for (int c0 = 4 * l; c0 < a.C; c0 += 64) {
            f32x4 d = {0.f, 0.f, 0.f, 0.f}, e = {0.f, 0.f, 0.f, 0.f};
            const int k = bi - c0;
            if (k == 0) { d.x = sd; e.x = sa; }
            if (k == 1) { d.y = sd; e.y = sa; }
            if (k == 2) { d.z = sd; e.z = sa; }
            if (k == 3) { d.w = sd; e.w = sa; }
            if (a.dz_d) *reinterpret_cast<f32x4*>(a.dz_d + g * a.C + c0) = d;
            if (a.dz_adv && g >= a.n0)
              *reinterpret_cast<f32x4*>(a.dz_adv + (g - a.n0) * a.C + c0) = e;
          }
        }
      }
      if (l == 0) {
        lt[0][row] = l0;
        lt[1][row] = l1;
        lt[2][row] = l2;
      }
    }
    __syncthreads();
    if (a.want_loss && tid < 64) {
      const float s0 = wave_sum(lt[0][tid]), s1 = wave_sum(lt[1][tid]), s2 = wave_sum(lt[2][tid]);
      if (tid == 0) {
        a.partial[3 * (size_t)tile + 0] = s0;
        a.partial[3 * (size_t)tile + 1] = s1;
        a.partial[3 * (size_t)tile + 2] = s2;
      }
    }
    __syncthreads();
  }
}

// the tiles' terms in tile order: one wave, lane t takes tiles t, t + 64, ...
__global__ void __launch_bounds__(64)
k_dd_tail_fin(const float* __restrict__ partial, int ntiles, long long n0, long long n1,
              float* __restrict__ losses) {
  const int lane = threadIdx.x;
  float a[3] = {0.f, 0.f, 0.f};
  for (int t = lane; t < ntiles; t += 64)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] += partial[3 * (size_t)t + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = wave_sum(a[k]);
  if (lane == 0) {
    const float adv = n1 ? a[0] / (float)n1 : 0.f;
    const float dgt = n0 ? 0.5f * (a[1] / (float)n0) : 0.f;
    const float dng = n1 ? 0.5f * (a[2] / (float)n1) : 0.f;
    losses[0] = adv;        // loss_adv
    losses[1] = dgt + dng;  // loss_D_point
    losses[2] = dgt;
    losses[3] = dng;
  }
}

// p -= lr g, or with acc: acc += g; p -= lr acc.  The product and the
// difference are rounded separately (contraction off: no fma), so the vector
// and the scalar form leave the same bits, those of float32 numpy.
__device__ __forceinline__ float sgd_elem(float p, float g, float lr) {
#pragma clang fp contract(off)
  const float s = lr * g;
  return p - s;
}
__device__ __forceinline__ float sgd_acc(float a, float g) {
#pragma clang fp contract(off)
  return a + g;
}

__global__ void __launch_bounds__(DD_T)
k_dd_sgd(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ acc, long long n,
         float lr, int vec) {
  const long long i0 = (long long)blockIdx.x * DD_T + threadIdx.x;
  const long long stride = (long long)gridDim.x * DD_T;
  long long done = 0;
  if (vec) {
    const long long n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* a4 = reinterpret_cast<f32x4*>(acc);
    for (long long i = i0; i < n4; i += stride) {
      f32x4 pv = p4[i];
      f32x4 gv = g4[i];
      if (acc) {
        const f32x4 av = a4[i];
        gv.x = sgd_acc(av.x, gv.x);
        gv.y = sgd_acc(av.y, gv.y);
        gv.z = sgd_acc(av.z, gv.z);
        gv.w = sgd_acc(av.w, gv.w);
        a4[i] = gv;
      }
      pv.x = sgd_elem(pv.x, gv.x, lr);
      pv.y = sgd_elem(pv.y, gv.y, lr);
      pv.z = sgd_elem(pv.z, gv.z, lr);
      pv.w = sgd_elem(pv.w, gv.w, lr);
      p4[i] = pv;
    }
    done = n4 << 2;
  }
  for (long long i = done + i0; i < n; i += stride) {
    float gv = g[i];
    if (acc) {
      gv = sgd_acc(acc[i], gv);
      acc[i] = gv;
    }
    p[i] = sgd_elem(p[i], gv, lr);
  }
}

inline int grid_for(long long work_items, int cap = 2048) {
  long long b = (work_items + DD_T - 1) / DD_T;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

}  // namespace pcadv

using namespace pcadv;

extern "C" {

int pcadv_dual_input(const float* logits, int64_t ld, int ncls, int64_t n0, int64_t n1, int t0,
                     int t1, float* x0, hipStream_t stream) {
  PC_REQUIRE(logits && x0 && n0 >= 0 && n1 >= 0 && ncls >= 2 && ncls <= DD_MAXC && ld >= ncls,
             "dual_input: bad shape (ncls = %d, ld = %lld)", ncls, (long long)ld);
  PC_REQUIRE(t0 >= PCADV_PWD_NONE && t0 <= PCADV_PWD_LOG_SOFTMAX && t1 >= PCADV_PWD_NONE &&
                 t1 <= PCADV_PWD_LOG_SOFTMAX,
             "dual_input: transforms (%d, %d)", t0, t1);
  if (n0 + n1 == 0) return PCADV_OK;
  hipLaunchKernelGGL(k_dd_input, dim3(grid_for(n0 + n1)), dim3(DD_T), 0, stream, logits,
                     (long long)ld, ncls, (long long)n0, (long long)n1, t0, t1, x0);
  PC_HIP_CHECK_LAUNCH("k_dd_input");
  return PCADV_OK;
}

int pcadv_dual_input_bwd(const float* x0, const float* dx0, int ncls, int64_t n, int t,
                         float* dlogits, int64_t ldd, hipStream_t stream) {
  PC_REQUIRE(x0 && dx0 && dlogits && n >= 0 && ncls >= 2 && ncls <= DD_MAXC && ldd >= ncls,
             "dual_input_bwd: bad shape (ncls = %d, ldd = %lld)", ncls, (long long)ldd);
  PC_REQUIRE(t >= PCADV_PWD_NONE && t <= PCADV_PWD_LOG_SOFTMAX, "dual_input_bwd: transform %d", t);
  if (n == 0) return PCADV_OK;
  hipLaunchKernelGGL(k_dd_input_bwd, dim3(grid_for(n)), dim3(DD_T), 0, stream, x0, dx0, ncls,
                     (long long)n, t, dlogits, (long long)ldd);
  PC_HIP_CHECK_LAUNCH("k_dd_input_bwd");
  return PCADV_OK;
}

int pcadv_lrelu_fwd(float* y, int64_t n, hipStream_t stream) {
  PC_REQUIRE(y && n >= 0, "lrelu_fwd: bad arguments");
  if (n == 0) return PCADV_OK;
  const int vec = al16(y);
  hipLaunchKernelGGL(k_dd_lrelu_fwd, dim3(grid_for(vec ? (n + 3) / 4 : n)), dim3(DD_T), 0, stream, y,
                     (long long)n, vec);
  PC_HIP_CHECK_LAUNCH("k_dd_lrelu_fwd");
  return PCADV_OK;
}

int pcadv_lrelu_bwd(float* d, const float* y, int64_t n, hipStream_t stream) {
  PC_REQUIRE(d && y && n >= 0, "lrelu_bwd: bad arguments");
  if (n == 0) return PCADV_OK;
  const int vec = al16(d) && al16(y);
  hipLaunchKernelGGL(k_dd_lrelu_bwd, dim3(grid_for(vec ? (n + 3) / 4 : n)), dim3(DD_T), 0, stream, d,
                     y, (long long)n, vec);
  PC_HIP_CHECK_LAUNCH("k_dd_lrelu_bwd");
  return PCADV_OK;
}

size_t pcadv_dual_point_tail_workspace_bytes(int64_t rows) {
  const size_t ntiles = (size_t)((rows + DD_ROWS - 1) / DD_ROWS);
  return 3 * (ntiles ? ntiles : 1) * sizeof(float) + 256;
}

int pcadv_dual_point_tail(const pcadv_dual_tail_args* a, hipStream_t stream) {
  PC_REQUIRE(a && a->y && a->out && a->argc, "dual_point_tail: y, out and argc are required");
  PC_REQUIRE(a->n0 >= 0 && a->n1 >= 0 && a->C >= 4 && a->C % 4 == 0 && a->C <= 4096 && al16(a->y),
             "dual_point_tail: n0 = %lld, n1 = %lld, C = %d (a multiple of 4, y 16-B aligned)",
             (long long)a->n0, (long long)a->n1, a->C);
  const long long M = a->n0 + a->n1;
  PC_REQUIRE(M < (1ll << 31), "dual_point_tail: %lld rows", M);
  if (M == 0) return PCADV_OK;
  const int ntiles = (int)((M + DD_ROWS - 1) / DD_ROWS);
  DdTail t{};
  t.y = a->y;
  t.C = a->C;
  t.n0 = a->n0;
  t.n1 = a->n1;
  t.out = a->out;
  t.argc = a->argc;
  t.want_loss = a->losses != nullptr;
  if (t.want_loss) {
    PC_REQUIRE(a->dout_d, "dual_point_tail: losses need dout_d");
    PC_REQUIRE(a->workspace && a->workspace_bytes >= pcadv_dual_point_tail_workspace_bytes(M),
               "dual_point_tail: workspace of %zu bytes, needs %zu", a->workspace_bytes,
               pcadv_dual_point_tail_workspace_bytes(M));
    PC_REQUIRE((!a->dz_d || al16(a->dz_d)) && (!a->dz_adv || al16(a->dz_adv)),
               "dual_point_tail: dz_d / dz_adv 16-B aligned");
    const bool drawn = (a->n0 > 0 && !a->soft0) || (a->n1 > 0 && !a->soft1);
    PC_REQUIRE(!drawn || a->step_count, "dual_point_tail: drawn labels need step_count");
    t.soft0 = a->soft0;
    t.soft1 = a->soft1;
    t.soft_out = a->soft_out;
    t.seed = a->rng_seed;
    t.step = a->step_count;
    t.dout_d = a->dout_d;
    t.dout_adv = a->dout_adv;
    t.lambda_adv = a->lambda_adv;
    t.dz_d = a->dz_d;
    t.dz_adv = a->dz_adv;
    t.partial = static_cast<float*>(a->workspace);
  }
  int grid = ntiles < 2048 ? ntiles : 2048;
  if (a->max_workgroups > 0 && grid > a->max_workgroups) grid = a->max_workgroups;
  hipLaunchKernelGGL(k_dd_tail, dim3(grid), dim3(DD_T), 0, stream, t, ntiles);
  PC_HIP_CHECK_LAUNCH("k_dd_tail");
  if (t.want_loss) {
    hipLaunchKernelGGL(k_dd_tail_fin, dim3(1), dim3(64), 0, stream, t.partial, ntiles,
                       (long long)a->n0, (long long)a->n1, a->losses);
    PC_HIP_CHECK_LAUNCH("k_dd_tail_fin");
  }
  return PCADV_OK;
}

int pcadv_sgd(float* p, const float* g, float* acc, int64_t n, float lr, hipStream_t stream) {
  PC_REQUIRE(p && g && n >= 0, "sgd: bad arguments");
  if (n == 0) return PCADV_OK;
  const int vec = al16(p) && al16(g) && (!acc || al16(acc));
  hipLaunchKernelGGL(k_dd_sgd, dim3(grid_for(vec ? (n + 3) / 4 : n)), dim3(DD_T), 0, stream, p, g,
                     acc, (long long)n, lr, vec);
  PC_HIP_CHECK_LAUNCH("k_dd_sgd");
  return PCADV_OK;
}

}  // extern "C"
