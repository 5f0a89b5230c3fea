// The semi-supervised term of run_training_seg_semi on the device
// (pcadv_row_semi_ce, utils/trainer.py:1999-2024): per row of the no-GT logits
// the pseudo-label (argmax, the first index on ties), kept where D's output is
// above the threshold; the mean cross entropy of the kept rows against their
// own pseudo-labels; and its gradient ADDED to dlogits.  Two launches: the
// first counts the kept rows and sums their losses per workgroup into fixed
// workspace slots, the second sums the slots in a fixed order (every workgroup
// the same way), so K is known before a gradient is written, and adds
// scale / K (softmax - onehot) to the kept rows.  Every slot is written on
// every call: the workspace never needs zeroing.  The row layout is
// k_row_eval's: sixteen lanes per row, four classes per lane.
//
// pcadv_row_semi_apply is the one-launch form for a caller that already holds K
// on the device (pcadv_stackdisc_forward_semi counts it in D's forward): the
// gradient pass alone, the same row code.
//
// The work per row is a handful of dependent steps (two loads, twelve
// cross-lane exchanges, an exp and a log), so a workgroup that walked many rows
// per slot would be bound by their latencies, not by memory: a workgroup takes
// as few rows as keep the grid within SM_MAXB workgroups (sixteen, one per
// slot, up to 32768 rows), and the second launch reads the slots with all its
// threads, SM_MAXB / SM_T independent loads each.
#include "common.h"

#include <cmath>

namespace pcadv {
namespace {

constexpr int SM_T = 256;    // threads per workgroup
constexpr int SM_LPR = 16;   // lanes per row: 4 classes each, ncls <= 64
constexpr int SM_SLOTS = SM_T / SM_LPR;  // rows in flight per workgroup
constexpr int SM_MAXB = 2048;  // workgroups (and workspace slots) per call, at most
constexpr int SM_WAVES = SM_T / 64;

struct RowSemi {
  const float* logits;
  long long ld;
  const float* d_out;
  float th, scale;
  float* dlogits;
  long long ldd;
  int32_t* labels_out;
  float* loss;
  int32_t* kept_out;
  int M, ncls;
  int rpb;  // rows per workgroup, a multiple of SM_SLOTS
  // workspace: one slot per workgroup
  double* part_ce;
  int32_t* part_k;
};

// One row by its sixteen lanes: the lane's four logits in v, the row's maximum
// bv and its first index bi, and es = the sum of exp(x - max) over the classes
// OTHER than bi (that one is exp(0) = 1 exactly), so the row's loss is
// log1p(es) and the pseudo-label's softmax - 1 is -es / (1 + es): neither
// cancels for a confident row.
template <bool VEC>
__device__ __forceinline__ void sm_row(const float* x, int c0, int ncls, float (&v)[4], float& bv,
                                       int& bi, float& es) {
  if (VEC && c0 + 4 <= ncls) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(x + c0);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c0 + j < ncls ? x[c0 + j] : -INFINITY;
  }
  bv = v[0];
  bi = c0;
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (ranks_before(v[j], c0 + j, bv, bi)) bv = v[j], bi = c0 + j;
#pragma unroll
  for (int o = SM_LPR / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, SM_LPR);
    const int oi = __shfl_xor(bi, o, SM_LPR);
    if (ranks_before(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  es = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) es += (c0 + j < ncls && c0 + j != bi) ? expf(v[j] - bv) : 0.f;
#pragma unroll
  for (int o = SM_LPR / 2; o > 0; o >>= 1) es += __shfl_xor(es, o, SM_LPR);
}

// A kept row's gradient coef (softmax - onehot), added to the lane's four
// columns of dlogits: k_row_semi_apply's statements, for k_row_semi_apply_dev
// (that kernel keeps its own copy, so that it compiles to what it did)
template <bool VEC>
__device__ __forceinline__ void sm_add_grad(const RowSemi& a, int r, int c0, float coef,
                                            const float (&v)[4], float bv, int bi, float es) {
  const float e = 1.f + es;
  float g[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) g[j] = coef * ((c0 + j == bi ? -es : expf(v[j] - bv)) / e);
  float* d = a.dlogits + (size_t)r * a.ldd + c0;
  if (VEC && c0 + 4 <= a.ncls) {
    f32x4 t = *reinterpret_cast<f32x4*>(d);
    t.x += g[0], t.y += g[1], t.z += g[2], t.w += g[3];
    *reinterpret_cast<f32x4*>(d) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < a.ncls) d[j] += g[j];
  }
}

// Launch 1: labels_out, and the workgroup's kept count and loss sum (f64, rows
// in order per slot, slots in order) into its workspace slot.  The threshold
// value and the row are loaded together (an ignored row's logits are read and
// dropped: one latency per row, not two).
template <bool VEC>
__global__ void __launch_bounds__(SM_T) k_row_semi_scan(const RowSemi a) {
  __shared__ double s_ce[SM_SLOTS];
  __shared__ int s_k[SM_SLOTS];
  const int tid = threadIdx.x, sub = tid & (SM_LPR - 1), slot = tid / SM_LPR;
  const int r0 = blockIdx.x * a.rpb, r1 = min(r0 + a.rpb, a.M);
  const int c0 = 4 * sub;
  double ce_sum = 0.0;
  int k = 0;
  for (int r = r0 + slot; r < r1; r += SM_SLOTS) {
    const bool keep = !(a.d_out[r] <= a.th);  // the row's sixteen lanes agree
    float v[4], bv, es;
    int bi;
    sm_row<VEC>(a.logits + (size_t)r * a.ld, c0, a.ncls, v, bv, bi, es);
    if (sub == 0) {
      if (keep) {
        ce_sum += (double)log1pf(es);
        ++k;
      }
      if (a.labels_out) a.labels_out[r] = keep ? bi : 255;
    }
  }
  if (sub == 0) {
    s_ce[slot] = ce_sum;
    s_k[slot] = k;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    int n = 0;
    for (int i = 0; i < SM_SLOTS; ++i) {
      s += s_ce[i];
      n += s_k[i];
    }
    a.part_ce[blockIdx.x] = s;
    a.part_k[blockIdx.x] = n;
  }
}

// Launch 2 (the same grid): every workgroup sums the workgroups' slots the same
// way (thread-strided, a butterfly per wave, the waves in order: one order for
// a given shape).  Workgroup 0 writes the loss and K; with K > 0 every
// workgroup adds its kept rows' gradients.
template <bool VEC>
__global__ void __launch_bounds__(SM_T) k_row_semi_apply(const RowSemi a) {
  __shared__ double s_ce[SM_WAVES];
  __shared__ int s_k[SM_WAVES];
  const int tid = threadIdx.x, sub = tid & (SM_LPR - 1), slot = tid / SM_LPR;
  const int nblk = gridDim.x;
  double s = 0.0;
  int n = 0;
#pragma unroll
  for (int i = 0; i < SM_MAXB / SM_T; ++i) {
    const int b = tid + i * SM_T;
    s += b < nblk ? a.part_ce[b] : 0.0;
    n += b < nblk ? a.part_k[b] : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // wave_sum (prims.h) of the two, interleaved
    s += __shfl_xor(s, o);
    n += __shfl_xor(n, o);
  }
  if ((tid & 63) == 0) s_ce[tid >> 6] = s, s_k[tid >> 6] = n;
  __syncthreads();
  double tot = 0.0;
  int K = 0;
#pragma unroll
  for (int w = 0; w < SM_WAVES; ++w) tot += s_ce[w], K += s_k[w];
  if (blockIdx.x == 0 && tid == 0) {
    *a.loss = K > 0 ? (float)(tot / (double)K) : 0.f;
    if (a.kept_out) *a.kept_out = K;
  }
  if (K == 0) return;
  const float coef = a.scale / (float)K;
  const int r0 = blockIdx.x * a.rpb, r1 = min(r0 + a.rpb, a.M);
  const int c0 = 4 * sub;
  for (int r = r0 + slot; r < r1; r += SM_SLOTS) {
    const bool keep = !(a.d_out[r] <= a.th);
    float v[4], bv, es;
    int bi;
    sm_row<VEC>(a.logits + (size_t)r * a.ld, c0, a.ncls, v, bv, bi, es);
    if (!keep) continue;  // after the row's exchanges: nothing of an ignored row is written
    const float e = 1.f + es;
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = coef * ((c0 + j == bi ? -es : expf(v[j] - bv)) / e);
    float* d = a.dlogits + (size_t)r * a.ldd + c0;
    if (VEC && c0 + 4 <= a.ncls) {
      f32x4 t = *reinterpret_cast<f32x4*>(d);
      t.x += g[0], t.y += g[1], t.z += g[2], t.w += g[3];
      *reinterpret_cast<f32x4*>(d) = t;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < a.ncls) d[j] += g[j];
    }
  }
}

// pcadv_row_semi_apply: k_row_semi_apply's second half alone, with K read from
// device memory (the stacked D's forward counted it, pwdisc.hip): no slot sum,
// no workspace.  labels_out is written for every row; with K <= 0 no row counts
// as kept (every label 255) and nothing else is written.
template <bool VEC>
__global__ void __launch_bounds__(SM_T) k_row_semi_apply_dev(const RowSemi a,
                                                             const int32_t* __restrict__ kept) {
  const int tid = threadIdx.x, sub = tid & (SM_LPR - 1), slot = tid / SM_LPR;
  const int K = *kept;
  const int r0 = blockIdx.x * a.rpb, r1 = min(r0 + a.rpb, a.M);
  if (K <= 0) {
    if (a.labels_out)
      for (int r = r0 + tid; r < r1; r += SM_T) a.labels_out[r] = 255;
    return;
  }
  const float coef = a.scale / (float)K;
  const int c0 = 4 * sub;
  for (int r = r0 + slot; r < r1; r += SM_SLOTS) {
    const bool keep = !(a.d_out[r] <= a.th);
    float v[4], bv, es;
    int bi;
    sm_row<VEC>(a.logits + (size_t)r * a.ld, c0, a.ncls, v, bv, bi, es);
    if (sub == 0 && a.labels_out) a.labels_out[r] = keep ? bi : 255;
    if (!keep) continue;
    sm_add_grad<VEC>(a, r, c0, coef, v, bv, bi, es);
  }
}

// rows per workgroup: the fewest (a multiple of SM_SLOTS) that keep the grid
// within SM_MAXB workgroups
int sm_rows_per_block(int M) {
  const long long per = ((long long)M + SM_MAXB - 1) / SM_MAXB;
  return (int)((per + SM_SLOTS - 1) / SM_SLOTS) * SM_SLOTS;
}

}  // namespace
}  // namespace pcadv

using namespace pcadv;

extern "C" {

size_t pcadv_row_semi_ce_workspace_bytes(int M) {
  (void)M;  // SM_MAXB slots whatever the shape
  return (size_t)SM_MAXB * (sizeof(double) + sizeof(int32_t)) + 256;
}

int pcadv_row_semi_ce(const float* logits, int64_t ld, const float* d_out, int M, int ncls,
                      float semi_th, float scale, float* dlogits, int64_t ldd,
                      int32_t* labels_out, float* loss, int32_t* kept_out, void* workspace,
                      size_t workspace_bytes, hipStream_t stream) {
  PC_REQUIRE(logits && d_out && dlogits && loss && M > 0 && ld >= ncls && ldd >= ncls,
             "row_semi_ce: bad shape");
  PC_REQUIRE(ncls >= 2 && ncls <= 4 * SM_LPR, "row_semi_ce: ncls %d outside 2..%d", ncls,
             4 * SM_LPR);
  PC_REQUIRE((long long)M * ld < (1LL << 40) && (long long)M * ldd < (1LL << 40),
             "row_semi_ce: logits too large");
  PC_REQUIRE(workspace && workspace_bytes >= pcadv_row_semi_ce_workspace_bytes(M) &&
                 (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "row_semi_ce: workspace (8-byte aligned, pcadv_row_semi_ce_workspace_bytes)");
  RowSemi a{};
  a.logits = logits, a.ld = ld, a.d_out = d_out, a.th = semi_th, a.scale = scale;
  a.dlogits = dlogits, a.ldd = ldd, a.labels_out = labels_out, a.loss = loss;
  a.kept_out = kept_out, a.M = M, a.ncls = ncls;
  a.rpb = sm_rows_per_block(M);
  const int nblk = (M + a.rpb - 1) / a.rpb;
  PC_REQUIRE(nblk >= 1 && nblk <= SM_MAXB, "row_semi_ce: internal: %d workgroups", nblk);
  a.part_ce = static_cast<double*>(workspace);
  a.part_k = reinterpret_cast<int32_t*>(a.part_ce + SM_MAXB);
  const bool vec = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits)) &
                    15) == 0 && ld % 4 == 0 && ldd % 4 == 0;
  if (vec) {
    hipLaunchKernelGGL(k_row_semi_scan<true>, dim3(nblk), dim3(SM_T), 0, stream, a);
    PC_HIP_CHECK_LAUNCH("k_row_semi_scan");
    hipLaunchKernelGGL(k_row_semi_apply<true>, dim3(nblk), dim3(SM_T), 0, stream, a);
  } else {
    hipLaunchKernelGGL(k_row_semi_scan<false>, dim3(nblk), dim3(SM_T), 0, stream, a);
    PC_HIP_CHECK_LAUNCH("k_row_semi_scan");
    hipLaunchKernelGGL(k_row_semi_apply<false>, dim3(nblk), dim3(SM_T), 0, stream, a);
  }
  PC_HIP_CHECK_LAUNCH("k_row_semi_apply");
  return PCADV_OK;
}

int pcadv_row_semi_apply(const float* logits, int64_t ld, const float* d_out, int M, int ncls,
                         float semi_th, float scale, const int32_t* kept, float* dlogits,
                         int64_t ldd, int32_t* labels_out, hipStream_t stream) {
  PC_REQUIRE(logits && d_out && dlogits && kept && M > 0 && ld >= ncls && ldd >= ncls,
             "row_semi_apply: bad shape");
  PC_REQUIRE(ncls >= 2 && ncls <= 4 * SM_LPR, "row_semi_apply: ncls %d outside 2..%d", ncls,
             4 * SM_LPR);
  PC_REQUIRE((long long)M * ld < (1LL << 40) && (long long)M * ldd < (1LL << 40),
             "row_semi_apply: logits too large");
  PC_REQUIRE((reinterpret_cast<uintptr_t>(kept) & 3) == 0, "row_semi_apply: kept is not 4-B aligned");
  RowSemi a{};
  a.logits = logits, a.ld = ld, a.d_out = d_out, a.th = semi_th, a.scale = scale;
  a.dlogits = dlogits, a.ldd = ldd, a.labels_out = labels_out, a.M = M, a.ncls = ncls;
  a.rpb = sm_rows_per_block(M);
  const int nblk = (M + a.rpb - 1) / a.rpb;
  PC_REQUIRE(nblk >= 1 && nblk <= SM_MAXB, "row_semi_apply: internal: %d workgroups", nblk);
  const bool vec = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits)) &
                    15) == 0 && ld % 4 == 0 && ldd % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(k_row_semi_apply_dev<true>, dim3(nblk), dim3(SM_T), 0, stream, a, kept);
  else
    hipLaunchKernelGGL(k_row_semi_apply_dev<false>, dim3(nblk), dim3(SM_T), 0, stream, a, kept);
  PC_HIP_CHECK_LAUNCH("k_row_semi_apply_dev");
  return PCADV_OK;
}

}  // extern "C"
