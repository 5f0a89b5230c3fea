// Evaluation metrics on the device (pcadv_row_eval): per row of a logits
// matrix the argmax (first index on ties, as np.argmax / torch.max give), the
// cross entropy against the label and whether the prediction is right; per
// call the batch's sums into a caller-owned accumulator; and, for rows grouped
// into clouds, each cloud's mean part IoU (utils/metric.py:19-30) from integer
// counts.  The test passes of the trainers (evaluate.py) run it after the
// forward, inside the batch's graph: nothing is copied to the host per batch.
#include "common.h"

#include <cmath>

namespace pcadv {
namespace {

constexpr int EV_T = 256;     // threads per workgroup
constexpr int EV_LPR = 16;    // lanes per row: 4 classes each, ncls <= 64
constexpr int EV_SLOTS = EV_T / EV_LPR;  // rows in flight per workgroup
constexpr int EV_ROWS = 256;  // rows per workgroup (at most; whole clouds when they fit)
constexpr int EV_MAXP = 8;    // parts per category (metric.seg_classes: at most 6)

struct RowEval {
  const float* logits;
  long long ld;
  const int64_t* labels;
  int M, ncls;
  int32_t* pred;
  // IoU (N > 0): clouds of N rows.  chunks == 0: a workgroup takes gpb whole
  // clouds (N <= EV_ROWS) and finishes them itself; chunks > 0: chunks
  // workgroups per cloud, their counts in fixed slots, finished by k_row_eval_fin
  int N, ngroups, gpb, chunks;
  const int64_t* group_cat;
  long long cat_stride;
  const int32_t* cat_parts;
  int ncat;
  const int32_t* cursor;
  double* iou_out;
  int32_t* cat_out;
  double* acc;
  // workspace: one slot per workgroup
  double* part_ce;
  int32_t* part_ok;
  int32_t* part_iou;  // [workgroup][EV_MAXP][I, U]
};

// metric.get_iou from a cloud's counts: a part absent from both counts 1, the
// parts summed in order from 0.0 and divided by their number (np.mean over
// fewer than 8 values is that sequential sum), so the f64 result is the host's.
__device__ __forceinline__ double ev_iou(const int* cnt, int count) {
  if (count < 0) return NAN;  // category outside [0, ncat)
  double s = 0.0;
  for (int p = 0; p < count; ++p) {
    const int I = cnt[2 * p], U = cnt[2 * p + 1];
    s += U == 0 ? 1.0 : (double)I / (double)U;
  }
  return s / (double)count;
}

// The parts (first, count) of cloud g; count -1 for a category out of range.
__device__ __forceinline__ void ev_parts(const RowEval& a, int g, int& first, int& count,
                                         int64_t& cat) {
  cat = a.group_cat[(long long)g * a.cat_stride];
  first = 0;
  count = -1;
  if (cat >= 0 && cat < a.ncat) {
    first = a.cat_parts[2 * cat];
    count = min(max(a.cat_parts[2 * cat + 1], 0), EV_MAXP);
  }
}

__device__ __forceinline__ void ev_write_iou(const RowEval& a, int g, const int* cnt, int count,
                                             int64_t cat) {
  const long long at = (a.cursor ? (long long)*a.cursor * a.ngroups : 0) + g;
  a.iou_out[at] = ev_iou(cnt, count);
  a.cat_out[at] = (int32_t)cat;
}

// The call's sums into acc, by the first wave of a workgroup: the workgroups'
// slots summed lane-strided then by a butterfly, a fixed order for a given
// shape (no floating-point atomics: two runs give the same bits).
__device__ __forceinline__ void ev_finish_acc(const RowEval& a, int nblk, int lane) {
  double s = 0.0;
  long long ok = 0;
  for (int b = lane; b < nblk; b += 64) {
    s += a.part_ce[b];
    ok += a.part_ok[b];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // wave_sum (prims.h) of the two, interleaved
    s += __shfl_xor(s, o);
    ok += __shfl_xor(ok, o);
  }
  if (lane == 0) {
    a.acc[0] += (double)ok;
    a.acc[1] += (double)(float)(s / (double)a.M);  // the batch's f32 mean (loss.item())
    a.acc[2] += (double)a.M;
    a.acc[3] += 1.0;
  }
}

// Sixteen lanes per row, four classes per lane (one 16-byte load where VEC:
// 16-byte aligned rows), sixteen rows in flight per workgroup.  The max and the
// exp sum are butterflies over the row's lanes; the row's leader lane keeps the
// CE sum (f64, in row order) and the right-prediction count in registers and
// counts the IoU intersections / unions with LDS integer atomics.
template <bool VEC>
__global__ void __launch_bounds__(EV_T) k_row_eval(const RowEval a) {
  __shared__ int cnt[EV_ROWS][2 * EV_MAXP];
  __shared__ int gfirst[EV_ROWS], gcount[EV_ROWS];
  __shared__ double s_ce[EV_SLOTS];
  __shared__ int s_ok[EV_SLOTS];
  const int tid = threadIdx.x, sub = tid & (EV_LPR - 1), slot = tid / EV_LPR;
  int g0 = 0, ng = 0, r0, r1;
  if (a.N > 0) {
    if (a.chunks) {
      g0 = blockIdx.x / a.chunks;
      ng = 1;
      r0 = g0 * a.N + (int)(blockIdx.x % a.chunks) * EV_ROWS;
      r1 = min(r0 + EV_ROWS, (g0 + 1) * a.N);
    } else {
      g0 = blockIdx.x * a.gpb;
      ng = min(a.gpb, a.ngroups - g0);
      r0 = g0 * a.N;
      r1 = r0 + ng * a.N;
    }
    for (int i = tid; i < ng * 2 * EV_MAXP; i += EV_T) (&cnt[0][0])[i] = 0;
    if (tid < ng) {
      int64_t cat;
      ev_parts(a, g0 + tid, gfirst[tid], gcount[tid], cat);
    }
    __syncthreads();
  } else {
    r0 = blockIdx.x * EV_ROWS;
    r1 = min(r0 + EV_ROWS, a.M);
  }
  double ce_sum = 0.0;
  int ok = 0;
  const int c0 = 4 * sub;
  for (int r = r0 + slot; r < r1; r += EV_SLOTS) {
    const float* x = a.logits + (size_t)r * a.ld;
    float v[4];
    if (VEC && c0 + 4 <= a.ncls) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(x + c0);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < a.ncls ? x[c0 + j] : -INFINITY;
    }
    const int64_t y = a.labels[r];
    float bv = v[0];
    int bi = c0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (ranks_before(v[j], c0 + j, bv, bi)) bv = v[j], bi = c0 + j;
#pragma unroll
    for (int o = EV_LPR / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, EV_LPR);
      const int oi = __shfl_xor(bi, o, EV_LPR);
      if (ranks_before(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) e += c0 + j < a.ncls ? expf(v[j] - bv) : 0.f;
#pragma unroll
    for (int o = EV_LPR / 2; o > 0; o >>= 1) e += __shfl_xor(e, o, EV_LPR);
    const float lse = bv + logf(e);
    const bool inr = y >= 0 && y < a.ncls;
    const int yy = inr ? (int)y : 0;
    const int yj = yy & 3;
    const float mine = yj == 0 ? v[0] : yj == 1 ? v[1] : yj == 2 ? v[2] : v[3];
    const float xy = __shfl(mine, yy >> 2, EV_LPR);
    if (sub == 0) {
      ce_sum += (double)(inr ? lse - xy : NAN);  // a label outside [0, ncls) is loud
      ok += (inr && bi == yy) ? 1 : 0;
      if (a.pred) a.pred[r] = bi;
      if (a.N > 0) {
        const int gl = a.chunks ? 0 : (r - r0) / a.N;
        const int first = gfirst[gl], count = gcount[gl];
        const int pg = yy - first, pp = bi - first;
        const bool gin = inr && pg >= 0 && pg < count, pin = pp >= 0 && pp < count;
        if (gin && pin && pg == pp) {
          atomicAdd(&cnt[gl][2 * pg], 1);
          atomicAdd(&cnt[gl][2 * pg + 1], 1);
        } else {
          if (gin) atomicAdd(&cnt[gl][2 * pg + 1], 1);
          if (pin) atomicAdd(&cnt[gl][2 * pp + 1], 1);
        }
      }
    }
  }
  if (sub == 0) {
    s_ce[slot] = ce_sum;
    s_ok[slot] = ok;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    int k = 0;
    for (int i = 0; i < EV_SLOTS; ++i) {
      s += s_ce[i];
      k += s_ok[i];
    }
    a.part_ce[blockIdx.x] = s;
    a.part_ok[blockIdx.x] = k;
  }
  if (a.N > 0) {
    if (a.chunks) {
      if (tid < 2 * EV_MAXP) a.part_iou[(size_t)blockIdx.x * 2 * EV_MAXP + tid] = cnt[0][tid];
    } else if (tid < ng) {
      ev_write_iou(a, g0 + tid, cnt[tid], gcount[tid],
                   a.group_cat[(long long)(g0 + tid) * a.cat_stride]);
    }
  }
  // one workgroup: it is also the finishing wave (lane 0 reads its own slot)
  if (gridDim.x == 1 && tid < 64) ev_finish_acc(a, 1, tid);
}

// After several workgroups: workgroup 0's first wave sums their slots into
// acc; with clouds cut into chunks, workgroups 1.. take a cloud per thread, add
// its chunks' counts and write its IoU record.
__global__ void __launch_bounds__(EV_T) k_row_eval_fin(const RowEval a, int nblk) {
  if (blockIdx.x == 0) {
    if (threadIdx.x < 64) ev_finish_acc(a, nblk, threadIdx.x);
    return;
  }
  const int g = (blockIdx.x - 1) * EV_T + threadIdx.x;
  if (g >= a.ngroups) return;
  int cnt[2 * EV_MAXP];
#pragma unroll
  for (int i = 0; i < 2 * EV_MAXP; ++i) cnt[i] = 0;
  for (int ch = 0; ch < a.chunks; ++ch) {
    const int32_t* p = a.part_iou + ((size_t)g * a.chunks + ch) * 2 * EV_MAXP;
#pragma unroll
    for (int i = 0; i < 2 * EV_MAXP; ++i) cnt[i] += p[i];
  }
  int first, count;
  int64_t cat;
  ev_parts(a, g, first, count, cat);
  ev_write_iou(a, g, cnt, count, cat);
}

// workgroups of a call are at most M / 128 + 1 (whole clouds per workgroup fill
// more than half of EV_ROWS; chunked clouds add fewer than one workgroup each)
size_t ev_max_blocks(int M) { return (size_t)(M > 0 ? M : 0) / (EV_ROWS / 2) + 1; }

}  // namespace
}  // namespace pcadv

using namespace pcadv;

extern "C" {

size_t pcadv_row_eval_workspace_bytes(int M) {
  return ev_max_blocks(M) * (sizeof(double) + sizeof(int32_t) * (1 + 2 * EV_MAXP)) + 256;
}

int pcadv_row_eval(const float* logits, int64_t ld, const int64_t* labels, int M, int ncls,
                   int32_t* pred, int rows_per_group, const int64_t* group_cat,
                   int64_t cat_stride, const int32_t* cat_parts, int ncat, const int32_t* cursor,
                   double* iou_out, int32_t* cat_out, double* acc, void* workspace,
                   size_t workspace_bytes, hipStream_t stream) {
  PC_REQUIRE(logits && labels && M > 0 && ld >= ncls, "row_eval: bad shape");
  PC_REQUIRE(ncls >= 2 && ncls <= 4 * EV_LPR, "row_eval: ncls %d outside 2..%d", ncls,
             4 * EV_LPR);
  PC_REQUIRE(acc, "row_eval: acc (double[4]) required");
  PC_REQUIRE((long long)M * ld < (1LL << 40), "row_eval: logits too large");
  const int N = rows_per_group;
  PC_REQUIRE(N >= 0, "row_eval: rows_per_group %d < 0", N);
  if (N > 0) {
    PC_REQUIRE(M % N == 0, "row_eval: M %d is not a multiple of rows_per_group %d", M, N);
    PC_REQUIRE(group_cat && cat_stride >= 1 && cat_parts && ncat > 0 && iou_out && cat_out,
               "row_eval: the IoU part needs group_cat, cat_stride >= 1, cat_parts, ncat > 0, "
               "iou_out and cat_out");
  }
  PC_REQUIRE(workspace && workspace_bytes >= pcadv_row_eval_workspace_bytes(M) &&
                 (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "row_eval: workspace (8-byte aligned, pcadv_row_eval_workspace_bytes)");
  RowEval a{};
  a.logits = logits, a.ld = ld, a.labels = labels, a.M = M, a.ncls = ncls, a.pred = pred;
  a.N = N, a.group_cat = group_cat, a.cat_stride = cat_stride, a.cat_parts = cat_parts;
  a.ncat = ncat, a.cursor = cursor, a.iou_out = iou_out, a.cat_out = cat_out, a.acc = acc;
  int nblk = (M + EV_ROWS - 1) / EV_ROWS;
  if (N > 0) {
    a.ngroups = M / N;
    if (N <= EV_ROWS) {
      a.gpb = EV_ROWS / N;
      nblk = (a.ngroups + a.gpb - 1) / a.gpb;
    } else {
      a.chunks = (N + EV_ROWS - 1) / EV_ROWS;
      nblk = a.ngroups * a.chunks;
    }
  }
  const size_t nmax = ev_max_blocks(M);
  PC_REQUIRE((size_t)nblk <= nmax, "row_eval: internal: %d workgroups", nblk);
  a.part_ce = static_cast<double*>(workspace);
  a.part_iou = reinterpret_cast<int32_t*>(a.part_ce + nmax);
  a.part_ok = a.part_iou + nmax * 2 * EV_MAXP;
  const bool vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && ld % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(k_row_eval<true>, dim3(nblk), dim3(EV_T), 0, stream, a);
  else
    hipLaunchKernelGGL(k_row_eval<false>, dim3(nblk), dim3(EV_T), 0, stream, a);
  PC_HIP_CHECK_LAUNCH("k_row_eval");
  if (nblk > 1) {
    const int extra = a.chunks ? (a.ngroups + EV_T - 1) / EV_T : 0;
    hipLaunchKernelGGL(k_row_eval_fin, dim3(1 + extra), dim3(EV_T), 0, stream, a, nblk);
    PC_HIP_CHECK_LAUNCH("k_row_eval_fin");
  }
  return PCADV_OK;
}

}  // extern "C"
