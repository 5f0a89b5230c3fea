// The T-Net glue of the regularised segmentation generator
// (PointNetSeg_regulization, models/pointnet.py:205-259;
// run_training_seg_stack_regulization, utils/trainer.py:1218-1429):
//
//   pcadv_cloud_xform_fwd   y = x T per cloud (torch.bmm, pointnet.py:231,238)
//   pcadv_cloud_xform_bwd   dT = x^T dy per cloud, dx += (dy T^T + add) [x > 0]
//   pcadv_tnet_mse_reg      MSELoss(T T^T, I) per batch and its gradient
//
// Rows are points, point-major, with caller-given row strides (the x3 column
// block of the [B*N][960] buffer is read and its gradient accumulated in
// place).  k = 128 runs on exact f32 MFMAs (32x32x2), k = 3 on VALU FMAs.
// Every sum runs in a fixed order: no atomics, bitwise reproducible.
#include "common.h"

namespace pcadv {
namespace {

constexpr int XK = 128;      // the feature transform's width
constexpr int XROWS = 32;    // rows of one MFMA tile
constexpr int XTILES = 4;    // row tiles one workgroup walks (its T fragments loaded once)
constexpr int XTHREADS = 256;

// k = 128, 4 waves: wave w owns columns [32 w, 32 w + 32) of a 32-row tile.
// BWD = false: y[n][j] = sum_i x[n][i] T[i][j].
// BWD = true:  dx[n][i] += (sum_j dy[n][j] T[i][j] + add[n][i]) * [x[n][i] > 0 if relu_x].
// The reduction index is walked in the order of mfma_rows_x_wt (common.h):
// per group of 8, (0, 4), (1, 5), (2, 6), (3, 7): one f32 fma chain.
template <bool BWD>
__global__ __launch_bounds__(XTHREADS) void k_xform128(
    const float* __restrict__ src, int64_t lds_, const float* __restrict__ T, float* dst,
    int64_t ldd, const float* __restrict__ add, const float* __restrict__ xmask, int64_t ldm,
    int relu_x, int Npts) {
  __shared__ float tile[XROWS * S128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int cloud = blockIdx.y;
  const int col0 = 32 * wave;
  const float* Tc = T + (size_t)cloud * XK * XK;
  const size_t row_base = (size_t)cloud * Npts;

  f32x4 bfrag[XK / 8];
  if (BWD) {
    load_bfrag<XK>(Tc, col0, lane, bfrag);  // B[k = j][col = i] = T[i][j]
  } else {
#pragma unroll
    for (int g = 0; g < XK / 8; ++g) {      // B[k = i][col = j] = T[i][j]
      const float* p = Tc + (size_t)(8 * g + 4 * h) * XK + col0 + r;
      bfrag[g].x = p[0];
      bfrag[g].y = p[XK];
      bfrag[g].z = p[2 * XK];
      bfrag[g].w = p[3 * XK];
    }
  }

  for (int t = 0; t < XTILES; ++t) {
    const int n0 = (blockIdx.x * XTILES + t) * XROWS;
    if (n0 >= Npts) break;  // uniform over the workgroup
    __syncthreads();
    for (int idx = tid; idx < XROWS * XK; idx += XTHREADS) {
      const int rr = idx >> 7, cc = idx & (XK - 1);
      const int n = n0 + rr;
      tile[rr * S128 + cc] = n < Npts ? src[(row_base + n) * lds_ + cc] : 0.f;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    acc = mfma_rows_x_wt<XK>(tile, S128, bfrag, acc, lane);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = n0 + acc_row(q, lane);
      if (n >= Npts) continue;
      const int c = col0 + r;
      float* o = dst + (row_base + n) * ldd + c;
      if (BWD) {
        float v = acc[q];
        if (add) v += add[(row_base + n) * XK + c];
        if (relu_x && !(xmask[(row_base + n) * ldm + c] > 0.f)) v = 0.f;
        *o = *o + v;
      } else {
        *o = acc[q];
      }
    }
  }
}

// dT[c][i][j] (+)= sum_n x[c][n][i] dy[c][n][j], k = 128: workgroup (bx, c)
// owns the 32 x 32 tile (bx >> 2, bx & 3) of dT_c; its wave w sums the w-th
// quarter of the cloud's points as one f32 fma chain in increasing order, and
// the four partial tiles are added in wave order: ((p0 + p1) + p2) + p3.
__global__ __launch_bounds__(XTHREADS) void k_xform128_dT(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ dy, int64_t lddy,
    float* __restrict__ dT, int accumulate, int Npts) {
  __shared__ float part[4][32][33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int cloud = blockIdx.y;
  const int i0 = 32 * (blockIdx.x >> 2), j0 = 32 * (blockIdx.x & 3);
  const size_t row_base = (size_t)cloud * Npts;
  const float* xa = x + row_base * ldx + i0 + r;
  const float* da = dy + row_base * lddy + j0 + r;
  const int quarter = 2 * ((Npts + 7) / 8);  // even: an MFMA step takes two points
  const int n_lo = wave * quarter;
  const int n_hi = min(n_lo + quarter, Npts);
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  constexpr int U = 8;  // loads of U MFMA steps in flight
  for (int n0 = n_lo; n0 < n_hi; n0 += 2 * U) {
    float a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = n0 + 2 * u + h;
      const bool in = n < n_hi;
      a[u] = in ? xa[(size_t)n * ldx] : 0.f;
      b[u] = in ? da[(size_t)n * lddy] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = mfma32(a[u], b[u], acc);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) part[wave][acc_row(q, lane)][r] = acc[q];
  __syncthreads();
  float* out = dT + (size_t)cloud * XK * XK;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + XTHREADS * q, row = e >> 5, col = e & 31;
    const float v = ((part[0][row][col] + part[1][row][col]) + part[2][row][col]) + part[3][row][col];
    float* o = out + (size_t)(i0 + row) * XK + j0 + col;
    *o = accumulate ? *o + v : v;
  }
}

// ---- k = 3: plain FMAs -------------------------------------------------------
__global__ __launch_bounds__(256) void k_xform3_fwd(const float* __restrict__ x, int64_t ldx,
                                                    const float* __restrict__ T, float* y,
                                                    int64_t ldy, int Npts, int64_t rows) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= rows) return;
  const float* t = T + (m / Npts) * 9;
  const float* p = x + m * ldx;
  const float p0 = p[0], p1 = p[1], p2 = p[2];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    y[m * ldy + j] = fmaf(p2, t[6 + j], fmaf(p1, t[3 + j], p0 * t[j]));
}

__global__ __launch_bounds__(256) void k_xform3_dx(
    const float* __restrict__ dy, int64_t lddy, const float* __restrict__ T, float* dx,
    int64_t lddx, const float* __restrict__ add, const float* __restrict__ xmask, int64_t ldm,
    int relu_x, int Npts, int64_t rows) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= rows) return;
  const float* t = T + (m / Npts) * 9;
  const float* g = dy + m * lddy;
  const float g0 = g[0], g1 = g[1], g2 = g[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float v = fmaf(g2, t[3 * i + 2], fmaf(g1, t[3 * i + 1], g0 * t[3 * i]));
    if (add) v += add[m * 3 + i];
    if (relu_x && !(xmask[m * ldm + i] > 0.f)) v = 0.f;
    dx[m * lddx + i] += v;
  }
}

// dT[c] (3 x 3), one workgroup per cloud: thread t sums the points t, t + 256,
// ... in increasing order, then a fixed binary tree over the 256 partials.
__global__ __launch_bounds__(256) void k_xform3_dT(const float* __restrict__ x, int64_t ldx,
                                                   const float* __restrict__ dy, int64_t lddy,
                                                   float* __restrict__ dT, int accumulate,
                                                   int Npts) {
  __shared__ float part[9][256];
  const int tid = threadIdx.x, cloud = blockIdx.x;
  const size_t row_base = (size_t)cloud * Npts;
  float s[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) s[q] = 0.f;
  for (int n = tid; n < Npts; n += 256) {
    const float* p = x + (row_base + n) * ldx;
    const float* g = dy + (row_base + n) * lddy;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) s[3 * i + j] = fmaf(p[i], g[j], s[3 * i + j]);
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) part[q][tid] = s[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w)
#pragma unroll
      for (int q = 0; q < 9; ++q) part[q][tid] += part[q][tid + w];
    __syncthreads();
  }
  if (tid < 9) {
    float* o = dT + (size_t)cloud * 9 + tid;
    *o = accumulate ? *o + part[tid][0] : part[tid][0];
  }
}

// ---- MSELoss(T T^T, I) ---------------------------------------------------------
// Workgroup (rb, c) owns the rows [32 rb, 32 rb + 32) of cloud c's S = T T^T - I
// and of G = S T (row i of G needs row i of S only).  T sits in LDS whole, the
// S rows beside it, both with rows of k + 1 floats (the column walks of T T^T
// stay conflict-free).  Element e of the row block belongs to thread
// e % REG_THREADS; every dot product runs over its index in increasing order.
// part_sum[c][rb] = the block's sum of S_ij^2 (a fixed tree over the threads'
// partials); dT_c += coef_g (S T_c) where S T_c is non-zero.
constexpr int REG_THREADS = 1024;
constexpr int REG_ROWS = 32;
constexpr int REG_MAXRB = 4;  // row blocks of a cloud at k = 128

__global__ __launch_bounds__(REG_THREADS) void k_mse_reg(const float* __restrict__ T, int k,
                                                         int B0, int C, float scale,
                                                         float* __restrict__ dT,
                                                         float* __restrict__ part_sum) {
  extern __shared__ float lds[];
  const int ld = k + 1;
  float* Ts = lds;
  float* Ss = lds + k * ld;
  __shared__ float red[REG_THREADS];
  const int tid = threadIdx.x, cloud = blockIdx.y;
  const int i0 = REG_ROWS * blockIdx.x;
  const int rows = min(REG_ROWS, k - i0);
  const float* Tc = T + (size_t)cloud * k * k;
  const int kk = k * k, ne = rows * k;
  for (int e = tid; e < kk; e += REG_THREADS) Ts[(e / k) * ld + e % k] = Tc[e];
  __syncthreads();
  float sq = 0.f;
  for (int e = tid; e < ne; e += REG_THREADS) {
    const int il = e / k, i = i0 + il, j = e % k;
    float s = 0.f;
    for (int m = 0; m < k; ++m) s = fmaf(Ts[i * ld + m], Ts[j * ld + m], s);
    if (i == j) s -= 1.f;
    Ss[il * ld + j] = s;
    sq = fmaf(s, s, sq);
  }
  red[tid] = sq;
  __syncthreads();
  for (int w = REG_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) part_sum[cloud * REG_MAXRB + blockIdx.x] = red[0];
  if (!dT) return;
  const int Bg = cloud < B0 ? B0 : C - B0;
  const float coef = scale * (4.f / ((float)Bg * (float)kk));
  float* dTc = dT + (size_t)cloud * kk + (size_t)i0 * k;
  for (int e = tid; e < ne; e += REG_THREADS) {
    const int il = e / k, j = e % k;
    float g = 0.f;
    for (int m = 0; m < k; ++m) g = fmaf(Ss[il * ld + m], Ts[m * ld + j], g);
    if (g != 0.f) dTc[e] += coef * g;  // T T^T = I: not even a -0 + 0 touches dT
  }
}

// loss[g] = (sum of the group's row-block sums, in cloud and row order) / (B_g k^2)
__global__ void k_mse_reg_finish(const float* __restrict__ part_sum, int k, int B0, int C,
                                 float* __restrict__ loss) {
  const int g = threadIdx.x;
  if (g > 1) return;
  const int lo = g ? B0 : 0, hi = g ? C : B0;
  const int nrb = (k + REG_ROWS - 1) / REG_ROWS;
  float s = 0.f;
  for (int c = lo; c < hi; ++c)
    for (int rb = 0; rb < nrb; ++rb) s += part_sum[c * REG_MAXRB + rb];
  loss[g] = hi > lo ? s / ((float)(hi - lo) * (float)(k * k)) : 0.f;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace pcadv

using namespace pcadv;

extern "C" {

int pcadv_cloud_xform_fwd(const float* x, int64_t ldx, const float* T, float* y, int64_t ldy,
                          int C, int Npts, int k, hipStream_t stream) {
  PC_REQUIRE(k == 3 || k == XK, "cloud_xform_fwd: k = %d (3 or 128)", k);
  PC_REQUIRE(C >= 0 && Npts >= 0, "cloud_xform_fwd: C = %d, Npts = %d", C, Npts);
  PC_REQUIRE((int64_t)C * Npts < (int64_t)1 << 31, "cloud_xform_fwd: C * Npts = %lld rows",
             (long long)C * Npts);
  PC_REQUIRE(ldx >= k && ldy >= k, "cloud_xform_fwd: ldx = %lld, ldy = %lld below k = %d",
             (long long)ldx, (long long)ldy, k);
  if (C == 0 || Npts == 0) return PCADV_OK;
  PC_REQUIRE(x && T && y, "cloud_xform_fwd: x, T and y are required");
  if (k == 3) {
    const int64_t rows = (int64_t)C * Npts;
    k_xform3_fwd<<<dim3((unsigned)((rows + 255) / 256)), 256, 0, stream>>>(x, ldx, T, y, ldy,
                                                                           Npts, rows);
  } else {
    const dim3 grid((Npts + XROWS * XTILES - 1) / (XROWS * XTILES), C);
    k_xform128<false><<<grid, XTHREADS, 0, stream>>>(x, ldx, T, y, ldy, nullptr, nullptr, 0, 0,
                                                     Npts);
  }
  PC_HIP_CHECK_LAUNCH("cloud_xform_fwd");
  return PCADV_OK;
}

int pcadv_cloud_xform_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                          const float* T, float* dT, int accumulate, float* dx, int64_t lddx,
                          const float* add, int relu_x, int C, int Npts, int k,
                          hipStream_t stream) {
  PC_REQUIRE(k == 3 || k == XK, "cloud_xform_bwd: k = %d (3 or 128)", k);
  PC_REQUIRE(C >= 0 && Npts >= 0, "cloud_xform_bwd: C = %d, Npts = %d", C, Npts);
  PC_REQUIRE((int64_t)C * Npts < (int64_t)1 << 31, "cloud_xform_bwd: C * Npts = %lld rows",
             (long long)C * Npts);
  PC_REQUIRE(lddy >= k && ldx >= k, "cloud_xform_bwd: lddy = %lld, ldx = %lld below k = %d",
             (long long)lddy, (long long)ldx, k);
  PC_REQUIRE(!dx || lddx >= k, "cloud_xform_bwd: lddx = %lld below k = %d", (long long)lddx, k);
  PC_REQUIRE(dx || !add, "cloud_xform_bwd: add without dx");
  PC_REQUIRE(dT || dx, "cloud_xform_bwd: neither dT nor dx");
  if (C == 0 || Npts == 0) return PCADV_OK;
  PC_REQUIRE(dy && x && T, "cloud_xform_bwd: dy, x and T are required");
  PC_REQUIRE(k == 3 || !dx || aligned16(T), "cloud_xform_bwd: T must be 16-byte aligned");
  const int64_t rows = (int64_t)C * Npts;
  if (dT) {
    if (k == 3)
      k_xform3_dT<<<dim3(C), 256, 0, stream>>>(x, ldx, dy, lddy, dT, accumulate, Npts);
    else
      k_xform128_dT<<<dim3((XK / 32) * (XK / 32), C), XTHREADS, 0, stream>>>(x, ldx, dy, lddy, dT, accumulate,
                                                               Npts);
    PC_HIP_CHECK_LAUNCH("cloud_xform_bwd (dT)");
  }
  if (dx) {
    if (k == 3) {
      k_xform3_dx<<<dim3((unsigned)((rows + 255) / 256)), 256, 0, stream>>>(
          dy, lddy, T, dx, lddx, add, x, ldx, relu_x, Npts, rows);
    } else {
      const dim3 grid((Npts + XROWS * XTILES - 1) / (XROWS * XTILES), C);
      k_xform128<true><<<grid, XTHREADS, 0, stream>>>(dy, lddy, T, dx, lddx, add, x, ldx, relu_x,
                                                      Npts);
    }
    PC_HIP_CHECK_LAUNCH("cloud_xform_bwd (dx)");
  }
  return PCADV_OK;
}

int pcadv_tnet_mse_reg(const float* T, int C, int B0, int k, float scale, float* loss, float* dT,
                       float* workspace, hipStream_t stream) {
  PC_REQUIRE(k == 3 || (k >= 4 && k <= 128 && k % 4 == 0),
             "tnet_mse_reg: k = %d (3, or a multiple of 4 up to 128)", k);
  PC_REQUIRE(C >= 0 && B0 >= 0 && B0 <= C, "tnet_mse_reg: C = %d, B0 = %d", C, B0);
  if (C == 0) return PCADV_OK;
  PC_REQUIRE(B0 >= 1, "tnet_mse_reg: group 0 is empty (B0 = 0 of C = %d)", C);
  PC_REQUIRE(T && loss && workspace, "tnet_mse_reg: T, loss and workspace are required");
  const size_t bytes = (size_t)(k + REG_ROWS) * (k + 1) * sizeof(float);
  static bool attr = false;  // once, for the largest k: nothing is set during a later capture
  if (!attr) {
    const size_t most = (size_t)(128 + REG_ROWS) * (128 + 1) * sizeof(float);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_mse_reg),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)most) != hipSuccess) {
      (void)hipGetLastError();
      set_error("tnet_mse_reg: cannot reserve %zu bytes of LDS", most);
      return PCADV_EHIP;
    }
    attr = true;
  }
  k_mse_reg<<<dim3((k + REG_ROWS - 1) / REG_ROWS, C), REG_THREADS, bytes, stream>>>(T, k, B0, C, scale, dT, workspace);
  PC_HIP_CHECK_LAUNCH("tnet_mse_reg");
  k_mse_reg_finish<<<dim3(1), 64, 0, stream>>>(workspace, k, B0, C, loss);
  PC_HIP_CHECK_LAUNCH("tnet_mse_reg (finish)");
  return PCADV_OK;
}

}  // extern "C"
