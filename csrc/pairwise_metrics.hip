// Pairwise-distance metrics beyond the L1 family: a register-tiled unexpanded
// contraction (KL divergence, Jensen-Shannon, Bray-Curtis), an elementwise
// Haversine kernel, and the fused expanded-form epilogue (Hellinger,
// Russel-Rao, Jaccard, Dice) over a GEMM result.
//
// Reference parity (WHAT): RAFT's historical distance enum — KLDivergence,
// JensenShannon, BrayCurtis, Haversine as unexpanded accumulations;
// HellingerExpanded, RusselRaoExpanded, JaccardExpanded, DiceExpanded as
// epilogues over the inner-product GEMM.
//
// MI355X design (HOW): a 256-thread block owns a 64x64 output tile and every
// thread a 4x4 micro-tile. Both operand panels are staged through LDS in
// K-chunks of 16 in a k-major layout panel[k][row], so ONE 16-byte LDS read
// per operand per k feeds 16 accumulates (the 32x32 kernel in pairwise.hip
// does one 4-byte read per accumulate).
//
// LDS layout: panel[k][LD] with LD = 64 + 4 floats (row padded by one
// 16-byte access width).
//   * reads (ds_read_b128, serviced in 16-lane groups, 64 banks): a thread
//     reads x rows [4*ty, 4*ty+4) and y rows [4*tx, 4*tx+4) of one k-row,
//     tx = tid % 16, ty = tid / 16. Every 16-lane group holds all 16 tx
//     values once -> 16 distinct contiguous 16-byte slots = 64 banks, no
//     conflict; the x read has at most two distinct addresses per group,
//     16 bytes apart (the rest broadcast).
//   * writes (ds_write_b128, 8-lane contiguous groups, 32 banks): a thread
//     stages 4 rows of ONE k (kk = tid % 16) as a float4 at panel[kk][4*rg].
//     Within a group kk = 0..7, same rg: dword offset 68*kk + 4*rg -> bank
//     (4*kk + 4*rg) % 32, eight distinct 4-bank slots. With LD = 64 all eight
//     would land on one slot (8-way); the pad removes it.
// Global loads keep lanes along k (16 lanes x 4 B contiguous per row) and are
// issued for chunk c+1 before the accumulate loop of chunk c.
//
// Per-element transcendental work is done at staging time, never per pair,
// where the formula allows it (see the per-metric notes below). Out-of-range
// rows and the K tail are zero-filled, and every metric is arranged so that
// a zero-filled element contributes exactly 0.

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

namespace {

constexpr int kTile = 64;   // output tile edge
constexpr int kTK = 16;     // K-chunk
constexpr int kLD = kTile + 4;  // padded k-row (floats), keeps 16-B alignment

constexpr int kCodeKL = 5;
constexpr int kCodeJS = 6;
constexpr int kCodeBrayCurtis = 7;
constexpr int kCodeHaversine = 8;

// log(1e-300): the reference clamps y at 1e-300 in fp64; fp32 cannot hold
// that, so y <= 0 maps straight to its log.
constexpr float kLogTiny = -690.77552789821f;
constexpr float kLn2 = 0.69314718055994531f;

// KL divergence  sum_k x (log x - L(y)),  term 0 where x <= 0.
//   staged x side: panel0 = xv = max(x, 0), panel1 = xv * log(xv) (0 at 0)
//   staged y side: panel0 = L(y) = y > 0 ? log y : log(1e-300)
//   inner loop: acc += xv * L(y) — one FMA per pair-element; the pair-
//   independent sum_k x log x rides along as 4 extra adds per k per thread.
//   Precise logf at staging (m+n logs per k, not m*n). Zero fill: xv = 0,
//   x log x = 0, L = finite -> contributes 0.
//
// Jensen-Shannon  sqrt(max(0.5 * sum_k [a log(a/m) + b log(b/m)], 0)),
//   a = max(x,0), b = max(y,0), m = (a+b)/2.
//   The "log m" form is used: a log(a/m) + b log(b/m)
//     = (a log a + b log b) - (a + b) log m,
//   with A = a log2 a and B = b log2 b staged per element, so the inner loop
//   has ONE log (v_log_f32 on m) per pair-element; ln 2 is applied once in
//   the epilogue. This form is chosen over a*log(a/m) because its d(x,x) is
//   EXACTLY 0: with a == b, m == a bit-for-bit, the staged and the inner log
//   are the same instruction on the same input, (a+b)*log2(m) = 2*fl(a log2 a)
//   and A + B = 2*fl(a log2 a) — both exact power-of-two scalings (the
//   product is kept un-fused for this reason). The x*log(x/m) form needs a
//   division and leaves a rounding residue on the diagonal.
//   Elements below FLT_MIN are treated as 0 on both sides (v_log_f32 does
//   not take denormals; their contribution is < 1e-35). Zero fill: A = B = 0,
//   m = 0 -> log skipped -> contributes 0.
//
// Bray-Curtis  sum|x-y| / sum|x+y|, 0 where the denominator is 0: two
//   accumulators per output, no transform. Zero fill contributes 0 to both.

template <int CODE>
struct Panels {
  static constexpr int NX = (CODE == kCodeBrayCurtis) ? 1 : 2;
  static constexpr int NY = (CODE == kCodeJS) ? 2 : 1;
  static constexpr int NACC = (CODE == kCodeBrayCurtis) ? 2 : 1;
};

__device__ __forceinline__ float js_xlog2x(float a) {
  return a >= FLT_MIN ? a * __log2f(a) : 0.f;
}

// transform 4 raw x values (same k, 4 consecutive rows) into the staged panels
template <int CODE>
__device__ __forceinline__ void stage_x(const float (&r)[4], float4 (&p)[2]) {
  float a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (CODE == kCodeKL) {
      a[i] = r[i] > 0.f ? r[i] : 0.f;
      b[i] = r[i] > 0.f ? r[i] * logf(r[i]) : 0.f;
    } else if constexpr (CODE == kCodeJS) {
      a[i] = r[i] >= FLT_MIN ? r[i] : 0.f;
      b[i] = js_xlog2x(r[i]);
    } else {
      a[i] = r[i];
      b[i] = 0.f;
    }
  }
  p[0] = make_float4(a[0], a[1], a[2], a[3]);
  p[1] = make_float4(b[0], b[1], b[2], b[3]);
}

template <int CODE>
__device__ __forceinline__ void stage_y(const float (&r)[4], float4 (&p)[2]) {
  float a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (CODE == kCodeKL) {
      a[i] = r[i] > 0.f ? logf(r[i]) : kLogTiny;
      b[i] = 0.f;
    } else if constexpr (CODE == kCodeJS) {
      a[i] = r[i] >= FLT_MIN ? r[i] : 0.f;
      b[i] = js_xlog2x(r[i]);
    } else {
      a[i] = r[i];
      b[i] = 0.f;
    }
  }
  p[0] = make_float4(a[0], a[1], a[2], a[3]);
  p[1] = make_float4(b[0], b[1], b[2], b[3]);
}

__device__ __forceinline__ float f4_get(const float4& v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

template <int CODE>
__global__ __launch_bounds__(256) void pairwise_tiled_kernel(
    const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
    long long m, long long n, long long d, long long tiles_n) {
  using P = Panels<CODE>;
  __shared__ __align__(16) float xs[P::NX][kTK][kLD];
  __shared__ __align__(16) float ys[P::NY][kTK][kLD];

  const long long bid = blockIdx.x;
  const long long bi = (bid / tiles_n) * kTile;  // x-row base
  const long long bj = (bid % tiles_n) * kTile;  // y-row base
  const int tx = threadIdx.x % 16;  // output cols 4*tx .. 4*tx+3
  const int ty = threadIdx.x / 16;  // output rows 4*ty .. 4*ty+3
  // staging role: one k (kk), four consecutive panel rows (4*rg ..)
  const int kk = threadIdx.x % kTK;
  const int rg = threadIdx.x / kTK;

  float acc[P::NACC][4][4];
  float rowterm[4] = {0.f, 0.f, 0.f, 0.f};  // KL: sum_k x log x
#pragma unroll
  for (int a = 0; a < P::NACC; a++)
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[a][r][c] = 0.f;

  float xr[4], yr[4];
  auto load_chunk = [&](long long k0) {
    const long long k = k0 + kk;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const long long gi = bi + rg * 4 + r;
      const long long gj = bj + rg * 4 + r;
      xr[r] = (gi < m && k < d) ? x[gi * d + k] : 0.f;
      yr[r] = (gj < n && k < d) ? y[gj * d + k] : 0.f;
    }
  };

  load_chunk(0);
  for (long long k0 = 0; k0 < d; k0 += kTK) {
    float4 px[2], py[2];
    stage_x<CODE>(xr, px);
    stage_y<CODE>(yr, py);
#pragma unroll
    for (int p = 0; p < P::NX; p++)
      *reinterpret_cast<float4*>(&xs[p][kk][rg * 4]) = px[p];
#pragma unroll
    for (int p = 0; p < P::NY; p++)
      *reinterpret_cast<float4*>(&ys[p][kk][rg * 4]) = py[p];
    __syncthreads();
    if (k0 + kTK < d) load_chunk(k0 + kTK);  // in flight during the accumulate

    // partial unroll: full unrolling hoists every LDS read of the chunk and
    // costs 200+ VGPRs (1-2 waves/SIMD); 4 keeps the kernels at <= 128
#pragma unroll 4
    for (int k = 0; k < kTK; k++) {
      const float4 xa = *reinterpret_cast<const float4*>(&xs[0][k][ty * 4]);
      const float4 ya = *reinterpret_cast<const float4*>(&ys[0][k][tx * 4]);
      if constexpr (CODE == kCodeKL) {
        const float4 xl = *reinterpret_cast<const float4*>(&xs[1][k][ty * 4]);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          rowterm[r] += f4_get(xl, r);
#pragma unroll
          for (int c = 0; c < 4; c++)
            acc[0][r][c] = fmaf(f4_get(xa, r), f4_get(ya, c), acc[0][r][c]);
        }
      } else if constexpr (CODE == kCodeJS) {
        const float4 xA = *reinterpret_cast<const float4*>(&xs[1][k][ty * 4]);
        const float4 yB = *reinterpret_cast<const float4*>(&ys[1][k][tx * 4]);
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
          for (int c = 0; c < 4; c++) {
            // product kept un-fused: d(x,x) is exactly 0 only if s * lm is
            // rounded before the subtraction (see above)
#pragma clang fp contract(off)
            const float s = f4_get(xa, r) + f4_get(ya, c);
            const float mm = 0.5f * s;
            const float lm = mm >= FLT_MIN ? __log2f(mm) : 0.f;
            const float prod = s * lm;
            const float t = (f4_get(xA, r) + f4_get(yB, c)) - prod;
            acc[0][r][c] += t;
          }
        }
      } else {  // Bray-Curtis
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
          for (int c = 0; c < 4; c++) {
            acc[0][r][c] += fabsf(f4_get(xa, r) - f4_get(ya, c));
            acc[P::NACC - 1][r][c] += fabsf(f4_get(xa, r) + f4_get(ya, c));
          }
        }
      }
    }
    __syncthreads();
  }

  // epilogue + store (16-byte stores when the row is aligned and in range)
  const long long gj0 = bj + tx * 4;
  const bool vec_ok = (n % 4 == 0) && (gj0 + 3 < n) &&
                      ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const long long gi = bi + ty * 4 + r;
    if (gi >= m) continue;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if constexpr (CODE == kCodeKL) {
        v[c] = rowterm[r] - acc[0][r][c];
      } else if constexpr (CODE == kCodeJS) {
        v[c] = sqrtf(fmaxf(0.5f * kLn2 * acc[0][r][c], 0.f));
      } else {
        const float den = acc[P::NACC - 1][r][c];
        v[c] = den > 0.f ? acc[0][r][c] / den : 0.f;
      }
    }
    float* op = out + gi * n + gj0;
    if (vec_ok) {
      *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (gj0 + c < n) op[c] = v[c];
    }
  }
}

// Haversine: rows are [lat, lon] in radians (d == 2) — no K loop, one output
// per thread, coalesced along j.
__global__ void haversine_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                 float* __restrict__ out, long long m, long long n) {
  const long long total = m * n;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const long long i = t / n;
    const long long j = t - i * n;
    const float lat1 = x[2 * i], lon1 = x[2 * i + 1];
    const float lat2 = y[2 * j], lon2 = y[2 * j + 1];
    const float sl = sinf(0.5f * (lat1 - lat2));
    const float so = sinf(0.5f * (lon1 - lon2));
    float h = sl * sl + cosf(lat1) * cosf(lat2) * so * so;
    h = fminf(fmaxf(h, 0.f), 1.f);
    out[t] = 2.f * asinf(sqrtf(h));
  }
}

template <int CODE>
void launch_tiled(const float* x, const float* y, float* out, long long m, long long n,
                  long long d, hipStream_t stream) {
  const long long tiles_m = (m + kTile - 1) / kTile;
  const long long tiles_n = (n + kTile - 1) / kTile;
  const long long blocks = tiles_m * tiles_n;
  if (blocks > (long long)INT_MAX)
    throw std::runtime_error("pairwise metrics: output too large for one launch");
  hipLaunchKernelGGL((pairwise_tiled_kernel<CODE>), dim3((unsigned)blocks), dim3(256), 0,
                     stream, x, y, out, m, n, d, tiles_n);
}

}  // namespace

// codes 5..8 of launch_pairwise_unexpanded (DistanceCode) land here
void launch_pairwise_metrics(const float* x, const float* y, float* out, long long m,
                             long long n, long long d, int code, hipStream_t stream) {
  if (d < 1) throw std::runtime_error("pairwise metrics: d must be >= 1");
  if (m <= 0 || n <= 0) return;
  switch (code) {
    case kCodeKL: launch_tiled<kCodeKL>(x, y, out, m, n, d, stream); break;
    case kCodeJS: launch_tiled<kCodeJS>(x, y, out, m, n, d, stream); break;
    case kCodeBrayCurtis: launch_tiled<kCodeBrayCurtis>(x, y, out, m, n, d, stream); break;
    case kCodeHaversine: {
      if (d != 2) throw std::runtime_error("haversine needs d == 2 ([lat, lon] rows)");
      const int grid = grid_1d(m * n, 256);
      hipLaunchKernelGGL(haversine_kernel, dim3(grid), dim3(256), 0, stream, x, y, out, m, n);
      break;
    }
    default: throw std::runtime_error("bad pairwise code");
  }
}

// --------------------------------------------------------------------------
// in-place fused expanded-form epilogue over a GEMM result g[m,n] = <x_i,y_j>
// codes (ExpandedDistanceCode): 0 = Hellinger   sqrt(max(1 - g, 0))
//                               1 = Russel-Rao  (d - g) / d
//                               2 = Jaccard     1 - g / (xa + ya - g)
//                               3 = Dice        1 - 2 g / (xa + ya)
// (Jaccard/Dice: 0 where the denominator is 0). xa/ya are the squared row
// norms and are read by codes 2 and 3 only. g is streamed as ONE flat
// [m*n] array in float4 groups (a group may straddle a row end, so any n
// keeps the 16-byte alignment of the base pointer) plus a ragged tail.
// --------------------------------------------------------------------------
template <int CODE>
__device__ __forceinline__ float expanded_op(float g, float xa, float ya, float d) {
  if constexpr (CODE == 0) return sqrtf(fmaxf(1.f - g, 0.f));
  if constexpr (CODE == 1) return (d - g) / d;
  if constexpr (CODE == 2) {
    const float den = xa + ya - g;
    return den != 0.f ? 1.f - g / den : 0.f;
  }
  const float den = xa + ya;
  return den != 0.f ? 1.f - 2.f * g / den : 0.f;
}

template <int CODE>
__global__ void expanded_epilogue_kernel(float* __restrict__ g, const float* __restrict__ xa,
                                         const float* __restrict__ ya, long long m,
                                         long long n, float d) {
  constexpr bool kNorms = (CODE >= 2);
  const long long total = m * n;
  const long long total4 = total / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long t = t0; t < total4; t += stride) {
    float4* gp = reinterpret_cast<float4*>(g) + t;
    float4 v = *gp;
    long long i = (t * 4) / n;
    long long j = (t * 4) - i * n;
    float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float xv = kNorms ? xa[i] : 0.f;
      const float yv = kNorms ? ya[j] : 0.f;
      r[e] = expanded_op<CODE>(r[e], xv, yv, d);
      if (++j == n) { j = 0; i++; }
    }
    *gp = make_float4(r[0], r[1], r[2], r[3]);
  }
  // ragged tail (total % 4 elements)
  for (long long e = total4 * 4 + t0; e < total; e += stride) {
    const long long i = e / n;
    const long long j = e - i * n;
    g[e] = expanded_op<CODE>(g[e], kNorms ? xa[i] : 0.f, kNorms ? ya[j] : 0.f, d);
  }
}

void launch_pairwise_expanded_epilogue(float* g, const float* xa, const float* ya,
                                       long long m, long long n, int code, float d,
                                       hipStream_t stream) {
  if (m <= 0 || n <= 0) return;
  if ((code == 2 || code == 3) && (xa == nullptr || ya == nullptr))
    throw std::runtime_error("expanded epilogue: Jaccard/Dice need the row norms");
  const int grid = grid_1d((m * n + 3) / 4, 256);
  const dim3 gd(grid), bd(256);
  switch (code) {
    case 0: hipLaunchKernelGGL((expanded_epilogue_kernel<0>), gd, bd, 0, stream, g, xa, ya, m, n, d); break;
    case 1: hipLaunchKernelGGL((expanded_epilogue_kernel<1>), gd, bd, 0, stream, g, xa, ya, m, n, d); break;
    case 2: hipLaunchKernelGGL((expanded_epilogue_kernel<2>), gd, bd, 0, stream, g, xa, ya, m, n, d); break;
    case 3: hipLaunchKernelGGL((expanded_epilogue_kernel<3>), gd, bd, 0, stream, g, xa, ya, m, n, d); break;
    default: throw std::runtime_error("bad expanded-epilogue code");
  }
}

}  // namespace raft_amd
