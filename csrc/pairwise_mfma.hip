// Pairwise L2-expanded distance tile kernel — split-bf16 MFMA with the
// epilogue fused into the C-write (BASELINE config 2's engine).
//
// Reference parity (WHAT): RAFT's historical pairwise-distance L2-expanded
// epilogue over the contraction engine. Versus the rocBLAS 3/6-GEMM
// beta-accumulate path, this writes the fp32 distance tile EXACTLY ONCE
// (d2 = xn + yn - 2 x.c computed in registers from the accumulator), cutting
// the dominant HBM cost of large distance matrices by ~5x
// (3-GEMM path: 3 writes + 2 reads + epilogue read/write = 7 tile passes).
//
// Same geometry/staging as fused_l2nn.hip (see mfma_common.h). Two families,
// tile writers and threshold filters, each in a 128^2 and a 256^2 geometry;
// pairwise_variant.h names the variants and resolves which one runs.

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "mfma_common.h"
#include "pairwise_variant.h"

namespace raft_amd {

// ---------------------------------------------------------------------------
// epilogues shared by the 128^2 (FR = 4) and 256^2 (FR = 8) kernels.
// C/D layout: col = lane&15 (+fc*16), row = (lane>>4)*4 + reg (+fr*16); a
// wave owns FR*16 rows x 64 columns.
// ---------------------------------------------------------------------------

// ragged-edge tile write: d2 = max(xn[r] + yn[c] - 2 acc, 0), one guarded
// scalar store per element. NT: non-temporal stores (streaming output, never
// re-read — keeps the L2 clear for the operand tiles).
template <int FR, bool NT>
__device__ __forceinline__ void pw_write_ragged(
    const f32x4 (&acc)[FR][4], const MfmaTile& t, const float* __restrict__ xn,
    const float* __restrict__ yn, float* __restrict__ out, long long m, long long n,
    long long ldo, bool do_sqrt) {
#pragma unroll
  for (int fr = 0; fr < FR; fr++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const long long row =
          t.row0 + t.wr * (FR * 16) + fr * 16 + (t.lane >> 4) * 4 + reg;
      if (row >= m) continue;
      const float xv = xn[row];
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
        const long long col = t.col0 + t.wc * 64 + fc * 16 + (t.lane & 15);
        if (col < n) {
          float v = fmaxf(xv + yn[col] - 2.f * acc[fr][fc][reg], 0.f);
          if (do_sqrt) v = sqrtf(v);
          if constexpr (NT)
            __builtin_nontemporal_store(v, &out[row * ldo + col]);
          else
            out[row * ldo + col] = v;
        }
      }
    }
  }
}

// interior tile write ((ldo & 3) == 0): stage 128 rows at a time through
// padded LDS ([128][TILE + 4] fp32 at `tile`, which the dead K-loop LDS
// provides) and dump them as coalesced dwordx4 rows. The direct path issues
// FR*16 scalar 4 B stores/thread each with 64-bit row*ldo address math —
// measured 12:1 VALU:MFMA, epilogue-dominated (418 Gdist/s vs the ~1.6
// Tdist/s write roofline). nt: non-temporal vs cached stores (A/B:
// write-combine behavior differs).
template <int FR>
__device__ __forceinline__ void pw_write_staged(
    const f32x4 (&acc)[FR][4], const MfmaTile& t, float* tile,
    const float* __restrict__ xn, const float* __restrict__ yn,
    float* __restrict__ out, long long ldo, bool do_sqrt, bool nt) {
  constexpr int TILE = FR * 32, LD = TILE + 4;
  constexpr int WAVE_ROWS = 8 / FR;  // wave rows per 128-row half: 2 or 1
  // a round of the dump writes 8 rows: TILE/4 threads x float4 per row
  const int tr = threadIdx.x / (TILE / 4);
  const int tc = (threadIdx.x % (TILE / 4)) * 4;
  float yn_r[4];
#pragma unroll
  for (int fc = 0; fc < 4; fc++)
    yn_r[fc] = yn[t.col0 + t.wc * 64 + fc * 16 + (t.lane & 15)];
#pragma unroll
  for (int half = 0; half < TILE / 128; half++) {
    __syncthreads();  // the K-loop, or the previous half's dump, is done
    if (TILE == 128 || t.wr / WAVE_ROWS == half) {
#pragma unroll
      for (int fr = 0; fr < FR; fr++) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int rl =
              (t.wr % WAVE_ROWS) * (FR * 16) + fr * 16 + (t.lane >> 4) * 4 + reg;
          const float xv = xn[t.row0 + half * 128 + rl];
#pragma unroll
          for (int fc = 0; fc < 4; fc++) {
            const int cl = t.wc * 64 + fc * 16 + (t.lane & 15);
            float v = fmaxf(xv + yn_r[fc] - 2.f * acc[fr][fc][reg], 0.f);
            if (do_sqrt) v = sqrtf(v);
            tile[rl * LD + cl] = v;
          }
        }
      }
    }
    __syncthreads();
    const float* src = tile + tr * LD + tc;
    float* dst = out + (t.row0 + half * 128 + tr) * ldo + t.col0 + tc;
    const long long dstep = 8 * ldo;
#pragma unroll
    for (int rnd = 0; rnd < 16; rnd++) {
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(src + rnd * 8 * LD);
      f32x4* dp = reinterpret_cast<f32x4*>(dst + rnd * dstep);
      if (nt)
        __builtin_nontemporal_store(v4, dp);
      else
        *dp = v4;
    }
  }
}

// filtered top-k emission: instead of writing the tile, emit only candidates
// with d2 <= thr[row] into per-row bounded buffers (the sample -> threshold ->
// filter kNN scheme: the m x n distance tile never touches HBM; expected
// emissions ~ O(k) per row).
//
// Epilogue VALU diet (same recipe as the l2nn 2d kernel, measured there via
// profiles/pmc_l2nn_x1v_gt8.txt): yn[col] and the col<n guard depend only on
// fc — hoisted to 4 registers (out-of-range columns carry +inf, so they can
// never pass the threshold); the fmax moves into the rare admitted-candidate
// store, with thr clamped to >= 0 once per row so the unclamped compare
// admits the same set.
template <int FR>
__device__ __forceinline__ void pw_filter_epilogue(
    const f32x4 (&acc)[FR][4], const MfmaTile& t, const float* __restrict__ xn,
    const float* __restrict__ yn, const float* __restrict__ thr,
    float* __restrict__ out_d, int* __restrict__ out_i, int* __restrict__ cnt,
    int cap, long long col_offset, long long m, long long n) {
  const long long colb = t.col0 + t.wc * 64 + (t.lane & 15);
  float yn_r[4];
#pragma unroll
  for (int fc = 0; fc < 4; fc++) {
    const long long col = colb + fc * 16;
    yn_r[fc] = col < n ? yn[col] : INFINITY;
  }
#pragma unroll
  for (int fr = 0; fr < FR; fr++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const long long row =
          t.row0 + t.wr * (FR * 16) + fr * 16 + (t.lane >> 4) * 4 + reg;
      if (row >= m) continue;
      const float xv = xn[row];
      const float tv = fmaxf(thr[row], 0.f);
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
        const float s = xv + yn_r[fc] - 2.f * acc[fr][fc][reg];
        if (s <= tv) {
          const int pos = atomicAdd(&cnt[row], 1);
          if (pos < cap) {
            out_d[row * cap + pos] = fmaxf(s, 0.f);
            out_i[row * cap + pos] = (int)(colb + fc * 16 + col_offset);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 128x128 tile: 256 threads (4 waves, 2x2 grid), 2 blocks/CU
// ---------------------------------------------------------------------------

template <int NSLICE, bool BK32 = false>
__launch_bounds__(256, 2)
__global__ void pairwise_l2_kernel(const SlicePtrs p,
                                   const float* __restrict__ xn,
                                   const float* __restrict__ yn,
                                   float* __restrict__ out,
                                   long long m, long long n, int d,
                                   long long ldo, int sqrt_out, int rg) {
  extern __shared__ __bf16 smem[];
  MfmaTile t;
  f32x4 acc[4][4];
  if (!mfma_tile_prologue<128>(rg, m, n, t, acc)) return;

  if constexpr (BK32 && NSLICE <= 2) {
    // counted-vmcnt BK=32 dbuf K-loop at 2 blocks/CU: no full drains AND
    // cross-block overlap (variant "128_bk32")
    mfma256_bk32_kloop<NSLICE, 128>(p, smem, acc, t, m, n, d);
  } else {
    mfma_tile_kloop<NSLICE>(p, smem, acc, t, m, n, d);
  }

  if (t.row0 + 128 <= m && t.col0 + 128 <= n && (ldo & 3) == 0) {
    // [128][132] fp32, 67.5 KiB: fits 2 blocks/CU
    pw_write_staged<4>(acc, t, reinterpret_cast<float*>(smem), xn, yn, out, ldo,
                       sqrt_out != 0, true);
    return;
  }
  pw_write_ragged<4, false>(acc, t, xn, yn, out, m, n, ldo, sqrt_out != 0);
}

template <int NSLICE>
__launch_bounds__(256, 2)
__global__ void pairwise_l2_filter_kernel(const SlicePtrs p,
                                          const float* __restrict__ xn,
                                          const float* __restrict__ yn,
                                          const float* __restrict__ thr,
                                          float* __restrict__ out_d,
                                          int* __restrict__ out_i,
                                          int* __restrict__ cnt, int cap,
                                          long long col_offset, long long m,
                                          long long n, int d, int rg) {
  extern __shared__ __bf16 smem[];
  MfmaTile t;
  f32x4 acc[4][4];
  if (!mfma_tile_prologue<128>(rg, m, n, t, acc)) return;
  mfma_tile_kloop<NSLICE>(p, smem, acc, t, m, n, d);
  pw_filter_epilogue<4>(acc, t, xn, yn, thr, out_d, out_i, cnt, cap, col_offset, m, n);
}

// ---------------------------------------------------------------------------
// Persistent-X filter (bf16 index, d <= 128): the X row panel (full depth,
// <= 32 KiB) stages ONCE per block and stays LDS-resident while the block
// walks CT col-tiles, double-buffering ONLY the 16 KiB C chunks with counted
// vmcnt (flight depth 1 chunk, no full drains). Halves the gloads per
// K-step and removes the X re-stage entirely; 64 KiB LDS keeps 2 blocks/CU
// (the l2nn persistent-X experiment lost to occupancy at 1 block/CU — this
// configuration keeps both the residency AND the 2-block overlap).
// Block decode groups same-col-group blocks on one XCD so the C panels are
// the L2-shared working set.
// ---------------------------------------------------------------------------
template <int CT = 8>
__launch_bounds__(256, 2)
__global__ void pairwise_l2_filter_px_kernel(
    const __bf16* __restrict__ x0g, const __bf16* __restrict__ c0g,
    const float* __restrict__ xn, const float* __restrict__ yn,
    const float* __restrict__ thr, float* __restrict__ out_d,
    int* __restrict__ out_i, int* __restrict__ cnt, int cap,
    long long col_offset, long long m, long long n, int d, int n_row_tiles) {
  extern __shared__ __bf16 smem[];
  const int kts = d / 64;

  // bijective XCD-contiguous remap, COLUMN-group-major (blocks sharing a C
  // group land on one XCD)
  const int t = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const long long row0 = (long long)(t % n_row_tiles) * 128;
  const int ctg = t / n_row_tiles;
  const long long col_base = (long long)ctg * CT * 128;
  if (row0 >= m || col_base >= n) return;
  const int nct = (int)((n - col_base + 127) / 128) < CT
                      ? (int)((n - col_base + 127) / 128)
                      : CT;

  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = threadIdx.x / RAFT_AMD_WAVE;
  const int wr = w >> 1, wc = w & 1;

  // stage the X panel once: kts chunks of [128][64] at kt*8192 elements
  for (int kt = 0; kt < kts; kt++)
    mfma_stage_tile128(x0g, smem + kt * 8192, row0, (long long)kt * 64, d,
                       m - 1);
  __bf16* cb0 = smem + kts * 8192;   // two 16 KiB C chunk buffers
  __bf16* cb1 = cb0 + 8192;
  const int total = nct * kts;
  auto stage_c = [&](int s, __bf16* buf) {
    const long long c0 = col_base + (long long)(s / kts) * 128;
    mfma_stage_tile128(c0g, buf, c0, (long long)(s % kts) * 64, d, n - 1);
  };
  stage_c(0, cb0);
  if (total > 1) stage_c(1, cb1);
  // X (4*kts gloads) + chunk 0 must land; chunk 1 stays in flight
  if (total > 1) {
    asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < total; s++) {
    const int kt = s % kts;
    __bf16* cbuf = (s & 1) ? cb1 : cb0;
    const __bf16* xchunk = smem + kt * 8192;
    // ALL fragments for this chunk first (a/b for both kf), then a barrier
    // confirming every wave's reads are done, THEN the refill of this
    // buffer with chunk s+2 — a mid-read refill races other waves' ds_reads
    bf16x8 a_frag[2][4], b_frag[2][4];
#pragma unroll
    for (int kf = 0; kf < 2; kf++) {
      const int kbyte = (kf * 32 + (lane >> 4) * 8) * 2;
#pragma unroll
      for (int fr = 0; fr < 4; fr++) {
        const int rr = wr * 64 + fr * 16 + (lane & 15);
        a_frag[kf][fr] = *reinterpret_cast<const bf16x8*>(
            (const char*)xchunk + mfma_swz(rr * 128 + kbyte));
      }
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
        const int cc = wc * 64 + fc * 16 + (lane & 15);
        b_frag[kf][fc] = *reinterpret_cast<const bf16x8*>(
            (const char*)cbuf + mfma_swz(cc * 128 + kbyte));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (s + 2 < total) stage_c(s + 2, cbuf);
#pragma unroll
    for (int kf = 0; kf < 2; kf++)
#pragma unroll
      for (int fr = 0; fr < 4; fr++)
#pragma unroll
        for (int fc = 0; fc < 4; fc++)
          acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[kf][fr], b_frag[kf][fc], acc[fr][fc], 0, 0, 0);
    if (kt == kts - 1) {
      // filter epilogue for this col tile (registers + global atomics only)
      const MfmaTile tile{row0, col_base + (long long)(s / kts) * 128, lane, wr, wc};
      pw_filter_epilogue<4>(acc, tile, xn, yn, thr, out_d, out_i, cnt, cap,
                            col_offset, m, n);
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // chunk s+1 must have landed before the next iteration reads it (leave
    // the 4 loads issued for s+2 in flight)
    if (s + 2 < total) {
      asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
  }
}

// ---------------------------------------------------------------------------
// 256x256 tile: 512 threads (8 waves, 2x4 grid; per-wave 128x64 fragment
// tile) over the BK=32 product-phase counted-vmcnt K-loop (mfma_common.h),
// 1 or 2 slices. Quarters the workgroup count of the 128x128 kernel — at
// small d (e.g. 128: only 2 K-steps) the per-workgroup prologue/epilogue is a
// first-order cost. The K-loop's old per-K-step `vmcnt(0)+barrier` full drain
// ran at 1 block/CU with nothing to hide it.
// ---------------------------------------------------------------------------

template <int NSLICE>
__launch_bounds__(512, 1)
__global__ void pairwise_l2_256_kernel(const SlicePtrs p,
                                       const float* __restrict__ xn,
                                       const float* __restrict__ yn,
                                       float* __restrict__ out,
                                       long long m, long long n, int d,
                                       long long ldo, int sqrt_out, int rg) {
  extern __shared__ __bf16 smem[];
  MfmaTile t;
  f32x4 acc[8][4];
  if (!mfma_tile_prologue<256>(rg, m, n, t, acc)) return;
  mfma256_bk32_kloop<NSLICE, 256>(p, smem, acc, t, m, n, d);

  const bool do_sqrt = (sqrt_out & 1) != 0;
  if (t.row0 + 256 <= m && t.col0 + 256 <= n && (ldo & 3) == 0) {
    // two halves through [128][260] fp32 (130 KiB); sqrt_out bit 1 selects
    // non-temporal stores
    pw_write_staged<8>(acc, t, reinterpret_cast<float*>(smem), xn, yn, out, ldo,
                       do_sqrt, (sqrt_out & 2) != 0);
    return;
  }
  pw_write_ragged<8, true>(acc, t, xn, yn, out, m, n, ldo, do_sqrt);
}

// this kernel has no tile writes, so the K-loop IS the kernel
template <int NSLICE>
__launch_bounds__(512, 2)
__global__ void pairwise_l2_filter256_kernel(const SlicePtrs p,
                                             const float* __restrict__ xn,
                                             const float* __restrict__ yn,
                                             const float* __restrict__ thr,
                                             float* __restrict__ out_d,
                                             int* __restrict__ out_i,
                                             int* __restrict__ cnt, int cap,
                                             long long col_offset, long long m,
                                             long long n, int d, int rg) {
  extern __shared__ __bf16 smem[];
  MfmaTile t;
  f32x4 acc[8][4];
  if (!mfma_tile_prologue<256>(rg, m, n, t, acc)) return;
  mfma256_bk32_kloop<NSLICE, 256>(p, smem, acc, t, m, n, d);
  pw_filter_epilogue<8>(acc, t, xn, yn, thr, out_d, out_i, cnt, cap, col_offset, m, n);
}

// ---------------------------------------------------------------------------
// variant selection (pairwise_variant.h)
// ---------------------------------------------------------------------------

namespace {

// A/B tuning switches, read once per process (docs/developer_guide.md)
struct PwEnv {
  bool pw256, bk32;       // Tile: variant overrides of "auto"
  bool filter256, px;     // Filter: variant overrides of "auto"
  bool rowmajor, nt;      // modifiers, environment-only
};

const PwEnv& pw_env() {
  static const PwEnv env = [] {
    auto on = [](const char* name) {
      const char* e = getenv(name);
      return e && e[0] == '1';
    };
    PwEnv v;
    // 256^2 writer: 4x fewer workgroups, but 1 block/CU serializes the
    // tile-store phase with the K-loop — measured 547 vs the 128^2 kernel's
    // 736 Gdist/s at 1Mx128 (round 2)
    v.pw256 = on("RAFT_AMD_PW256");
    v.bk32 = on("RAFT_AMD_PW_BK32");
    // A/B @100M-row kNN: 128-tile 9006 q/s vs 256-tile 7226 — the 4-wave
    // 2-block filter wins (same pattern as the fused L2-NN A/B)
    v.filter256 = on("RAFT_AMD_FILTER256");
    // persistent-X: 7.5k vs 9.9k q/s at the 100M headline — the 1-chunk
    // flight depth can't hide HBM latency in the streaming regime and the
    // per-chunk lockstep loses to the independent full-drain blocks
    v.px = on("RAFT_AMD_KNN_PX");
    // the 128^2 writer walks the 8x8 super-tile column-major (adjacent output
    // segments written by temporally adjacent blocks — DRAM page locality);
    // RAFT_AMD_PW_RM=1 restores row-major
    v.rowmajor = on("RAFT_AMD_PW_RM");
    // 256^2 writer interior stores: default cached (write-combining via L2)
    v.nt = on("RAFT_AMD_PW_NT");
    return v;
  }();
  return env;
}

constexpr const char* kVariantNames[] = {"auto", "128", "128_bk32", "256", "px"};

// the condition `v` violates on this shape, or nullptr
const char* pw_variant_violation(PwVariant v, int nslice, long long n, int d) {
  switch (v) {
    case PwVariant::T128Bk32:
    case PwVariant::T256:
      if (nslice > 2) return "nslice must be 1 or 2 (BK=32 K-loop)";
      return nullptr;
    case PwVariant::Px:
      if (nslice != 1) return "nslice must be 1";
      if (d % 64 != 0 || d > 128) return "d must be 64 or 128 (X stays in LDS)";
      if (n < 1024) return "n must be at least 1024";
      return nullptr;
    default:
      return nullptr;
  }
}

// the 128^2 writer the environment picks (RAFT_AMD_PW_BK32 silently does not
// apply at three slices)
PwVariant pw_auto_128(int nslice, int d) {
  return pw_env().bk32 && nslice <= 2 && d % 32 == 0 ? PwVariant::T128Bk32
                                                     : PwVariant::T128;
}

// what the environment and the measured defaults pick: the 128^2 kernels
// unless a variable asks for a losing variant where auto's heuristic lets it
PwVariant pw_auto_variant(PwFamily family, int nslice, long long m, long long n, int d) {
  const PwEnv& env = pw_env();
  const bool big = nslice <= 2 && m >= 512 && n >= 512;
  if (family == PwFamily::Tile)
    return env.pw256 && big ? PwVariant::T256 : pw_auto_128(nslice, d);
  if (env.filter256 && big) return PwVariant::T256;
  if (env.px && !pw_variant_violation(PwVariant::Px, nslice, n, d)) return PwVariant::Px;
  return PwVariant::T128;
}

// blocks of the 8x8 super-tiled grid of tile x tile tiles, and the rg that
// xcd_supertile_decode takes: rg = ceil(R/8), R = ceil(m/tile)
dim3 supertile_grid(long long m, long long n, int tile, int* rg) {
  *rg = (int)((m + 8 * tile - 1) / (8 * tile));
  const int cg = (int)((n + 8 * tile - 1) / (8 * tile));
  return dim3((unsigned)((long long)*rg * cg * 64));
}

// Launch Kernel with `lds` bytes of dynamic LDS. Above the 64 KiB a kernel
// may use by default, the limit is raised first, once per kernel
// instantiation and size.
template <auto Kernel, typename... Args>
void pw_launch(dim3 grid, int block, size_t lds, hipStream_t stream, Args... args) {
  static size_t lds_limit = 64 * 1024;
  if (lds > lds_limit) {
    HIP_CHECK(hipFuncSetAttribute((const void*)Kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
    lds_limit = lds;
  }
  hipLaunchKernelGGL(Kernel, grid, dim3(block), lds, stream, args...);
}

// f(std::integral_constant<int, nslice>) for nslice in 1..MAX
template <int MAX, typename F>
void pw_for_nslice(int nslice, const char* who, F&& f) {
  if (nslice == 1) return f(std::integral_constant<int, 1>{});
  if (nslice == 2) return f(std::integral_constant<int, 2>{});
  if constexpr (MAX == 3)
    if (nslice == 3) return f(std::integral_constant<int, 3>{});
  throw std::runtime_error(std::string(who) + ": nslice must be 1" +
                           (MAX == 3 ? ", 2 or 3" : " or 2"));
}

}  // namespace

const char* pw_variant_name(PwVariant v) { return kVariantNames[(int)v]; }

PwVariant pw_variant_from_name(PwFamily family, const std::string& name, bool* known) {
  const PwVariant other = family == PwFamily::Tile ? PwVariant::Px : PwVariant::T128Bk32;
  for (int i = 0; i < (int)(sizeof(kVariantNames) / sizeof(kVariantNames[0])); i++)
    if (name == kVariantNames[i] && (PwVariant)i != other) {
      *known = true;
      return (PwVariant)i;
    }
  *known = false;
  return PwVariant::Auto;
}

PwPlan pw_resolve_variant(PwFamily family, int nslice, long long m, long long n, int d,
                          PwVariant requested) {
  if (requested == PwVariant::Auto) return {pw_auto_variant(family, nslice, m, n, d), {}};
  PwPlan plan{requested, {}};
  if (const char* why = pw_variant_violation(requested, nslice, n, d))
    plan.error = std::string(family == PwFamily::Tile ? "pairwise_l2_mfma" : "pairwise_l2_filter") +
                 " variant '" + pw_variant_name(requested) + "': " + why;
  return plan;
}

void launch_pairwise_l2_tile(const PwPlan& plan, const void** xsl, const void** csl,
                             const float* xn, const float* yn, float* out, long long m,
                             long long n, int d, long long ldo, int nslice,
                             bool sqrt_out, hipStream_t stream) {
  if (!plan.error.empty()) throw std::runtime_error(plan.error);
  const SlicePtrs p(xsl, csl, nslice);
  const PwEnv& env = pw_env();
  int rg;
  if (plan.variant == PwVariant::T256) {
    const dim3 grid = supertile_grid(m, n, 256, &rg);
    // K-loop: 8 x 16 KiB BK=32 dbuf regions (128 KiB); epilogue staging:
    // [128][260] fp32 (130 KiB), the larger
    const size_t lds = 128 * 260 * 4;
    const int so_bits = (sqrt_out ? 1 : 0) | (env.nt ? 2 : 0);
    pw_for_nslice<2>(nslice, "pairwise 256^2 kernel", [&](auto ns) {
      pw_launch<pairwise_l2_256_kernel<decltype(ns)::value>>(
          grid, 512, lds, stream, p, xn, yn, out, m, n, d, ldo, so_bits, rg);
    });
    return;
  }
  const dim3 grid = supertile_grid(m, n, 128, &rg);
  if (!env.rowmajor) rg = -rg;  // rg < 0: column-major slot order
  const size_t lds_k = (size_t)nslice * 2 * 8192 * sizeof(__bf16);
  const size_t lds_epi = 128 * 132 * 4;  // padded fp32 staging tile
  const size_t lds = lds_k > lds_epi ? lds_k : lds_epi;
  const bool bk32 = plan.variant == PwVariant::T128Bk32;
  pw_for_nslice<3>(nslice, "pairwise_l2_mfma", [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    // <3, true> is never instantiated: the BK=32 K-loop has no 3-slice form
    if (bk32 && NS <= 2)
      pw_launch<pairwise_l2_kernel<NS, NS <= 2>>(grid, 256, lds, stream, p, xn, yn, out,
                                                 m, n, d, ldo, (int)sqrt_out, rg);
    else
      pw_launch<pairwise_l2_kernel<NS, false>>(grid, 256, lds, stream, p, xn, yn, out,
                                               m, n, d, ldo, (int)sqrt_out, rg);
  });
}

void launch_pairwise_l2_filter(const PwPlan& plan, const void** xsl, const void** csl,
                               const float* xn, const float* yn, const float* thr,
                               float* out_d, int* out_i, int* cnt, int cap,
                               long long col_offset, long long m, long long n, int d,
                               int nslice, hipStream_t stream) {
  if (!plan.error.empty()) throw std::runtime_error(plan.error);
  const SlicePtrs p(xsl, csl, nslice);
  if (plan.variant == PwVariant::Px) {
    constexpr int CT = 8;
    const int n_row_tiles = (int)((m + 127) / 128);
    const int n_groups = (int)((n + (long long)CT * 128 - 1) / ((long long)CT * 128));
    const dim3 grid((unsigned)((long long)n_row_tiles * n_groups));
    const size_t lds = (size_t)(d / 64) * 8192 * 2 + 2 * 16384;  // X + 2 C bufs
    pw_launch<pairwise_l2_filter_px_kernel<CT>>(grid, 256, lds, stream, p.x[0], p.c[0],
                                                xn, yn, thr, out_d, out_i, cnt, cap,
                                                col_offset, m, n, d, n_row_tiles);
    return;
  }
  int rg;
  if (plan.variant == PwVariant::T256) {
    const dim3 grid = supertile_grid(m, n, 256, &rg);
    const size_t lds = 8 * 16384;  // the BK=32 K-loop's 8 x 16 KiB dbuf regions
    pw_for_nslice<2>(nslice, "pairwise filter 256^2 kernel", [&](auto ns) {
      pw_launch<pairwise_l2_filter256_kernel<decltype(ns)::value>>(
          grid, 512, lds, stream, p, xn, yn, thr, out_d, out_i, cnt, cap, col_offset, m,
          n, d, rg);
    });
    return;
  }
  const dim3 grid = supertile_grid(m, n, 128, &rg);
  const size_t lds = (size_t)nslice * 2 * 8192 * sizeof(__bf16);
  pw_for_nslice<3>(nslice, "pairwise_l2_filter", [&](auto ns) {
    pw_launch<pairwise_l2_filter_kernel<decltype(ns)::value>>(
        grid, 256, lds, stream, p, xn, yn, thr, out_d, out_i, cnt, cap, col_offset, m, n,
        d, rg);
  });
}

// ---- include/raft_amd/distance.hpp: the environment-resolved 128^2 kernels
// and the 256^2 tile writer ---------------------------------------------------

void launch_pairwise_l2_mfma(const void** xsl, const void** csl, const float* xn,
                             const float* yn, float* out, long long m, long long n,
                             int d, long long ldo, int nslice, bool sqrt_out,
                             hipStream_t stream) {
  launch_pairwise_l2_tile({pw_auto_128(nslice, d), {}}, xsl, csl, xn, yn, out, m, n, d,
                          ldo, nslice, sqrt_out, stream);
}

void launch_pairwise_l2_mfma256(const void** xsl, const void** csl, const float* xn,
                                const float* yn, float* out, long long m, long long n,
                                int d, long long ldo, int nslice, bool sqrt_out,
                                hipStream_t stream) {
  launch_pairwise_l2_tile({PwVariant::T256, {}}, xsl, csl, xn, yn, out, m, n, d, ldo,
                          nslice, sqrt_out, stream);
}

void launch_pairwise_l2_filter(const void** xsl, const void** csl, const float* xn,
                               const float* yn, const float* thr, float* out_d,
                               int* out_i, int* cnt, int cap, long long col_offset,
                               long long m, long long n, int d, int nslice,
                               hipStream_t stream) {
  const PwEnv& env = pw_env();
  const bool px = env.px && !pw_variant_violation(PwVariant::Px, nslice, n, d);
  launch_pairwise_l2_filter({px ? PwVariant::Px : PwVariant::T128, {}}, xsl, csl, xn, yn,
                            thr, out_d, out_i, cnt, cap, col_offset, m, n, d, nslice,
                            stream);
}

}  // namespace raft_amd
