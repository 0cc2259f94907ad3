// Fused L2-NN, 1-slice X-in-register variant of the 2D-grid engine
// (fused_l2nn_2d.hip): same block -> (row tile, col-tile group) mapping and
// XCD-contiguous swizzle, different inner structure.
//
// WHY: at n = 1024, GT = 8 the 2d engine's block re-stages its 128 x d X
// panel through LDS once per column tile, drains every K-step with
// vmcnt(0) + two barriers and keeps nothing in flight across them. With one
// slice and d <= 256 the panel is 64 KiB per block, 64 VGPRs per lane over 4
// waves, so here
//  * the waves stand 4x1: wave w owns rows 32w .. 32w+31 of the tile and all
//    128 columns. Its X fragments load ONCE, global -> register in MFMA A
//    layout, and stay for all GT column tiles: X never touches LDS;
//  * C is one continuous stream of GT * KT chunks of 128 x 64 bf16 through
//    two 16 KiB LDS buffers. Per chunk: one drain (`s_waitcnt` + raw
//    `s_barrier`, one asm statement), then the next chunk's loads are issued
//    into the other buffer, then the MFMAs run on the current one. One
//    barrier per K-step, and the next tile's first chunk is in flight under
//    the top-2 fold;
//  * a block whose group covers all of n writes dmin / amin / dmin2 itself
//    (what l2nn_combine_kernel<false> would write): no partials, no combine.
// Every output element sees the same MFMA sequence in the same K order as in
// the 2d engine, so the two agree bit for bit.
//
// Measured at 10M x 256, k = 1024: 5.47 ms against the
// 2d engine's 7.61 at GT 8; GT 4 5.99; s_setprio(1) around the MFMA groups
// 5.53 (a loser, removed). The drain is `vmcnt(0) lgkmcnt(0)`: see the loop.

#include <hip/hip_runtime.h>

#include "l2nn_engine.h"
#include "l2nn_top2.h"

namespace raft_amd {

namespace {

constexpr int XREG_CHUNK = 8192;  // bf16 elements of one 128 x 64 C chunk
constexpr int XREG_RING = 2;      // LDS buffers of the C stream (double buffer)

}  // namespace

template <int KT /* d / 64 */, int GT>
__launch_bounds__(256, 2)
__global__ void fused_l2nn_xreg_kernel(const __bf16* __restrict__ x,
                                       const __bf16* __restrict__ c,
                                       const float* __restrict__ cn,
                                       const float* __restrict__ xn,
                                       float* __restrict__ pd,
                                       float* __restrict__ pd2,
                                       int* __restrict__ pi,
                                       float* __restrict__ dmin,
                                       int* __restrict__ amin,
                                       float* __restrict__ dmin2,
                                       long long m, int n, int n_groups) {
  extern __shared__ __bf16 smem[];
  constexpr int d = KT * 64;

  const int t = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const long long row0 = (long long)(t / n_groups) * 128;
  const int grp = t % n_groups;

  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = threadIdx.x / RAFT_AMD_WAVE;

  // the wave's X panel, MFMA A layout: a[kt][kf][fr] is row
  // 32w + 16fr + (lane & 15), k = 64kt + 32kf + 8(lane >> 4) .. +7
  bf16x8 a[KT][2][2];
#pragma unroll
  for (int fr = 0; fr < 2; fr++) {
    long long r = row0 + w * 32 + fr * 16 + (lane & 15);
    if (r > m - 1) r = m - 1;
    const __bf16* xp = x + r * d + (lane >> 4) * 8;
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
      for (int kf = 0; kf < 2; kf++)
        a[kt][kf][fr] = *reinterpret_cast<const bf16x8*>(xp + kt * 64 + kf * 32);
  }

  // C staging, the source-swizzled addressing of mfma_tile_kloop: this
  // thread's 4 sources of the group's chunk (g = 0, kt = 0), and the LDS
  // destinations inside a ring buffer (n % 128 == 0: no column clamp)
  const __bf16* cp[4];
  int ldst[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int o_src = mfma_swz(j * 4096 + (int)threadIdx.x * 16);
    cp[j] = c + ((long long)grp * GT * 128 + (o_src >> 7)) * d + ((o_src & 127) >> 1);
    ldst[j] = (j * 4096 + w * 1024) / 2;
  }
  // B fragment (column fc*16 + (lane & 15), k half kf) byte offset inside a
  // ring buffer: the swizzle reads row bits 0..2 only, which fc*16 leaves
  // alone, so fragment fc is boff[kf] + fc * 2048 (an immediate offset)
  int boff[2];
#pragma unroll
  for (int kf = 0; kf < 2; kf++)
    boff[kf] = mfma_swz((lane & 15) * 128 + (kf * 32 + (lane >> 4) * 8) * 2);

  float best[2][4], best2[2][4];
  int bidx[2][4];
  top2_init(best, best2, bidx);

#pragma unroll
  for (int j = 0; j < 4; j++) GLOAD_LDS(cp[j], smem + ldst[j]);
  int par = 0;  // odd KT: buffer of the tile's first chunk

#pragma unroll 1
  for (int g = 0; g < GT; g++) {
    f32x4 acc[2][8];
#pragma unroll
    for (int fr = 0; fr < 2; fr++)
#pragma unroll
      for (int fc = 0; fc < 8; fc++) acc[fr][fc] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int kt = 0; kt < KT; kt++) {
      // this wave's loads of the chunk have landed; past the barrier so have
      // everyone's, and every wave is done reading the other buffer.
      // lgkmcnt(0): the compiler moves the previous chunk's last MFMAs, and
      // with them the wait for their ds_reads, below this statement; the
      // reads must have returned before another wave may overwrite the buffer
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      // chunk g*KT + kt sits in buffer (g*KT + kt) & 1: compile-time for
      // even KT, alternating per tile for odd KT
      const int buf = (KT & 1) ? ((kt & 1) ^ par) : (kt & 1);
      const int nxt = buf ^ 1;
      if (kt + 1 < KT) {
#pragma unroll
        for (int j = 0; j < 4; j++)
          GLOAD_LDS(cp[j] + (kt + 1) * 64, smem + nxt * XREG_CHUNK + ldst[j]);
      } else if (g + 1 < GT) {
        // the next tile's first chunk: in flight under the top-2 fold
#pragma unroll
        for (int j = 0; j < 4; j++)
          GLOAD_LDS(cp[j] + 128 * d, smem + nxt * XREG_CHUNK + ldst[j]);
      }
      // keep the issue here, ahead of the chunk's MFMAs (left alone, the
      // scheduler sinks it to just before the next drain)
      __builtin_amdgcn_sched_barrier(0);
      const char* cs = reinterpret_cast<const char*>(smem + buf * XREG_CHUNK);
#pragma unroll
      for (int kf = 0; kf < 2; kf++) {
        bf16x8 b[8];
#pragma unroll
        for (int fc = 0; fc < 8; fc++)
          b[fc] = *reinterpret_cast<const bf16x8*>(cs + boff[kf] + fc * 2048);
#pragma unroll
        for (int fr = 0; fr < 2; fr++)
#pragma unroll
          for (int fc = 0; fc < 8; fc++)
            acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[kt][kf][fr], b[fc], acc[fr][fc], 0, 0, 0);
      }
    }
    if (KT & 1) par ^= 1;
#pragma unroll
    for (int j = 0; j < 4; j++) cp[j] += 128 * d;

    // lane-local running top-2 across the group's tiles (disjoint columns)
    top2_fold_tile(acc, cn, (grp * GT + g) * 128 + (lane & 15), best, best2, bidx);
  }

  // every lane parks its 8 (fr, reg) triples as candidate lane & 15 of its
  // row ([128][17] planes, 26 KiB of the ring; park's first barrier ends the
  // stream's use of it and no load is outstanding); one thread per row merges
  top2_park_tile<2, 128 * 17, 17, 1>(smem, true, w * 32, lane, lane & 15, best, best2,
                                     bidx);
  const int rl = threadIdx.x;
  if (rl < 128 && row0 + rl < m) {
    if (n_groups == 1) {
      // the only group: finish the row as l2nn_combine_kernel<false> does
      float v, v2;
      int vi;
      top2_merge_parked<16, 128 * 17, 17, 1, false>(smem, rl, v, v2, vi);
      const float xr = xn[row0 + rl];
      dmin[row0 + rl] = fmaxf(v + xr, 0.f);
      amin[row0 + rl] = vi;
      if (dmin2) dmin2[row0 + rl] = v2 + xr;
    } else {
      top2_write_partial<16, 128 * 17, 17, 1, false>(smem, rl, pd, pd2, pi,
                                                     (long long)grp * m + row0 + rl);
    }
  }
}

// resolved gt divides n / 128 (l2nn_resolve_engine); d is 64 .. 256
void launch_l2nn_xreg(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                      float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                      long long m, int n, int d, int gt, hipStream_t stream) {
  const int n_groups = n / 128 / gt;
  const int grid = (int)((m + 127) / 128) * n_groups;
  // the ring; the [128][17] epilogue (26 KiB) reuses it
  const size_t lds = (size_t)XREG_RING * XREG_CHUNK * sizeof(__bf16);
#define L2NN_XREG_LAUNCH(K, G)                                                  \
  hipLaunchKernelGGL((fused_l2nn_xreg_kernel<K, G>), dim3(grid), dim3(256), lds, \
                     stream, p.x[0], p.c[0], cn, xn, pd, pd2, pi, dmin, amin,   \
                     dmin2, m, n, n_groups)
#define L2NN_XREG_KT(G)                      \
  do {                                       \
    if (d == 64) L2NN_XREG_LAUNCH(1, G);     \
    else if (d == 128) L2NN_XREG_LAUNCH(2, G); \
    else if (d == 192) L2NN_XREG_LAUNCH(3, G); \
    else L2NN_XREG_LAUNCH(4, G);             \
  } while (0)
  if (gt == 1) L2NN_XREG_KT(1);
  else if (gt == 2) L2NN_XREG_KT(2);
  else if (gt == 4) L2NN_XREG_KT(4);
  else L2NN_XREG_KT(8);
#undef L2NN_XREG_KT
#undef L2NN_XREG_LAUNCH
  if (n_groups > 1)
    launch_l2nn_combine<false>(pd, pd2, pi, xn, dmin, amin, dmin2, m, n_groups, stream);
}

}  // namespace raft_amd
