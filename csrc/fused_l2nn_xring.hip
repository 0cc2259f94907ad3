// Fused L2-NN, 1-slice X-in-register engine with a counted C ring: the
// 2d_xreg kernel (fused_l2nn_xreg.hip) with the memory waits of its tile loop
// taken out. Grid, XCD swizzle, 4x1 wave layout, X fragments in registers,
// the source-swizzled C image, the top-2 fold / park / merge and the direct
// write are 2d_xreg's; every output element sees the same MFMA sequence in
// the same K order, so the two agree bit for bit.
//
// WHAT CHANGED, and why (docs/performance.md, round 4):
//  * the C stream's LDS-DMA pieces are issued from inline asm, so the
//    compiler keeps no books on them: in 2d_xreg it answered every in-flight
//    piece with a `vmcnt(0)` ahead of the tile's first MFMA, which made chunk
//    0's MFMAs wait for chunk 1. Here the ring has four 16 KiB buffers, up
//    to three chunks are in flight and the waits are counted by hand;
//  * the group's ||c||^2 values are staged in LDS once, in the prologue, so
//    the tile loop holds no VMEM instruction but the stream (a plain load in
//    the loop would make every hand count wrong);
//  * the B fragments are read one MFMA group ahead: the reads of a chunk's
//    second k half stand before the MFMAs of its first, and the next chunk's
//    barrier stands between the two MFMA groups, so that the reads of the
//    next chunk's first k half stand before the MFMAs of this one's second.
//    The compiler counts its own ds_reads (`lgkmcnt(n)` ladders).
//
// THE WAIT AND BARRIER TABLE. The stream is chunks p = 0 .. N-1 (N = GT * KT),
// chunk p lives in ring buffer p & 3, every wave issues 4 pieces per chunk
// and they return in issue order. I(q) is the issue of chunk q, W(q) / B(q)
// the wait and the raw barrier for chunk q, R0(q) / R1(q) the ds_reads of
// its k half 0 / 1, M0(q) / M1(q) the MFMA groups that consume them.
//
//   prologue   I(0) I(1) I(2)   W(0) B(0)   R0(0)
//   body p     R1(p)  M0(p)  W(p+1) B(p+1)  I(p+3)  R0(p+1)  M1(p)
//              (the last body has no W, B, I, R0)
//
//   chunk q is retired   by W(q): at W(q), q >= 1, the wave has issued chunks
//                        .. q+1 and nothing later (I(q+1) stands in body
//                        q-2), so `vmcnt(4)` leaves only the 4 pieces of
//                        chunk q+1 in flight; when chunk q+1 does not exist
//                        (q = N-1) it is `vmcnt(0)`: the counts over the
//                        stream's last two chunks are 4, 0. W(0) is written
//                        to leave chunks 1 and 2: `vmcnt(8)`, 4 at N = 2, 0
//                        at N = 1. What runs is stricter: the X panel's
//                        plain loads are consumed just before it, and the
//                        compiler's own wait for the last of them is a
//                        `vmcnt(0)`, which drains the pieces too (in either
//                        issue order). Once per block.
//   chunk q is published by B(q): every wave has passed its own W(q).
//   buffer q & 3 is freed by B(q+1): the chunk's last reads, R1(q), stand
//                        before W(q+1), whose `lgkmcnt(0)` retires them, and
//                        past B(q+1) that holds for every wave. Its next
//                        writer is I(q+4), which stands after B(q+2).
//   I(p+3) writes buffer (p+3) & 3 = (p-1) & 3, freed by B(p).
//
// A read placed before the count that retires its chunk passes every test
// whenever the DMA happens to land first: R0(q) and R1(q) stand after B(q) in
// the source, and the asm statements' memory clobbers keep them there (the
// compiler may move MFMAs across a W / B, never a read). No `__syncthreads()`
// runs while a piece is outstanding; the park's first barrier follows an
// explicit `vmcnt(0)`.
//
// LDS: 4 x 16 KiB ring + GT * 128 floats = 68 KiB at GT 8, 2 blocks / CU.

#include <hip/hip_runtime.h>

#include "l2nn_engine.h"
#include "l2nn_top2.h"

namespace raft_amd {

namespace {

constexpr int XRING_CHUNK = 8192;  // bf16 elements of one 128 x 64 C chunk
constexpr int XRING_RING = 4;      // LDS buffers of the C stream

// one LDS-DMA piece: 64 lanes x 16 B from each lane's `gsrc` to LDS bytes
// lds_dst .. lds_dst + 1023 (wave-uniform). M0 is saved, set, used and
// restored inside the one statement; the compiler does not count the load.
__device__ __forceinline__ void xring_glds16(const __bf16* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}

// W + B of the table: at most CNT pieces of this wave still in flight, every
// ds_read of this wave returned, then the raw barrier
template <int CNT>
__device__ __forceinline__ void xring_wait_barrier() {
  static_assert(CNT == 0 || CNT == 4 || CNT == 8, "whole chunks of 4 pieces");
  if constexpr (CNT == 8)
    asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if constexpr (CNT == 4)
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

}  // namespace

template <int KT /* d / 64 */, int GT>
__launch_bounds__(256, 2)
__global__ void fused_l2nn_xring_kernel(const __bf16* __restrict__ x,
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
  constexpr int N = GT * KT;  // chunks of the block's stream

  const int t = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const long long row0 = (long long)(t / n_groups) * 128;
  const int grp = t % n_groups;

  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / RAFT_AMD_WAVE);

  // C staging, the source-swizzled addressing of mfma_tile_kloop: this
  // thread's 4 sources of the group's chunk (g = 0, kt = 0), and the wave's
  // LDS byte destinations inside ring buffer 0 (n % 128 == 0: no column clamp)
  const unsigned ring0 = __builtin_amdgcn_readfirstlane(
      (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) void*)smem);
  const __bf16* cp[4];
  unsigned ldst[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int o_src = mfma_swz(j * 4096 + (int)threadIdx.x * 16);
    cp[j] = c + ((long long)grp * GT * 128 + (o_src >> 7)) * d + ((o_src & 127) >> 1);
    ldst[j] = ring0 + j * 4096 + w * 1024;
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

  // Prologue, in issue order: the group's GT * 128 norms (plain loads), I(0)
  // I(1) I(2), the X panel (plain loads). The compiler counts its own loads
  // only, and every count it takes is at least as strict with the uncounted
  // pieces in the queue. All plain loads are consumed here, before the loop:
  // left outstanding at its head, they would put the compiler's own
  // `vmcnt(n)` ladder into every tile and drain the ring with it.
  constexpr int CNV = (GT * 128 + 255) / 256;
  float cn_t[CNV];
#pragma unroll
  for (int v = 0; v < CNV; v++) {
    // 256 threads: only GT 1 has fewer norms than threads
    const int i = GT == 1 ? (int)threadIdx.x & 127 : (int)threadIdx.x + v * 256;
    cn_t[v] = cn[grp * GT * 128 + i];
  }
#pragma unroll
  for (int q = 0; q < 3 && q < N; q++)
#pragma unroll
    for (int j = 0; j < 4; j++)
      xring_glds16(cp[j] + (q / KT) * 128 * d + (q % KT) * 64,
                   ldst[j] + q * (XRING_CHUNK * 2));

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
  // the norms go behind the ring; published by B(0), whose wait carries
  // lgkmcnt(0). Padded centroid rows keep their +inf.
  float* cns = reinterpret_cast<float*>(smem + XRING_RING * XRING_CHUNK);
#pragma unroll
  for (int v = 0; v < CNV; v++) {
    const int i = (int)threadIdx.x + v * 256;
    if (GT > 1 || i < 128) cns[i] = cn_t[v];
  }
  // the X panel has landed before the loop is entered
#pragma unroll
  for (int kt = 0; kt < KT; kt++)
#pragma unroll
    for (int kf = 0; kf < 2; kf++)
#pragma unroll
      for (int fr = 0; fr < 2; fr++) asm volatile("" : "+v"(a[kt][kf][fr]));

  // W(0) B(0), R0(0)
  xring_wait_barrier<(N >= 3 ? 8 : N == 2 ? 4 : 0)>();
  bf16x8 b0[8], b1[8];  // the fragments of k half 0 / 1
#pragma unroll
  for (int fc = 0; fc < 8; fc++)
    b0[fc] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(smem) +
                                              boff[0] + fc * 2048);
  // ring buffer of the tile's first chunk, (g * KT) & 3: always 0 at KT 4,
  // carried at run time otherwise
  int base = 0;

#pragma unroll 1
  for (int g = 0; g < GT; g++) {
    f32x4 acc[2][8];
#pragma unroll
    for (int fr = 0; fr < 2; fr++)
#pragma unroll
      for (int fc = 0; fc < 8; fc++) acc[fr][fc] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int kt = 0; kt < KT; kt++) {
      // body p, p = g * KT + kt (the table above)
      const int buf = KT == 4 ? kt : ((base + kt) & 3);
      const char* cs = reinterpret_cast<const char*>(smem + buf * XRING_CHUNK);
      // R1(p), M0(p)
#pragma unroll
      for (int fc = 0; fc < 8; fc++)
        b1[fc] = *reinterpret_cast<const bf16x8*>(cs + boff[1] + fc * 2048);
#pragma unroll
      for (int fr = 0; fr < 2; fr++)
#pragma unroll
        for (int fc = 0; fc < 8; fc++)
          acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kt][0][fr], b0[fc],
                                                                acc[fr][fc], 0, 0, 0);
      if (kt + 1 < KT || g + 1 < GT) {
        // W(p+1) B(p+1): chunk p+2 stays in flight where it exists
        if (g + (kt + 2) / KT < GT)
          xring_wait_barrier<4>();
        else
          xring_wait_barrier<0>();
        // I(p+3): chunk (kt + 3) % KT of tile g + (kt + 3) / KT
        const int dt = (kt + 3) / KT, kk = (kt + 3) % KT;
        if (g + dt < GT) {
          const int nxt = (buf + 3) & 3;
#pragma unroll
          for (int j = 0; j < 4; j++)
            xring_glds16(cp[j] + dt * 128 * d + kk * 64,
                         ldst[j] + nxt * (XRING_CHUNK * 2));
        }
        // R0(p+1): at a tile's last chunk these ride through the fold
        const char* ns =
            reinterpret_cast<const char*>(smem + ((buf + 1) & 3) * XRING_CHUNK);
#pragma unroll
        for (int fc = 0; fc < 8; fc++)
          b0[fc] = *reinterpret_cast<const bf16x8*>(ns + boff[0] + fc * 2048);
      }
      // M1(p)
#pragma unroll
      for (int fr = 0; fr < 2; fr++)
#pragma unroll
        for (int fc = 0; fc < 8; fc++)
          acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kt][1][fr], b1[fc],
                                                                acc[fr][fc], 0, 0, 0);
    }
    if (KT != 4) base = (base + KT) & 3;
#pragma unroll
    for (int j = 0; j < 4; j++) cp[j] += 128 * d;

    // lane-local running top-2 across the group's tiles (disjoint columns);
    // the tile's norms come from LDS (reading them under the last chunk's
    // MFMAs, eight more live registers there, spilled)
    float cn_r[8];
#pragma unroll
    for (int fc = 0; fc < 8; fc++) cn_r[fc] = cns[g * 128 + (lane & 15) + fc * 16];
    top2_fold_tile_cn(acc, cn_r, (grp * GT + g) * 128 + (lane & 15), best, best2, bidx);
  }

  // every lane parks its 8 (fr, reg) triples as candidate lane & 15 of its
  // row ([128][17] planes, 26 KiB of the ring). W(N-1) left no piece in
  // flight; the wait says so where the park's barrier needs it
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
void launch_l2nn_xring(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                       float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                       long long m, int n, int d, int gt, hipStream_t stream) {
  const int n_groups = n / 128 / gt;
  const int grid = (int)((m + 127) / 128) * n_groups;
  // the ring (the [128][17] epilogue, 26 KiB, reuses it) and the norms
  const size_t lds =
      (size_t)XRING_RING * XRING_CHUNK * sizeof(__bf16) + (size_t)gt * 128 * sizeof(float);
  // the ring alone is the 64 KiB default dynamic-LDS limit: every
  // instantiation asks for its ring + norms
  static bool attr_set = false;
  if (!attr_set) {
#define L2NN_XRING_ATTR(K, G)                                                \
  HIP_CHECK(hipFuncSetAttribute((const void*)&fused_l2nn_xring_kernel<K, G>, \
                                hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                XRING_RING * XRING_CHUNK * 2 + G * 128 * 4))
#define L2NN_XRING_ATTR_KT(G) \
  L2NN_XRING_ATTR(1, G);      \
  L2NN_XRING_ATTR(2, G);      \
  L2NN_XRING_ATTR(3, G);      \
  L2NN_XRING_ATTR(4, G)
    L2NN_XRING_ATTR_KT(1);
    L2NN_XRING_ATTR_KT(2);
    L2NN_XRING_ATTR_KT(4);
    L2NN_XRING_ATTR_KT(8);
#undef L2NN_XRING_ATTR_KT
#undef L2NN_XRING_ATTR
    attr_set = true;
  }
#define L2NN_XRING_LAUNCH(K, G)                                                  \
  hipLaunchKernelGGL((fused_l2nn_xring_kernel<K, G>), dim3(grid), dim3(256), lds, \
                     stream, p.x[0], p.c[0], cn, xn, pd, pd2, pi, dmin, amin,    \
                     dmin2, m, n, n_groups)
#define L2NN_XRING_KT(G)                        \
  do {                                          \
    if (d == 64) L2NN_XRING_LAUNCH(1, G);       \
    else if (d == 128) L2NN_XRING_LAUNCH(2, G); \
    else if (d == 192) L2NN_XRING_LAUNCH(3, G); \
    else L2NN_XRING_LAUNCH(4, G);               \
  } while (0)
  if (gt == 1) L2NN_XRING_KT(1);
  else if (gt == 2) L2NN_XRING_KT(2);
  else if (gt == 4) L2NN_XRING_KT(4);
  else L2NN_XRING_KT(8);
#undef L2NN_XRING_KT
#undef L2NN_XRING_LAUNCH
  if (n_groups > 1)
    launch_l2nn_combine<false>(pd, pd2, pi, xn, dmin, amin, dmin2, m, n_groups, stream);
}

}  // namespace raft_amd
