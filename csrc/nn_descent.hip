// NN-descent: the two device steps of the kNN-graph build of
// raft_amd/neighbors/nn_descent.py, which states the algorithm.
//
// Reference parity (WHAT): cuvs::neighbors::nn_descent (GNND local join and
// list update). HOW is CDNA4-native: the per-node all-pairs distances are a
// 64 x 128 bf16 MFMA tile whose operands are GATHERED rows, and the neighbour
// lists are merged by one block per target with no lock between blocks.
//
// ---- nn_descent_join: one 256-thread block per node -------------------------
// The node's sample lists NEW[2S] and OLD[2S] (S <= 32, -1 = no row) are padded
// to 64 rows each. A = NEW (64 rows), B = [NEW | OLD] (128 rows): the first
// half of B is A itself, so one K-chunk of 64 features is two [64][64] bf16
// tiles in LDS, 8 KiB each, and the double buffer is 32 KiB. With the ids,
// norms and best-keys the block holds under 35 KiB, so four blocks share a CU.
//
// Gather: a chunk is 128 rows x 8 slots of 8 features; thread t owns slots
// (row j * 32 + t / 8, slot t % 8), j = 0..3, so eight consecutive lanes read
// one row's 128 B (bf16 / fp16) or 256 B (fp32) contiguously. A slot is one
// 16-byte load of 8 bf16 / fp16, or two 16-byte loads of 4 fp32 narrowed to
// bf16 in registers (fp16 goes through fp32), and one 16-byte store to the
// XOR-swizzled tile (mfma_swz, rows of 128 B). A slot that crosses d, and every
// slot of a data set whose base or row pitch is not 16-byte aligned, takes the
// element-wise path: the same elements by guarded scalar loads, zeros past d.
// An id outside [0, n) is replaced by -1 before an address is formed; a -1 row
// loads nothing and is zero.
//
// Pipeline: the loads of chunk t + 1 are issued into registers, the MFMAs of
// chunk t run from LDS buffer t & 1, then the registers are narrowed and stored
// to the other buffer and ONE barrier ends the step. The random-row gather is
// the latency-bound part and spends its flight time under the matrix work.
//
// Wave split: the four waves form a 2 x 2 grid, wave (wr, wc) owns rows
// [32 wr, 32 wr + 32) of A and columns [64 wc, 64 wc + 64) of B: acc[2][4]
// fragments of 16 x 16 (32 VGPRs), per 32-feature half step 2 A and 4 B
// fragment reads (ds_read_b128) feed 8 mfma_f32_16x16x32_bf16. wc = 0 is
// NEW x NEW, wc = 1 is NEW x OLD; a wave whose half has no row skips its MFMAs.
//
// Epilogue, in registers and LDS only: value = (nu + nv) - 2 dot (the sum of
// norms first, so value(u, v) == value(v, u)), or -dot for inner product; NaN
// becomes +inf, -0 becomes +0. key = (ordered value bits << 32) | id. Per row
// the 4 column fragments are reduced in the lane, then over the 16 lanes of a
// fragment row by an xor butterfly, then one 64-bit LDS atomicMin per (wave,
// row) into rowBestNew (wc = 0) or rowBestOld (wc = 1). Waves with wc = 1 also
// reduce per column over their 8 rows and the 4 lane groups and atomicMin into
// colBestNew. 3 * 2S threads decode the triples (target, id, value) and write
// them coalesced; the distance tile never reaches memory.
//
// ---- nn_descent_merge: one 256-thread block per target ----------------------
// The host groups the triples by target (a stable sort of the target column and
// segment offsets [n + 1]); a block with an empty segment returns at once. The
// list (K <= 256 entries) lives in LDS as value / id / flag arrays. Per round
// up to 512 - K triples of the segment join it as 64-bit keys in a buffer of
// P = pow2(K + chunk) <= 512 slots:
//   sort 1 by (id, source, value): a list entry carries its POSITION instead of
//     the value and source 0, so it precedes every triple of its id; an entry
//     whose id equals its predecessor's is a repeat and drops out;
//   sort 2 by (value, id) with the new flag riding in bit 31 of the low word
//     (ids are below 2^31), masked out of the comparison;
//   the first K keys are decoded back into the list.
// A hub target whose segment exceeds one chunk loops. New flags are written
// with the list, and (new flags after - new flags before) is added to the
// device counter with one integer atomic per block.
//
// REASONED, not measured: the tile split, the four-blocks-per-CU LDS budget and
// the chunk size of the merge; benchmarks/bench_nn_descent.py times the whole
// build.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "common.h"
#include "mfma_common.h"

namespace raft_amd {

constexpr int NND_BLOCK = 256;
constexpr int NND_MAX_D = 4096;
constexpr int NND_MAX_SAMPLES = 32;
constexpr int NND_MAX_K = 256;
constexpr int NND_MERGE_SLOTS = 512;
constexpr unsigned long long NND_NONE = ~0ull;

// ascending-as-unsigned bits of a value; NaN -> +inf, -0 -> +0
__device__ __forceinline__ unsigned int nnd_ordered(float v) {
  if (v != v) v = INFINITY;
  if (v == 0.f) v = 0.f;
  const unsigned int b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float nnd_value(unsigned int b) {
  return __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b);
}

// element types: a slot is 8 features, LOADS 16-byte pieces
struct NndF32 {
  using raw = float;
  static constexpr int LOADS = 2;
  __device__ __forceinline__ static __bf16 narrow(raw v) { return (__bf16)v; }
};
struct NndBF16 {
  using raw = unsigned short;
  static constexpr int LOADS = 1;
};
struct NndF16 {
  using raw = _Float16;
  static constexpr int LOADS = 1;
  __device__ __forceinline__ static __bf16 narrow(raw v) { return (__bf16)(float)v; }
};

// features [k, k + 8) of a row; a null row gives zeros and reads nothing
template <typename E>
__device__ __forceinline__ void nnd_load_slot(uint4 (&w)[E::LOADS],
                                              const typename E::raw* __restrict__ row, int k,
                                              int d, bool vec) {
  using raw = typename E::raw;
#pragma unroll
  for (int i = 0; i < E::LOADS; i++) w[i] = make_uint4(0u, 0u, 0u, 0u);
  if (row == nullptr || k >= d) return;
  if (vec && k + 8 <= d) {
#pragma unroll
    for (int i = 0; i < E::LOADS; i++) w[i] = reinterpret_cast<const uint4*>(row + k)[i];
  } else {
    raw x[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      x[e] = (raw)0;
      if (k + e < d) x[e] = row[k + e];
    }
    __builtin_memcpy(w, x, sizeof(x));
  }
}

template <typename E>
__device__ __forceinline__ uint4 nnd_to_bf16(const uint4 (&w)[E::LOADS]) {
  if constexpr (E::LOADS == 1 && sizeof(typename E::raw) == 2 &&
                !__is_same(typename E::raw, _Float16)) {
    return w[0];
  } else {
    typename E::raw x[8];
    __builtin_memcpy(x, w, sizeof(x));
    __bf16 h[8];
#pragma unroll
    for (int e = 0; e < 8; e++) h[e] = E::narrow(x[e]);
    uint4 out;
    __builtin_memcpy(&out, h, sizeof(out));
    return out;
  }
}

template <typename E>
__launch_bounds__(NND_BLOCK)
__global__ void nn_descent_join_kernel(const typename E::raw* __restrict__ data, long long n,
                                       long long pitch, const float* __restrict__ norms,
                                       const int* __restrict__ new_ids,
                                       const int* __restrict__ old_ids, int* __restrict__ out_tgt,
                                       int* __restrict__ out_id, float* __restrict__ out_val,
                                       int d, int S2, bool vec, bool ip) {
  using raw = typename E::raw;
  __shared__ __attribute__((aligned(16))) unsigned char tiles[2][2][8192];  // [buffer][NEW | OLD]
  __shared__ int sid[128];                 // NEW ids [0, 64), OLD ids [64, 128)
  __shared__ float snorm[128];
  __shared__ unsigned long long best[3][64];  // rowBestNew, rowBestOld, colBestNew

  const int t = threadIdx.x;
  const int lane = t % RAFT_AMD_WAVE;
  const int wave = t / RAFT_AMD_WAVE;
  const int wr = wave >> 1, wc = wave & 1;
  const long long node = blockIdx.x;

  int my_id = -1;
  if (t < 128) {
    const int idx = t & 63;
    if (idx < S2) my_id = (t < 64 ? new_ids : old_ids)[node * S2 + idx];
    if (my_id < 0 || my_id >= n) my_id = -1;
    sid[t] = my_id;
    snorm[t] = my_id >= 0 ? norms[my_id] : 0.f;
  }
  if (t < 192) best[t >> 6][t & 63] = NND_NONE;
  // both are barriers; the results are block-uniform
  const bool any_new = __syncthreads_or(t < 64 && my_id >= 0);
  const bool any_old = __syncthreads_or(t >= 64 && t < 128 && my_id >= 0);
  const int n_out = 3 * S2;
  if (!any_new) {
    if (t < n_out) {
      out_tgt[node * n_out + t] = -1;
      out_id[node * n_out + t] = -1;
      out_val[node * n_out + t] = INFINITY;
    }
    return;
  }

  // this thread's four slots of a chunk
  const int q = t & 7;
  const raw* rowp[4];
  int off[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = j * 32 + (t >> 3);
    const int id = sid[r];
    rowp[j] = id >= 0 ? data + (long long)id * pitch : nullptr;
    off[j] = mfma_swz((r & 63) * 128 + q * 16);
  }

  f32x4 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 w[4][E::LOADS];
  auto gather = [&](int kt) {
#pragma unroll
    for (int j = 0; j < 4; j++) nnd_load_slot<E>(w[j], rowp[j], kt * 64 + q * 8, d, vec);
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      *reinterpret_cast<uint4*>(&tiles[buf][j >> 1][off[j]]) = nnd_to_bf16<E>(w[j]);
  };

  const int k_tiles = (d + 63) / 64;
  const bool work = wc == 0 || any_old;
  gather(0);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < k_tiles; kt++) {
    const int cur = kt & 1;
    if (kt + 1 < k_tiles) gather(kt + 1);
    if (work) {
#pragma unroll
      for (int kf = 0; kf < 2; kf++) {
        bf16x8 a_frag[2], b_frag[4];
        const int kbyte = (kf * 32 + (lane >> 4) * 8) * 2;
#pragma unroll
        for (int fr = 0; fr < 2; fr++) {
          const int r = wr * 32 + fr * 16 + (lane & 15);
          a_frag[fr] =
              *reinterpret_cast<const bf16x8*>(&tiles[cur][0][mfma_swz(r * 128 + kbyte)]);
        }
#pragma unroll
        for (int fc = 0; fc < 4; fc++) {
          const int c = fc * 16 + (lane & 15);
          b_frag[fc] =
              *reinterpret_cast<const bf16x8*>(&tiles[cur][wc][mfma_swz(c * 128 + kbyte)]);
        }
#pragma unroll
        for (int fr = 0; fr < 2; fr++)
#pragma unroll
          for (int fc = 0; fc < 4; fc++)
            acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag[fr], b_frag[fc],
                                                                  acc[fr][fc], 0, 0, 0);
      }
    }
    // buffer cur ^ 1 was last read in step kt - 1, which ended with a barrier
    if (kt + 1 < k_tiles) stage(cur ^ 1);
    __syncthreads();
  }

  // epilogue: acc[fr][fc][reg] is row (lane >> 4) * 4 + reg, column lane & 15
  if (work) {
    unsigned long long cb[4] = {NND_NONE, NND_NONE, NND_NONE, NND_NONE};
#pragma unroll
    for (int fr = 0; fr < 2; fr++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int row = wr * 32 + fr * 16 + (lane >> 4) * 4 + reg;
        const int uid = sid[row];
        const float nu = snorm[row];
        unsigned long long rb = NND_NONE;
#pragma unroll
        for (int fc = 0; fc < 4; fc++) {
          const int col = wc * 64 + fc * 16 + (lane & 15);
          const int vid = sid[col];
          if (uid >= 0 && vid >= 0 && uid != vid) {
            const float dot = acc[fr][fc][reg];
            const float v = ip ? -dot : (nu + snorm[col]) - 2.f * dot;
            const unsigned long long hi = (unsigned long long)nnd_ordered(v) << 32;
            const unsigned long long kr = hi | (unsigned int)vid;
            const unsigned long long kc = hi | (unsigned int)uid;
            rb = kr < rb ? kr : rb;
            cb[fc] = kc < cb[fc] ? kc : cb[fc];
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const unsigned long long other = __shfl_xor(rb, o, RAFT_AMD_WAVE);
          rb = other < rb ? other : rb;
        }
        if ((lane & 15) == 0 && rb != NND_NONE) atomicMin(&best[wc][row], rb);
      }
    if (wc == 1) {
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
          const unsigned long long other = __shfl_xor(cb[fc], o, RAFT_AMD_WAVE);
          cb[fc] = other < cb[fc] ? other : cb[fc];
        }
        if (lane < 16 && cb[fc] != NND_NONE) atomicMin(&best[2][fc * 16 + lane], cb[fc]);
      }
    }
  }
  __syncthreads();

  if (t < n_out) {
    const int seg = t / S2, idx = t - seg * S2;
    const int u = sid[(seg == 2 ? 64 : 0) + idx];
    const unsigned long long key = best[seg][idx];
    const bool hit = u >= 0 && key != NND_NONE;
    out_tgt[node * n_out + t] = hit ? u : -1;
    out_id[node * n_out + t] = hit ? (int)(unsigned int)key : -1;
    out_val[node * n_out + t] = hit ? nnd_value((unsigned int)(key >> 32)) : INFINITY;
  }
}

// ascending bitonic sort of keys[0, P), P a power of two; MASKED ignores bit 31
template <bool MASKED>
__device__ __forceinline__ void nnd_bitonic(unsigned long long* keys, int P) {
  constexpr unsigned long long M = MASKED ? ~(1ull << 31) : ~0ull;
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < (P >> 1); i += NND_BLOCK) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = keys[lo], b = keys[hi];
        if (((a & M) > (b & M)) == up) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
    }
  }
  __syncthreads();
}

__launch_bounds__(NND_BLOCK)
__global__ void nn_descent_merge_kernel(float* __restrict__ vals, int* __restrict__ ids,
                                        unsigned char* __restrict__ flags, long long n, int K,
                                        const long long* __restrict__ seg_off,
                                        const int* __restrict__ cand_id,
                                        const float* __restrict__ cand_val,
                                        unsigned long long* __restrict__ counter) {
  __shared__ unsigned long long keys[NND_MERGE_SLOTS];
  __shared__ float lval[NND_MAX_K];
  __shared__ int lid[NND_MAX_K];
  __shared__ unsigned char lflag[NND_MAX_K];

  const int t = threadIdx.x;
  const long long u = blockIdx.x;
  const long long s0 = seg_off[u], s1 = seg_off[u + 1];
  if (s0 >= s1) return;  // block-uniform, ahead of the first barrier

  bool mine = false;
  if (t < K) {
    int id = ids[u * K + t];
    if (id < 0 || id >= n) id = -1;
    lid[t] = id;
    lval[t] = vals[u * K + t];
    mine = id >= 0 && flags[u * K + t] != 0;
    lflag[t] = mine;
  }
  const int before = __syncthreads_count(mine);

  for (long long pos = s0; pos < s1; pos += NND_MERGE_SLOTS - K) {
    const long long left = s1 - pos;
    const int c = left < NND_MERGE_SLOTS - K ? (int)left : NND_MERGE_SLOTS - K;
    int P = 2;
    while (P < K + c) P <<= 1;

    for (int i = t; i < P; i += NND_BLOCK) {
      unsigned long long key = NND_NONE;
      if (i < K) {
        if (lid[i] >= 0) key = ((unsigned long long)(unsigned int)lid[i] << 33) | (unsigned int)i;
      } else if (i < K + c) {
        const int id = cand_id[pos + i - K];
        if (id >= 0 && id < n && id != u)
          key = ((unsigned long long)(unsigned int)id << 33) | (1ull << 32) |
                nnd_ordered(cand_val[pos + i - K]);
      }
      keys[i] = key;
    }
    nnd_bitonic<false>(keys, P);

    // a repeat equals its predecessor's id; the rest become (value, flag, id) keys
    unsigned long long k2[2] = {NND_NONE, NND_NONE};
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int i = t + r * NND_BLOCK;
      if (i < P) {
        const unsigned long long k = keys[i];
        const bool dup = i > 0 && (keys[i - 1] >> 33) == (k >> 33);
        if (k != NND_NONE && !dup) {
          const unsigned int id = (unsigned int)(k >> 33);
          const unsigned int low = (unsigned int)k;
          if ((k >> 32) & 1ull) {
            k2[r] = ((unsigned long long)low << 32) | (1u << 31) | id;
          } else {
            k2[r] = ((unsigned long long)nnd_ordered(lval[low]) << 32) |
                    ((unsigned int)lflag[low] << 31) | id;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; r++)
      if (t + r * NND_BLOCK < P) keys[t + r * NND_BLOCK] = k2[r];
    nnd_bitonic<true>(keys, P);

    if (t < K) {
      const unsigned long long k = t < P ? keys[t] : NND_NONE;
      const bool ok = k != NND_NONE;
      lval[t] = ok ? nnd_value((unsigned int)(k >> 32)) : INFINITY;
      lid[t] = ok ? (int)((unsigned int)k & 0x7fffffffu) : -1;
      lflag[t] = ok && (((unsigned int)k >> 31) != 0);
    }
    __syncthreads();
  }

  const bool now = t < K && lid[t] >= 0 && lflag[t] != 0;
  const int after = __syncthreads_count(now);
  if (t < K) {
    vals[u * K + t] = lval[t];
    ids[u * K + t] = lid[t];
    flags[u * K + t] = lflag[t];
  }
  if (t == 0 && after != before)
    atomicAdd(counter, (unsigned long long)(long long)(after - before));
}

void launch_nn_descent_join(const void* dataset, int dtype, long long n, long long row_pitch,
                            const float* norms, const int* new_ids, const int* old_ids,
                            int* out_target, int* out_id, float* out_val, long long n_nodes, int d,
                            int n_samples, int metric, hipStream_t stream) {
  if (n_nodes <= 0) return;
  if (dtype < 0 || dtype > 2)
    throw std::runtime_error("nn_descent_join: dtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("nn_descent_join: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (n < 1 || n >= 2147483648ll || n_nodes > 2147483647ll || row_pitch < 0)
    throw std::runtime_error("nn_descent_join: serves 1 to 2^31 - 1 rows and nodes");
  if (d < 1 || d > NND_MAX_D || n_samples < 1 || n_samples > NND_MAX_SAMPLES)
    throw std::runtime_error("nn_descent_join: serves 1 <= d <= " + std::to_string(NND_MAX_D) +
                             " and 1 <= n_samples <= " + std::to_string(NND_MAX_SAMPLES));
  const size_t esize = dtype == 0 ? 4 : 2;
  const bool vec = reinterpret_cast<uintptr_t>(dataset) % 16 == 0 &&
                   ((size_t)row_pitch * esize) % 16 == 0;
  const bool ip = metric == 2;
  const dim3 grid((unsigned)n_nodes), block(NND_BLOCK);
  const int S2 = 2 * n_samples;
  if (dtype == 0)
    hipLaunchKernelGGL(nn_descent_join_kernel<NndF32>, grid, block, 0, stream,
                       static_cast<const float*>(dataset), n, row_pitch, norms, new_ids, old_ids,
                       out_target, out_id, out_val, d, S2, vec, ip);
  else if (dtype == 1)
    hipLaunchKernelGGL(nn_descent_join_kernel<NndBF16>, grid, block, 0, stream,
                       static_cast<const unsigned short*>(dataset), n, row_pitch, norms, new_ids,
                       old_ids, out_target, out_id, out_val, d, S2, vec, ip);
  else
    hipLaunchKernelGGL(nn_descent_join_kernel<NndF16>, grid, block, 0, stream,
                       static_cast<const _Float16*>(dataset), n, row_pitch, norms, new_ids,
                       old_ids, out_target, out_id, out_val, d, S2, vec, ip);
  HIP_CHECK(hipGetLastError());
}

void launch_nn_descent_merge(float* vals, int* ids, unsigned char* flags, long long n, int k,
                             const long long* seg_off, const int* cand_id, const float* cand_val,
                             unsigned long long* counter, hipStream_t stream) {
  if (n <= 0) return;
  if (n >= 2147483648ll || k < 1 || k > NND_MAX_K)
    throw std::runtime_error("nn_descent_merge: serves fewer than 2^31 rows and 1 <= k <= " +
                             std::to_string(NND_MAX_K));
  hipLaunchKernelGGL(nn_descent_merge_kernel, dim3((unsigned)n), dim3(NND_BLOCK), 0, stream, vals,
                     ids, flags, n, k, seg_off, cand_id, cand_val, counter);
  HIP_CHECK(hipGetLastError());
}

}  // namespace raft_amd
