// refine: exact re-rank of kNN candidates, gather + distance + select fused.
//
// Reference parity (WHAT): raft::neighbors::refine. For every query the rows
// dataset[candidates[query][*]] are gathered, their exact fp32 distance to the
// query is computed and the k best are returned, best first, ties to the
// smaller id. A repeated candidate id is returned repeatedly. HOW is
// CDNA4-native: neither the gathered rows nor the [q, n_cand] distances reach
// memory.
//
// ---- work split -----------------------------------------------------------
// One block of 256 threads (4 waves) per query, grid x = q. A single query, or
// a handful, therefore occupies that many blocks and no more: accepted, one
// query is never split over blocks.
//
// Dynamic LDS: the query as fp32 [dq], dq = d rounded up to one lane's step
// (4 elements for fp32 rows, 8 for bf16 / fp16 rows; the tail is zero), then
// 64-bit keys [P], P = n_cand rounded up to a power of two, at least 256.
// d <= 8192 and n_cand <= 4096 give at most 32 KiB + 32 KiB = 64 KiB, inside
// the default limit. At d = 128 with a few hundred candidates it is under
// 5 KiB, so the 2048-thread limit of a CU sets occupancy, not LDS.
//
// ---- phase 1: gather and distance -----------------------------------------
// A candidate row is read by a SUB-WAVE of L lanes; a lane takes one 16-byte
// piece of the row per step (4 fp32, or 8 bf16 / fp16 widened in registers;
// the data set is never widened in memory). L is a template tier in
// {8, 16, 32, 64}: the smallest that covers the row in one step, else 64 with
// several steps. The 256 / L sub-waves of a block each keep U candidates in
// flight (U = 4 for L < 64; for L = 64 U = 2 and the step loop is unrolled by
// two), so every lane has four independent row loads outstanding before the
// first is used: the gather is random over whole rows and latency-bound.
//
// The query piece is one 16-byte LDS read per 4 floats: lanes of different
// sub-waves read the same address (a broadcast), lanes of one sub-wave read
// consecutive 16 bytes, so a ds_read_b128 of a wave touches every bank equally
// often and needs no padding. Partial sums are reduced over the L lanes by an
// xor butterfly (log2 L steps); lane 0 of the sub-wave writes the key.
//
// Template axis VECTOR: the 16-byte global load needs a 16-byte aligned base,
// a row pitch that is a multiple of 16 bytes and d a multiple of the step.
// Everything else takes the element-wise path, which loads the SAME elements
// of the same lane with guarded scalar loads. Both paths therefore add in the
// same order, and a result does not depend on stride or alignment.
//
// L2 is the unexpanded fp32 sum fma(x - q, x - q, acc), inner product is
// fma(x, q, acc); elements past d are 0 on both sides and add exactly 0. The
// square root of euclidean is a runtime flag applied to the k results only.
//
// An id outside [0, n) is not a candidate: it is checked before an address is
// formed and never dereferenced.
//
// ---- phase 2: select -------------------------------------------------------
// key = (ordered distance bits << 32) | uint32(id). "Ordered" is the sign-flip
// transform of the fp32 bits (ascending as unsigned); for inner product the
// bits are complemented, so one ascending sort serves both directions and ties
// still go to the smaller id. A NaN distance is replaced by +inf (-inf for
// inner product) before the key is made and keeps its id. Invalid candidates
// and pad slots are all-ones, which no valid key equals since n < 2^32 - 1.
// A block-wide bitonic sort of the P keys runs in LDS, every stage behind a
// block barrier (stages inside one wave's span could drop it; they do not, so
// nothing relies on wave lockstep). Partners are `stride` keys apart: for
// stride >= 32 a wave's 64-bit reads are consecutive, for smaller strides the
// lanes skip every other run of `stride` keys, which at worst doubles the LDS
// passes of that stage. Threads then decode the first k keys straight into
// dists / ids: inverse transform, square root if asked, (bad, -1) for the
// sentinel.
//
// Every early exit would have to be block-uniform and ahead of the first
// barrier; there is none: a block always runs both phases.
//
// The tiers, unroll factors and bank reasoning above are REASONED from the
// layout. Measured: register and scratch use per instantiation and the timings
// of docs/performance.md, "refine"; no PMC run has been taken.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

constexpr int REFINE_BLOCK = 256;
constexpr int REFINE_MAX_D = 8192;
constexpr int REFINE_MAX_CAND = 4096;
constexpr int REFINE_MIN_KEYS = 256;
constexpr unsigned long long REFINE_SENTINEL = ~0ull;

// element types: how 16 bytes of a row widen to fp32
struct RefineF32 {
  using raw = float;
  static constexpr int VEC = 4;
  __device__ __forceinline__ static float widen(raw v) { return v; }
};
struct RefineBF16 {
  using raw = unsigned short;
  static constexpr int VEC = 8;
  __device__ __forceinline__ static float widen(raw v) {
    return __uint_as_float((unsigned int)v << 16);
  }
};
struct RefineF16 {
  using raw = _Float16;
  static constexpr int VEC = 8;
  __device__ __forceinline__ static float widen(raw v) { return (float)v; }
};

// piece s (E::VEC elements) of row id; `live` false gives zeros and reads nothing
template <typename E, bool VECTOR>
__device__ __forceinline__ void refine_load(typename E::raw (&x)[E::VEC],
                                            const typename E::raw* __restrict__ data,
                                            long long id, long long pitch, int s, int d,
                                            bool live) {
  using raw = typename E::raw;
  if constexpr (VECTOR) {
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (live) w = *reinterpret_cast<const uint4*>(data + id * pitch + (long long)s * E::VEC);
    __builtin_memcpy(x, &w, sizeof(w));
  } else {
#pragma unroll
    for (int e = 0; e < E::VEC; e++) {
      const int f = s * E::VEC + e;
      x[e] = (raw)0;
      if (live && f < d) x[e] = data[id * pitch + f];
    }
  }
}

template <bool IP>
__device__ __forceinline__ unsigned long long refine_key(float v, long long id, bool ok) {
  if (!ok) return REFINE_SENTINEL;
  if (v != v) v = IP ? -INFINITY : INFINITY;
  unsigned int b = __float_as_uint(v);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if constexpr (IP) b = ~b;
  return ((unsigned long long)b << 32) | (unsigned int)id;
}

template <typename E, int L, bool VECTOR, bool IP>
__launch_bounds__(REFINE_BLOCK)
__global__ void refine_kernel(const typename E::raw* __restrict__ data, long long n,
                              long long pitch, const float* __restrict__ queries,
                              const long long* __restrict__ cand, float* __restrict__ dists,
                              long long* __restrict__ ids, int d, int n_cand, int P, int k,
                              bool sqrt_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char refine_lds[];
  constexpr int V = E::VEC;
  constexpr int NS = REFINE_BLOCK / L;      // sub-waves of a block
  constexpr int U = L == 64 ? 2 : 4;        // candidates a sub-wave has in flight
  constexpr int SU = L == 64 ? 2 : 1;       // steps in flight per candidate
  const int t = threadIdx.x;
  const int chunks = (d + V - 1) / V;
  const int dq = chunks * V;
  float* qs = reinterpret_cast<float*>(refine_lds);                              // [dq]
  unsigned long long* keys =
      reinterpret_cast<unsigned long long*>(refine_lds + (size_t)dq * sizeof(float));  // [P]

  const long long qrow = blockIdx.x;
  const float* qp = queries + qrow * d;
  for (int i = t; i < dq; i += REFINE_BLOCK) qs[i] = i < d ? qp[i] : 0.f;
  for (int i = n_cand + t; i < P; i += REFINE_BLOCK) keys[i] = REFINE_SENTINEL;
  __syncthreads();

  // phase 1: the trip counts of both loops are block-uniform
  const int sub = t / L, sl = t % L;
  const long long* crow = cand + qrow * n_cand;
  for (int c0 = 0; c0 < n_cand; c0 += NS * U) {
    long long id[U];
    bool ok[U];
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int c = c0 + u * NS + sub;
      id[u] = c < n_cand ? crow[c] : -1;
      ok[u] = id[u] >= 0 && id[u] < n;
      acc[u] = 0.f;
    }
    for (int s0 = sl; s0 < chunks; s0 += L * SU) {
      typename E::raw x[SU][U][V];
#pragma unroll
      for (int j = 0; j < SU; j++)
#pragma unroll
        for (int u = 0; u < U; u++)
          refine_load<E, VECTOR>(x[j][u], data, id[u], pitch, s0 + j * L, d,
                                 ok[u] && s0 + j * L < chunks);
#pragma unroll
      for (int j = 0; j < SU; j++) {
        const int s = s0 + j * L;
        if (s < chunks) {
          float qv[V];
#pragma unroll
          for (int e = 0; e < V; e += 4) {
            const float4 q4 = *reinterpret_cast<const float4*>(qs + s * V + e);
            qv[e] = q4.x, qv[e + 1] = q4.y, qv[e + 2] = q4.z, qv[e + 3] = q4.w;
          }
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int e = 0; e < V; e++) {
              const float xv = E::widen(x[j][u][e]);
              if constexpr (IP) {
                acc[u] = fmaf(xv, qv[e], acc[u]);
              } else {
                const float diff = xv - qv[e];
                acc[u] = fmaf(diff, diff, acc[u]);
              }
            }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
      for (int off = L >> 1; off > 0; off >>= 1)
        acc[u] += __shfl_xor(acc[u], off, RAFT_AMD_WAVE);
      const int c = c0 + u * NS + sub;
      if (sl == 0 && c < n_cand) keys[c] = refine_key<IP>(acc[u], id[u], ok[u]);
    }
  }

  // phase 2: ascending bitonic sort of keys[0 .. P)
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = t; i < (P >> 1); i += REFINE_BLOCK) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((a > b) == up) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
    }
  }
  __syncthreads();

  const float bad = IP ? -INFINITY : INFINITY;
  for (int j = t; j < k; j += REFINE_BLOCK) {
    const unsigned long long key = j < P ? keys[j] : REFINE_SENTINEL;
    float v = bad;
    long long id = -1;
    if (key != REFINE_SENTINEL) {
      unsigned int b = (unsigned int)(key >> 32);
      if constexpr (IP) b = ~b;
      b = (b & 0x80000000u) ? (b ^ 0x80000000u) : ~b;
      v = __uint_as_float(b);
      if (sqrt_out) v = sqrtf(v);
      id = (long long)(unsigned int)key;
    }
    dists[qrow * k + j] = v;
    ids[qrow * k + j] = id;
  }
}

int refine_key_slots(int n_cand) {
  int p = REFINE_MIN_KEYS;
  while (p < n_cand) p <<= 1;
  return p;
}

namespace {

struct RefineArgs {
  const void* data;
  long long n, pitch;
  const float* queries;
  const long long* cand;
  float* dists;
  long long* ids;
  long long n_queries;
  int d, n_cand, P, k;
  bool ip, sqrt_out;
  size_t lds;
  hipStream_t stream;
};

template <typename E, int L, bool VECTOR, bool IP>
void refine_launch(const RefineArgs& a) {
  hipLaunchKernelGGL((refine_kernel<E, L, VECTOR, IP>), dim3((unsigned)a.n_queries),
                     dim3(REFINE_BLOCK), a.lds, a.stream,
                     static_cast<const typename E::raw*>(a.data), a.n, a.pitch, a.queries,
                     a.cand, a.dists, a.ids, a.d, a.n_cand, a.P, a.k, a.sqrt_out);
}

template <typename E, int L>
void refine_pick_path(const RefineArgs& a, bool vector) {
  if (vector) {
    if (a.ip) refine_launch<E, L, true, true>(a);
    else refine_launch<E, L, true, false>(a);
  } else {
    if (a.ip) refine_launch<E, L, false, true>(a);
    else refine_launch<E, L, false, false>(a);
  }
}

template <typename E>
void refine_pick_tier(RefineArgs a) {
  const int chunks = (a.d + E::VEC - 1) / E::VEC;
  a.lds = (size_t)chunks * E::VEC * sizeof(float) + (size_t)a.P * sizeof(unsigned long long);
  const size_t row_bytes = (size_t)a.pitch * sizeof(typename E::raw);
  const bool vector = a.d % E::VEC == 0 && reinterpret_cast<uintptr_t>(a.data) % 16 == 0 &&
                      row_bytes % 16 == 0;
  if (chunks <= 8) refine_pick_path<E, 8>(a, vector);
  else if (chunks <= 16) refine_pick_path<E, 16>(a, vector);
  else if (chunks <= 32) refine_pick_path<E, 32>(a, vector);
  else refine_pick_path<E, 64>(a, vector);
}

}  // namespace

void launch_refine(const void* dataset, int dtype, long long n, long long row_pitch,
                   const float* queries, const long long* candidates, float* dists,
                   long long* ids, long long n_queries, int d, int n_cand, int k, int metric,
                   hipStream_t stream) {
  if (n_queries <= 0 || n_cand <= 0) return;
  if (dtype < 0 || dtype > 2)
    throw std::runtime_error("refine: dtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("refine: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (n < 0 || n >= 4294967295ll)
    throw std::runtime_error("refine: the data set must have fewer than 2^32 - 1 rows");
  if (row_pitch < 0) throw std::runtime_error("refine: negative row pitch");
  if (d < 1 || d > REFINE_MAX_D || n_cand > REFINE_MAX_CAND)
    throw std::runtime_error("refine: serves 1 <= d <= " + std::to_string(REFINE_MAX_D) +
                             " and n_cand <= " + std::to_string(REFINE_MAX_CAND));
  const int P = refine_key_slots(n_cand);
  if (k < 1 || k > P)
    throw std::runtime_error("refine: k must be in [1, " + std::to_string(P) + "]");
  if (n_queries > 2147483647ll) throw std::runtime_error("refine: grid out of range");
  RefineArgs a{dataset, n, row_pitch, queries, candidates, dists, ids, n_queries,
               d, n_cand, P, k, metric == 2, metric == 1, 0, stream};
  if (dtype == 0) refine_pick_tier<RefineF32>(a);
  else if (dtype == 1) refine_pick_tier<RefineBF16>(a);
  else refine_pick_tier<RefineF16>(a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace raft_amd
