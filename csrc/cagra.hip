// cagra: greedy graph search (one block per query) and detour-count pruning
// (one block per node).
//
// Reference parity (WHAT): cuvs::neighbors::cagra search (the single-CTA
// algorithm) and the first half of cagra::optimize. raft_amd/neighbors/cagra.py
// holds the definition of both in plain torch; these kernels reproduce it. HOW
// is CDNA4-native.
//
// ==== cagra_search ==========================================================
// One block of 256 threads (4 waves) per query, grid x = q. A handful of
// queries fills a handful of blocks: accepted, a query is never split.
//
// ---- LDS (dynamic, sized from the actual parameters, <= 64 KiB) ------------
//   qs      fp32 [dq]   the query, dq = d rounded up to one lane's step
//   keys    u64  [P]    P = pow2 >= itopk + CP, CP = pow2 >= max(C, S)
//                       [0, itopk)    the list, ascending
//                       [itopk, P-CP) all-ones
//                       [P-CP, P)     this round's candidate keys
//   table   u32  [H]    visited ids, open addressing, all-ones = empty
//   cid     i32  [CP]   this round's candidate ids, -1 = dropped
//   parents i32  [w], then the parent count
// d <= 4096, itopk <= 512, C = w * graph_degree <= 512, S <= 512, H <= 8192:
// 16 + 8 + 32 + 2 KiB and a few words.
//
// ---- key --------------------------------------------------------------------
// (ordered distance bits << 32) | (id << 1) | expanded. "Ordered" is refine's
// sign-flip transform, complemented for inner product, NaN replaced by the
// metric's bad value first. Ids in the list and the batch are distinct, so the
// expanded flag in bit 0 never decides an order; n < 2^31 keeps id << 1 in 32
// bits. All-ones is "no entry" and reads as expanded.
//
// ---- one round ---------------------------------------------------------------
// 1. candidate ids: round 0 the seeds, later the graph rows of the parents,
//    read coalesced (16 bytes per lane where graph_degree % 4 == 0).
// 2. `count` bounds the ids in the table (every batch is counted whole, so it
//    is block-uniform without a reduction). If count + batch > H / 2 the table
//    is cleared, the list's ids are re-inserted and count = itopk. A row
//    outside the list can then be computed again; its key is above the list's
//    worst, so the list does not change.
// 3. one thread per candidate: the range check, then an LDS atomicCAS insert.
//    An id found in the table (visited, or a repeat within the batch: which
//    lane wins does not matter) becomes -1.
// 4. gather as in refine.hip: a sub-wave of SW in {8, 16, 32, 64} lanes per row,
//    one 16-byte load per lane and step, fp32 / bf16 / fp16 widened in
//    registers, U rows in flight per sub-wave (the chain graph row -> vector
//    row -> sort -> parent is latency-bound), an element-wise path with the
//    same per-lane order for a misaligned base, pitch or d, xor butterfly.
// 5. bitonic sort of the CP candidate keys, descending.
// 6. keys[0, P) is now ascending | all-ones | descending, a bitonic sequence:
//    ONE bitonic merge of log2(P) steps leaves the itopk best in front.
// 7. wave 0 scans the list for the first w unexpanded entries by ballot and
//    prefix popcount, flags them and writes their ids as parents.
// The loop ends when no parent was found or after max_iterations rounds; both
// are block-uniform. The epilogue decodes the first k keys into dists / ids.
// No host sync, no global atomics, no scratch in device memory.
//
// ==== cagra_prune ===========================================================
// One block per node A, kd <= 256. LDS: A's row, an id -> rank table of
// 4 * pow2(kd) slots (load <= 1/4), kd detour counters, pow2(kd) sort keys.
// Waves take the neighbours B round-robin, read B's row coalesced, probe the
// table for every D and on a hit with kAB < kAD and kBD < kAD add one to
// detour[kAD] with an LDS atomic. Keys (detour << 16) | rank (detour <=
// 255^2 < 2^16), absent entries all-ones, are bitonic-sorted; the first g
// ranks are written as ids.
//
// All of the above is REASONED from the layout; see docs/performance.md,
// "CAGRA", for what has been measured.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

constexpr int CAGRA_BLOCK = 256;
constexpr int CAGRA_MAX_D = 4096;
constexpr int CAGRA_MAX_ITOPK = 512;
constexpr int CAGRA_MAX_CAND = 512;
constexpr int CAGRA_MAX_HASH = 8192;
constexpr int CAGRA_MAX_KD = 256;
constexpr unsigned long long CAGRA_NO_KEY = ~0ull;
constexpr unsigned int CAGRA_EMPTY = ~0u;

struct CagraF32 {
  using raw = float;
  static constexpr int VEC = 4;
  __device__ __forceinline__ static float widen(raw v) { return v; }
};
struct CagraBF16 {
  using raw = unsigned short;
  static constexpr int VEC = 8;
  __device__ __forceinline__ static float widen(raw v) {
    return __uint_as_float((unsigned int)v << 16);
  }
};
struct CagraF16 {
  using raw = _Float16;
  static constexpr int VEC = 8;
  __device__ __forceinline__ static float widen(raw v) { return (float)v; }
};

// piece s (E::VEC elements) of row id; `live` false gives zeros and reads nothing
template <typename E, bool VECTOR>
__device__ __forceinline__ void cagra_load(typename E::raw (&x)[E::VEC],
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
__device__ __forceinline__ unsigned long long cagra_key(float v, int id, bool ok) {
  if (!ok) return CAGRA_NO_KEY;
  if (v != v) v = IP ? -INFINITY : INFINITY;
  unsigned int b = __float_as_uint(v);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if constexpr (IP) b = ~b;
  return ((unsigned long long)b << 32) | ((unsigned int)id << 1);
}

__device__ __forceinline__ unsigned int cagra_hash(unsigned int id, int shift) {
  return (id * 0x9E3779B1u) >> shift;
}

// true when id was not in the table (and now is). The load stays at or below
// 1/2, so an empty slot is always met; the trip bound only guards the loop.
__device__ __forceinline__ bool cagra_visit(unsigned int* table, int H, int shift,
                                            unsigned int id) {
  unsigned int s = cagra_hash(id, shift);
  for (int trip = 0; trip < H; trip++) {
    const unsigned int old = atomicCAS(&table[s], CAGRA_EMPTY, id);
    if (old == CAGRA_EMPTY) return true;
    if (old == id) return false;
    s = (s + 1) & (unsigned int)(H - 1);
  }
  return false;
}

// one compare-exchange step of a bitonic network over a[0, m), m a power of two
template <typename K>
__device__ __forceinline__ void cagra_bitonic_step(K* a, int m, int size, int stride, bool desc,
                                                   int t) {
  for (int i = t; i < (m >> 1); i += CAGRA_BLOCK) {
    const int lo = 2 * i - (i & (stride - 1));
    const int hi = lo + stride;
    const bool up = ((lo & size) == 0) != desc;
    const K x = a[lo], y = a[hi];
    if ((x > y) == up) {
      a[lo] = y;
      a[hi] = x;
    }
  }
}

// full sort of a[0, m); a barrier stands before every step and after the last
template <typename K>
__device__ __forceinline__ void cagra_bitonic_sort(K* a, int m, bool desc, int t) {
  for (int size = 2; size <= m; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      cagra_bitonic_step(a, m, size, stride, desc, t);
    }
  __syncthreads();
}

// distances of cid[0, batch) into cand[0, batch); the trip counts are block-uniform
template <typename E, int SW, bool VECTOR, bool IP>
__device__ __forceinline__ void cagra_gather(const typename E::raw* __restrict__ data, int n,
                                             long long pitch, const float* qs, const int* cid,
                                             unsigned long long* cand, int batch, int d,
                                             int chunks, int t) {
  constexpr int V = E::VEC;
  constexpr int NS = CAGRA_BLOCK / SW;      // sub-waves of a block
  constexpr int U = SW == 64 ? 2 : 4;       // rows a sub-wave has in flight
  constexpr int SU = SW == 64 ? 2 : 1;      // steps in flight per row
  const int sub = t / SW, sl = t % SW;
  for (int c0 = 0; c0 < batch; c0 += NS * U) {
    int id[U];
    bool ok[U];
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int c = c0 + u * NS + sub;
      id[u] = c < batch ? cid[c] : -1;
      ok[u] = id[u] >= 0 && id[u] < n;
      acc[u] = 0.f;
    }
    for (int s0 = sl; s0 < chunks; s0 += SW * SU) {
      typename E::raw x[SU][U][V];
#pragma unroll
      for (int j = 0; j < SU; j++)
#pragma unroll
        for (int u = 0; u < U; u++)
          cagra_load<E, VECTOR>(x[j][u], data, id[u], pitch, s0 + j * SW, d,
                                ok[u] && s0 + j * SW < chunks);
#pragma unroll
      for (int j = 0; j < SU; j++) {
        const int s = s0 + j * SW;
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
      for (int off = SW >> 1; off > 0; off >>= 1)
        acc[u] += __shfl_xor(acc[u], off, RAFT_AMD_WAVE);
      const int c = c0 + u * NS + sub;
      if (sl == 0 && c < batch) cand[c] = cagra_key<IP>(acc[u], id[u], ok[u]);
    }
  }
}

struct CagraSearchShape {
  int d, itopk, width, degree, n_seeds, max_it, P, CP, H, hash_shift, k;
  bool sqrt_out, graph_vec;
};

template <typename E, int SW, bool VECTOR, bool IP>
__launch_bounds__(CAGRA_BLOCK)
__global__ void cagra_search_kernel(const typename E::raw* __restrict__ data, int n,
                                    long long pitch, const int* __restrict__ graph,
                                    const float* __restrict__ queries,
                                    const int* __restrict__ seeds, long long seed_pitch,
                                    float* __restrict__ dists, long long* __restrict__ ids,
                                    CagraSearchShape sh) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cagra_lds[];
  constexpr int V = E::VEC;
  const int t = threadIdx.x;
  const int d = sh.d, itopk = sh.itopk, g = sh.degree, P = sh.P, CP = sh.CP, H = sh.H;
  const int chunks = (d + V - 1) / V;
  const int dq = chunks * V;
  float* qs = reinterpret_cast<float*>(cagra_lds);                                    // [dq]
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(qs + dq);         // [P]
  unsigned int* table = reinterpret_cast<unsigned int*>(keys + P);                    // [H]
  int* cid = reinterpret_cast<int*>(table + H);                                       // [CP]
  int* parents = cid + CP;                                                            // [w] + 1
  unsigned long long* cand = keys + (P - CP);

  const long long qrow = blockIdx.x;
  const float* qp = queries + qrow * d;
  for (int i = t; i < dq; i += CAGRA_BLOCK) qs[i] = i < d ? qp[i] : 0.f;
  for (int i = t; i < P - CP; i += CAGRA_BLOCK) keys[i] = CAGRA_NO_KEY;
  for (int i = t; i < H; i += CAGRA_BLOCK) table[i] = CAGRA_EMPTY;

  int count = 0;              // bound of the ids in the table, block-uniform
  int batch = sh.n_seeds;     // candidates of this round, block-uniform
  const int* srow = seeds + qrow * seed_pitch;
  for (int c = t; c < batch; c += CAGRA_BLOCK) cid[c] = srow[c];
  __syncthreads();

  for (int it = 0; it < sh.max_it; it++) {
    // 2. keep the table at or below half full
    if (count + batch > (H >> 1)) {
      for (int i = t; i < H; i += CAGRA_BLOCK) table[i] = CAGRA_EMPTY;
      __syncthreads();
      for (int i = t; i < itopk; i += CAGRA_BLOCK) {
        const unsigned long long key = keys[i];
        if (key != CAGRA_NO_KEY) cagra_visit(table, H, sh.hash_shift, (unsigned int)key >> 1);
      }
      count = itopk;
      __syncthreads();
    }
    count += batch;
    // 3. range check, then visited / repeat check
    for (int c = t; c < batch; c += CAGRA_BLOCK) {
      const int id = cid[c];
      const bool fresh = id >= 0 && id < n && cagra_visit(table, H, sh.hash_shift, (unsigned int)id);
      if (!fresh) cid[c] = -1;
    }
    for (int c = batch + t; c < CP; c += CAGRA_BLOCK) cand[c] = CAGRA_NO_KEY;
    __syncthreads();
    // 4. distances of the survivors
    cagra_gather<E, SW, VECTOR, IP>(data, n, pitch, qs, cid, cand, batch, d, chunks, t);
    // 5. candidates descending (the sort opens with a barrier)
    cagra_bitonic_sort(cand, CP, true, t);
    // 6. ascending | all-ones | descending: one merge
    for (int stride = P >> 1; stride > 0; stride >>= 1) {
      cagra_bitonic_step(keys, P, P, stride, false, t);
      __syncthreads();
    }
    for (int i = itopk + t; i < P - CP; i += CAGRA_BLOCK) keys[i] = CAGRA_NO_KEY;
    // 7. the first w unexpanded entries become parents
    if (t < RAFT_AMD_WAVE) {
      int found = 0;
      for (int base = 0; base < itopk && found < sh.width; base += RAFT_AMD_WAVE) {
        const int i = base + t;
        const unsigned long long key = i < itopk ? keys[i] : CAGRA_NO_KEY;
        const bool open = (key & 1ull) == 0;
        const unsigned long long mask = __ballot(open);
        const int at = found + __popcll(mask & ((1ull << t) - 1ull));
        if (open && at < sh.width) {
          parents[at] = (int)((unsigned int)key >> 1);
          keys[i] = key | 1ull;
        }
        found += __popcll(mask);
      }
      if (t == 0) parents[sh.width] = found < sh.width ? found : sh.width;
    }
    __syncthreads();
    const int np = parents[sh.width];
    if (np == 0 || it + 1 == sh.max_it) break;
    // 1. the graph rows of the parents
    batch = np * g;
    if (sh.graph_vec) {
      for (int c = 4 * t; c < batch; c += 4 * CAGRA_BLOCK) {
        const int j = c / g;
        *reinterpret_cast<int4*>(cid + c) =
            *reinterpret_cast<const int4*>(graph + (long long)parents[j] * g + (c - j * g));
      }
    } else {
      for (int c = t; c < batch; c += CAGRA_BLOCK) {
        const int j = c / g;
        cid[c] = graph[(long long)parents[j] * g + (c - j * g)];
      }
    }
    __syncthreads();
  }
  __syncthreads();

  const float bad = IP ? -INFINITY : INFINITY;
  for (int j = t; j < sh.k; j += CAGRA_BLOCK) {
    const unsigned long long key = keys[j];
    float v = bad;
    long long id = -1;
    if (key != CAGRA_NO_KEY) {
      unsigned int b = (unsigned int)(key >> 32);
      if constexpr (IP) b = ~b;
      b = (b & 0x80000000u) ? (b ^ 0x80000000u) : ~b;
      v = __uint_as_float(b);
      // fp64 root rounded once to fp32: correctly rounded, equal to the host's
      if (sh.sqrt_out) v = (float)sqrt((double)v);
      id = (long long)((unsigned int)key >> 1);
    }
    dists[qrow * sh.k + j] = v;
    ids[qrow * sh.k + j] = id;
  }
}

// ---- prune -------------------------------------------------------------------

__launch_bounds__(CAGRA_BLOCK)
__global__ void cagra_prune_kernel(const int* __restrict__ graph, int* __restrict__ out, int n,
                                   int kd, int g, int T, int shift, int KP) {
  __shared__ int row[CAGRA_MAX_KD];
  __shared__ int detour[CAGRA_MAX_KD];
  __shared__ unsigned int keys[CAGRA_MAX_KD];
  __shared__ unsigned int slot_id[4 * CAGRA_MAX_KD];
  __shared__ int slot_rank[4 * CAGRA_MAX_KD];
  const int t = threadIdx.x;
  const long long a = blockIdx.x;
  if (t < kd) {
    const int v = graph[a * kd + t];
    row[t] = v >= 0 && v < n ? v : -1;
    detour[t] = 0;
  }
  for (int i = t; i < T; i += CAGRA_BLOCK) {
    slot_id[i] = CAGRA_EMPTY;
    slot_rank[i] = CAGRA_MAX_KD;
  }
  __syncthreads();
  // id -> rank; a repeated id (outside the contract) keeps its smallest rank
  if (t < kd && row[t] >= 0) {
    const unsigned int id = (unsigned int)row[t];
    unsigned int s = cagra_hash(id, shift);
    for (int trip = 0; trip < T; trip++) {
      const unsigned int old = atomicCAS(&slot_id[s], CAGRA_EMPTY, id);
      if (old == CAGRA_EMPTY || old == id) {
        atomicMin(&slot_rank[s], t);
        break;
      }
      s = (s + 1) & (unsigned int)(T - 1);
    }
  }
  __syncthreads();
  const int wave = t / RAFT_AMD_WAVE, lane = t % RAFT_AMD_WAVE;
  for (int k_ab = wave; k_ab < kd; k_ab += CAGRA_BLOCK / RAFT_AMD_WAVE) {
    const int b = row[k_ab];
    if (b < 0) continue;
    for (int k_bd = lane; k_bd < kd; k_bd += RAFT_AMD_WAVE) {
      const int dn = graph[(long long)b * kd + k_bd];
      if (dn < 0 || dn >= n) continue;
      unsigned int s = cagra_hash((unsigned int)dn, shift);
      for (int trip = 0; trip < T; trip++) {
        const unsigned int v = slot_id[s];
        if (v == CAGRA_EMPTY) break;
        if (v == (unsigned int)dn) {
          const int k_ad = slot_rank[s];
          if (k_ab < k_ad && k_bd < k_ad) atomicAdd(&detour[k_ad], 1);
          break;
        }
        s = (s + 1) & (unsigned int)(T - 1);
      }
    }
  }
  __syncthreads();
  if (t < KP)
    keys[t] = t < kd && row[t] >= 0 ? ((unsigned int)detour[t] << 16) | (unsigned int)t
                                    : CAGRA_EMPTY;
  cagra_bitonic_sort(keys, KP, false, t);
  if (t < g) {
    const unsigned int key = keys[t];
    out[a * g + t] = key == CAGRA_EMPTY ? -1 : row[key & 0xffffu];
  }
}

// ---- launchers ---------------------------------------------------------------

namespace {

int cagra_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

int cagra_log2(int p) {
  int l = 0;
  while ((1 << l) < p) l++;
  return l;
}

}  // namespace

int cagra_search_key_slots(int itopk, int n_candidates, int n_seeds) {
  return cagra_pow2(itopk + cagra_pow2(n_candidates > n_seeds ? n_candidates : n_seeds));
}

size_t cagra_search_lds_bytes(int d, int vec, int itopk, int n_candidates, int n_seeds,
                              int hash_slots, int search_width) {
  const int cp = cagra_pow2(n_candidates > n_seeds ? n_candidates : n_seeds);
  const size_t dq = (size_t)((d + vec - 1) / vec) * vec;
  return dq * sizeof(float) +
         (size_t)cagra_search_key_slots(itopk, n_candidates, n_seeds) * sizeof(unsigned long long) +
         (size_t)hash_slots * sizeof(unsigned int) + (size_t)cp * sizeof(int) +
         (size_t)(search_width + 1) * sizeof(int);
}

namespace {

struct CagraSearchArgs {
  const void* data;
  int n;
  long long pitch;
  const int* graph;
  const float* queries;
  const int* seeds;
  long long seed_pitch;
  float* dists;
  long long* ids;
  long long n_queries;
  CagraSearchShape sh;
  bool ip;
  hipStream_t stream;
};

template <typename E, int SW, bool VECTOR, bool IP>
void cagra_search_launch(const CagraSearchArgs& a, size_t lds) {
  hipLaunchKernelGGL((cagra_search_kernel<E, SW, VECTOR, IP>), dim3((unsigned)a.n_queries),
                     dim3(CAGRA_BLOCK), lds, a.stream,
                     static_cast<const typename E::raw*>(a.data), a.n, a.pitch, a.graph,
                     a.queries, a.seeds, a.seed_pitch, a.dists, a.ids, a.sh);
}

template <typename E, int SW>
void cagra_search_pick_path(const CagraSearchArgs& a, size_t lds, bool vector) {
  if (vector) {
    if (a.ip) cagra_search_launch<E, SW, true, true>(a, lds);
    else cagra_search_launch<E, SW, true, false>(a, lds);
  } else {
    if (a.ip) cagra_search_launch<E, SW, false, true>(a, lds);
    else cagra_search_launch<E, SW, false, false>(a, lds);
  }
}

template <typename E>
void cagra_search_pick_tier(const CagraSearchArgs& a) {
  const int chunks = (a.sh.d + E::VEC - 1) / E::VEC;
  const size_t lds = cagra_search_lds_bytes(a.sh.d, E::VEC, a.sh.itopk,
                                            a.sh.width * a.sh.degree, a.sh.n_seeds, a.sh.H,
                                            a.sh.width);
  if (lds > 65536) throw std::runtime_error("cagra_search: more than 64 KiB of LDS");
  const size_t row_bytes = (size_t)a.pitch * sizeof(typename E::raw);
  const bool vector = a.sh.d % E::VEC == 0 && reinterpret_cast<uintptr_t>(a.data) % 16 == 0 &&
                      row_bytes % 16 == 0;
  if (chunks <= 8) cagra_search_pick_path<E, 8>(a, lds, vector);
  else if (chunks <= 16) cagra_search_pick_path<E, 16>(a, lds, vector);
  else if (chunks <= 32) cagra_search_pick_path<E, 32>(a, lds, vector);
  else cagra_search_pick_path<E, 64>(a, lds, vector);
}

}  // namespace

void launch_cagra_search(const void* dataset, int dtype, long long n, long long row_pitch,
                         const int* graph, int graph_degree, const float* queries,
                         const int* seeds, long long seed_pitch, int n_seeds, float* dists,
                         long long* ids, long long n_queries, int d, int k, int itopk_size,
                         int search_width, int max_iterations, int hash_slots, int metric,
                         hipStream_t stream) {
  if (n_queries <= 0) return;
  if (dtype < 0 || dtype > 2)
    throw std::runtime_error("cagra_search: dtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("cagra_search: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (n < 1 || n >= 2147483648ll)
    throw std::runtime_error("cagra_search: the data set must have 1 to 2^31 - 1 rows");
  if (row_pitch < 0 || seed_pitch < 0) throw std::runtime_error("cagra_search: negative pitch");
  if (d < 1 || d > CAGRA_MAX_D || itopk_size < 1 || itopk_size > CAGRA_MAX_ITOPK ||
      search_width < 1 || graph_degree < 1 ||
      (long long)search_width * graph_degree > CAGRA_MAX_CAND || n_seeds < 1 ||
      n_seeds > CAGRA_MAX_CAND || k < 1 || k > itopk_size || max_iterations < 1)
    throw std::runtime_error(
        "cagra_search: serves 1 <= d <= 4096, itopk_size <= 512, search_width * graph_degree "
        "<= 512, 1 <= n_seeds <= 512, 1 <= k <= itopk_size and max_iterations >= 1");
  const int C = search_width * graph_degree;
  const int widest = C > n_seeds ? C : n_seeds;
  if (hash_slots < 2 * (itopk_size + widest) || hash_slots > CAGRA_MAX_HASH ||
      (hash_slots & (hash_slots - 1)))
    throw std::runtime_error("cagra_search: hash_slots must be a power of two in [2 * "
                             "(itopk_size + max(candidates, n_seeds)), 8192]");
  if (n_queries > 2147483647ll) throw std::runtime_error("cagra_search: grid out of range");
  CagraSearchShape sh;
  sh.d = d, sh.itopk = itopk_size, sh.width = search_width, sh.degree = graph_degree;
  sh.n_seeds = n_seeds, sh.max_it = max_iterations;
  sh.CP = cagra_pow2(widest);
  sh.P = cagra_search_key_slots(itopk_size, C, n_seeds);
  sh.H = hash_slots, sh.hash_shift = 32 - cagra_log2(hash_slots), sh.k = k;
  sh.sqrt_out = metric == 1;
  sh.graph_vec = graph_degree % 4 == 0 && reinterpret_cast<uintptr_t>(graph) % 16 == 0;
  CagraSearchArgs a{dataset, (int)n, row_pitch, graph, queries, seeds, seed_pitch, dists, ids,
                    n_queries, sh, metric == 2, stream};
  if (dtype == 0) cagra_search_pick_tier<CagraF32>(a);
  else if (dtype == 1) cagra_search_pick_tier<CagraBF16>(a);
  else cagra_search_pick_tier<CagraF16>(a);
  HIP_CHECK(hipGetLastError());
}

void launch_cagra_prune(const int* knn_graph, int* pruned, long long n, int kd, int graph_degree,
                        hipStream_t stream) {
  if (n <= 0) return;
  if (n >= 2147483648ll) throw std::runtime_error("cagra_prune: needs fewer than 2^31 rows");
  if (kd < 1 || kd > CAGRA_MAX_KD || graph_degree < 1 || graph_degree > kd)
    throw std::runtime_error("cagra_prune: serves 1 <= graph_degree <= kd <= 256");
  const int KP = cagra_pow2(kd);
  const int T = 4 * KP;
  hipLaunchKernelGGL(cagra_prune_kernel, dim3((unsigned)n), dim3(CAGRA_BLOCK), 0, stream,
                     knn_graph, pruned, (int)n, kd, graph_degree, T, 32 - cagra_log2(T), KP);
  HIP_CHECK(hipGetLastError());
}

}  // namespace raft_amd
