// Pairwise L2 kernel selection (pairwise_mfma.hip): the one place that reads
// the RAFT_AMD_PW_*, RAFT_AMD_PW256, RAFT_AMD_FILTER256 and RAFT_AMD_KNN_PX
// tuning variables and holds every variant's shape predicate. Host-only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

namespace raft_amd {

enum class PwFamily {
  Tile,    // pairwise_l2_mfma: writes the distance tile
  Filter,  // pairwise_l2_filter: emits the pairs under a per-row threshold
};

enum class PwVariant {
  Auto,      // "auto": environment overrides, then the measured defaults
  T128,      // "128": 128^2 tile, 4 waves, 2 blocks/CU
  T128Bk32,  // "128_bk32": 128^2 over the BK=32 counted-vmcnt K-loop (Tile)
  T256,      // "256": 256^2 tile, 8 waves, BK=32 counted-vmcnt K-loop
  Px,        // "px": 128-row X panel LDS-resident over 8 col tiles (Filter)
};

const char* pw_variant_name(PwVariant v);
// Auto with *known = false for a name the family does not have
PwVariant pw_variant_from_name(PwFamily family, const std::string& name, bool* known);

struct PwPlan {
  PwVariant variant;  // never Auto
  std::string error;  // non-empty: `requested` cannot run this shape
};

// requested == Auto resolves the environment and the defaults; a named variant
// is checked against its shape predicate and never replaced. Every caller has
// already checked nslice in 1..3 and d % 64 == 0.
PwPlan pw_resolve_variant(PwFamily family, int nslice, long long m, long long n, int d,
                          PwVariant requested);

// run a resolved plan (throws plan.error); ldo = row stride of `out`
void launch_pairwise_l2_tile(const PwPlan& plan, const void** xsl, const void** csl,
                             const float* xn, const float* yn, float* out, long long m,
                             long long n, int d, long long ldo, int nslice,
                             bool sqrt_out, hipStream_t stream);
void launch_pairwise_l2_filter(const PwPlan& plan, const void** xsl, const void** csl,
                               const float* xn, const float* yn, const float* thr,
                               float* out_d, int* out_i, int* cnt, int cap,
                               long long col_offset, long long m, long long n, int d,
                               int nslice, hipStream_t stream);

}  // namespace raft_amd
