// Fused L2-NN engine selection (l2nn_engine.h) and the public launchers of
// include/raft_amd/neighbors.hpp, which are the environment-resolved variants
// of one engine each.

#include <cstdlib>
#include <stdexcept>

#include "l2nn_engine.h"

namespace raft_amd {

namespace {

// A/B tuning switches, read once per process (docs/developer_guide.md)
struct L2nnEnv {
  char mode_2d, mode_256;  // '0' off, '1' wherever the shape allows, else auto
  char mode_xreg;          // '0' off, '1' on, else the measured default
  char mode_xring;         // '0' off, '1' on, else the measured default
  char w8;                 // '0' off, '2' for every nslice, else 3-slice only
  int gt;                  // 1, 2, 4 or 8; 0 = per-nslice default
  bool bk32, adirect, db, phased, persist;
};

const L2nnEnv& l2nn_env() {
  static const L2nnEnv env = [] {
    auto first = [](const char* name) {
      const char* e = getenv(name);
      return e ? e[0] : '\0';
    };
    L2nnEnv v;
    v.mode_2d = first("RAFT_AMD_L2NN_2D");
    v.mode_256 = first("RAFT_AMD_L2NN_256");
    v.mode_xreg = first("RAFT_AMD_L2NN_XREG");
    v.mode_xring = first("RAFT_AMD_L2NN_XRING");
    v.w8 = first("RAFT_AMD_L2NN_W8");
    const char* g = getenv("RAFT_AMD_L2NN_GT");
    v.gt = g ? atoi(g) : 0;
    if (v.gt != 1 && v.gt != 2 && v.gt != 4 && v.gt != 8) v.gt = 0;
    v.bk32 = first("RAFT_AMD_L2NN_BK32") == '1';
    v.adirect = first("RAFT_AMD_L2NN_AD") == '1';
    v.db = first("RAFT_AMD_L2NN_DB") == '1';
    v.phased = first("RAFT_AMD_L2NN_PHASED") == '1';
    v.persist = first("RAFT_AMD_PERSIST_L2NN") == '1';
    return v;
  }();
  return env;
}

constexpr const char* kEngineNames[] = {"auto",      "v1",      "v1_db", "v1_phased",
                                        "2d",        "2d_phased", "2d_bk32", "2d_ad",
                                        "256",       "w8",      "persist", "2d_xreg",
                                        "2d_xring"};

// auto picks 2d_xreg over 2d where both fit: 5.47 against 7.61 ms at
// 10M x 256 k=1024, one process, alternating
constexpr bool kXregDefault = true;

// auto picks 2d_xring over 2d_xreg: 4.94 against 5.16 ms at 10M x 256 k=1024,
// one process, alternating
constexpr bool kXringDefault = true;

bool is_2d(L2nnEngine e) {
  return e == L2nnEngine::TwoD || e == L2nnEngine::TwoDPhased ||
         e == L2nnEngine::TwoDBk32 || e == L2nnEngine::TwoDAd;
}

// the condition `e` violates on this shape, or nullptr. Every caller has
// already checked nslice in 1..3, n % 128 == 0 and d % 64 == 0.
const char* l2nn_engine_violation(L2nnEngine e, int nslice, int n, int d) {
  switch (e) {
    case L2nnEngine::V1Phased:
    case L2nnEngine::TwoDPhased:
      if (nslice != 2) return "the product-phase K-loop needs nslice == 2";
      return nullptr;
    case L2nnEngine::TwoD:
    case L2nnEngine::TwoDBk32:
    case L2nnEngine::TwoDAd:
      // 3-slice LDS (96 KiB) would drop to 1 block/CU: not instantiated
      if (nslice > 2) return "nslice must be 1 or 2";
      return nullptr;
    case L2nnEngine::E256:
      if (nslice > 2) return "nslice must be 1 or 2";
      if (n % 256 != 0) return "n must be a multiple of 256";
      return nullptr;
    case L2nnEngine::W8:
      if (n % 256 != 0) return "n must be a multiple of 256";
      return nullptr;
    case L2nnEngine::Persist:
      if (d > 256) return "d must be at most 256 (X stays in LDS)";
      return nullptr;
    case L2nnEngine::TwoDXreg:
    case L2nnEngine::TwoDXring:
      if (nslice != 1) return "nslice must be 1";
      if (d > 256) return "d must be at most 256 (X stays in registers)";
      return nullptr;
    default:
      return nullptr;
  }
}

// 2d auto: pays off when the col-tile loop is long enough that X re-reads
// dominate and m is large enough that partial traffic amortizes (16.9 ms vs
// v1's 17.4-18.0 at 10M x 256 k=1024, HBM reads 49 GB -> 6.7 GB; see
// BASELINE.md schedule table)
bool l2nn_2d_wanted(int nslice, long long m, int n) {
  const char mode = l2nn_env().mode_2d;
  return mode != '0' && nslice <= 2 && (mode == '1' || (n >= 512 && m >= 1000000));
}

// 2d_xreg takes the 1-slice d <= 256 shapes from 2d where 2d is wanted;
// RAFT_AMD_L2NN_XREG=0 gives them back, =1 is the default spelled out
bool l2nn_xreg_wanted() {
  const char mode = l2nn_env().mode_xreg;
  return mode != '0' && (mode == '1' || kXregDefault);
}

// 2d_xring takes 2d_xreg's shapes where it is wanted; RAFT_AMD_L2NN_XRING=0
// gives them back, =1 takes them whatever the default
bool l2nn_xring_wanted() {
  const char mode = l2nn_env().mode_xring;
  return mode != '0' && (mode == '1' || kXringDefault);
}

// w8 wins only for NSLICE=3 (staging-bound: halved X re-reads beat the lost
// cross-block barrier overlap); the 4-wave 2-block v1 kernel wins for
// NSLICE<=2 (34.3 vs 38.0 ms/step at 10M x 256 k=1024). RAFT_AMD_L2NN_W8=2
// forces w8 for ALL nslice (A/B experiments).
bool l2nn_w8_wanted(int nslice, int n, int d) {
  return n % 256 == 0 && d % 64 == 0 && (l2nn_env().w8 == '2' || nslice == 3);
}

// what the environment and the measured defaults pick
L2nnEngine l2nn_auto_engine(int nslice, long long m, int n, int d) {
  const L2nnEnv& env = l2nn_env();
  auto fits = [&](L2nnEngine e) { return !l2nn_engine_violation(e, nslice, n, d); };
  if (env.persist) {  // measured slower than v1 at 10M x 256 (occupancy)
    if (fits(L2nnEngine::Persist)) return L2nnEngine::Persist;
  } else {
    // 256: auto is OFF. Measured (profiles/pmc_l2nn_256_ab.txt): the 256^2
    // counted-vmcnt schedule at 1 block/CU loses to the 128^2 2-blocks/CU
    // implicit overlap on this op at every shape tried (23.7 vs 16.8 ms at
    // 10M x 1024 d=256). Kept as the base for future schedule work.
    if (env.mode_256 == '1' && fits(L2nnEngine::E256)) return L2nnEngine::E256;
    if (l2nn_2d_wanted(nslice, m, n)) {
      if (l2nn_xreg_wanted() && fits(L2nnEngine::TwoDXreg))
        return l2nn_xring_wanted() ? L2nnEngine::TwoDXring : L2nnEngine::TwoDXreg;
      if (env.bk32) return L2nnEngine::TwoDBk32;
      if (env.adirect) return L2nnEngine::TwoDAd;
      return env.phased && nslice == 2 ? L2nnEngine::TwoDPhased : L2nnEngine::TwoD;
    }
    if (env.w8 != '0' && l2nn_w8_wanted(nslice, n, d)) return L2nnEngine::W8;
  }
  if (env.db) return L2nnEngine::V1Db;
  return env.phased && nslice == 2 ? L2nnEngine::V1Phased : L2nnEngine::V1;
}

}  // namespace

const char* l2nn_engine_name(L2nnEngine e) { return kEngineNames[(int)e]; }

L2nnEngine l2nn_engine_from_name(const std::string& name, bool* known) {
  *known = true;
  for (int i = 0; i < (int)(sizeof(kEngineNames) / sizeof(kEngineNames[0])); i++)
    if (name == kEngineNames[i]) return (L2nnEngine)i;
  *known = false;
  return L2nnEngine::Auto;
}

L2nnPlan l2nn_resolve_engine(int nslice, long long m, int n, int d,
                             L2nnEngine requested, int gt) {
  L2nnPlan plan{requested, 0, 0, {}};
  if (requested == L2nnEngine::Auto) {
    plan.engine = l2nn_auto_engine(nslice, m, n, d);
  } else if (const char* why = l2nn_engine_violation(requested, nslice, n, d)) {
    plan.error = std::string("fused_l2nn engine '") + l2nn_engine_name(requested) +
                 "': " + why;
    return plan;
  }
  if (is_2d(plan.engine)) {
    // col-tiles per block, nslice-aware default (measured at 10M x 256
    // k=1024: 1-slice GT8 9.55 / GT4 9.69 / GT2 11.30 ms — the epilogue is a
    // bigger share of the cheaper 1-product k-loop, so amortizing it over
    // more tiles wins; 2-slice GT2 remains the optimum). GT=8 is instantiated
    // for the 1-slice 64-wide K-loop only. Halve until it divides the
    // col-tile count, so odd tile counts (e.g. n=384) keep the 2D engine.
    if (gt == 0) gt = l2nn_env().gt;
    if (gt == 0) gt = nslice == 1 ? 8 : 2;
    if (gt > 4 && (nslice == 2 || plan.engine == L2nnEngine::TwoDBk32)) gt = 4;
    const int tiles = n / 128;
    while (gt > 1 && tiles % gt != 0) gt >>= 1;
    plan.gt = gt;
    plan.n_groups = tiles / gt;
  } else if (plan.engine == L2nnEngine::TwoDXreg ||
             plan.engine == L2nnEngine::TwoDXring) {
    // same rule as the 1-slice 2d default; a single group writes the result
    // itself and needs no partials
    if (gt == 0) gt = l2nn_env().gt;
    if (gt == 0) gt = 8;
    const int tiles = n / 128;
    while (gt > 1 && tiles % gt != 0) gt >>= 1;
    plan.gt = gt;
    plan.n_groups = tiles / gt > 1 ? tiles / gt : 0;
  } else if (plan.engine == L2nnEngine::E256) {
    plan.n_groups = n / 256;
  }
  return plan;
}

void launch_fused_l2nn(const L2nnPlan& plan, const void** xsl, const void** csl,
                       const float* xn, const float* cn, float* pd, float* pd2,
                       int* pi, float* dmin, int* amin, float* dmin2, long long m,
                       int n, int d, int nslice, hipStream_t stream) {
  if (!plan.error.empty()) throw std::runtime_error(plan.error);
  const SlicePtrs p(xsl, csl, nslice);
  if (is_2d(plan.engine))
    launch_l2nn_2d(p, xn, cn, pd, pd2, pi, dmin, amin, dmin2, m, n, d, nslice,
                   plan.engine, plan.gt, stream);
  else if (plan.engine == L2nnEngine::TwoDXreg)
    launch_l2nn_xreg(p, xn, cn, pd, pd2, pi, dmin, amin, dmin2, m, n, d, plan.gt, stream);
  else if (plan.engine == L2nnEngine::TwoDXring)
    launch_l2nn_xring(p, xn, cn, pd, pd2, pi, dmin, amin, dmin2, m, n, d, plan.gt, stream);
  else if (plan.engine == L2nnEngine::E256)
    launch_l2nn_256(p, xn, cn, pd, pd2, pi, dmin, amin, dmin2, m, n, d, nslice, stream);
  else if (plan.engine == L2nnEngine::W8)
    launch_l2nn_w8(p, xn, cn, dmin, amin, dmin2, m, n, d, nslice, stream);
  else if (plan.engine == L2nnEngine::Persist)
    launch_l2nn_persist(p, xn, cn, dmin, amin, dmin2, m, n, d, nslice, stream);
  else
    launch_l2nn_v1(p, xn, cn, dmin, amin, dmin2, m, n, d, nslice, plan.engine, stream);
}

// ---- include/raft_amd/neighbors.hpp: one engine each, environment-resolved --

static void check_nslice(int nslice) {
  if (nslice < 1 || nslice > 3)
    throw std::runtime_error("fused_l2nn: nslice must be 1, 2 or 3");
}

void launch_fused_l2nn_split(const void** xsl, const void** csl, const float* xn,
                             const float* cn, float* dmin, int* amin, float* dmin2,
                             long long m, int n, int d, int nslice,
                             hipStream_t stream) {
  check_nslice(nslice);
  const L2nnEnv& env = l2nn_env();
  const L2nnEngine v1 = env.db ? L2nnEngine::V1Db
                        : env.phased && nslice == 2 ? L2nnEngine::V1Phased
                                                    : L2nnEngine::V1;
  launch_fused_l2nn({v1, 0, 0, {}}, xsl, csl, xn, cn, nullptr, nullptr, nullptr, dmin,
                    amin, dmin2, m, n, d, nslice, stream);
}

bool fused_l2nn_2d_supported(int nslice, long long m, int n, int d) {
  return n % 128 == 0 && l2nn_2d_wanted(nslice, m, n);
}

void launch_fused_l2nn_2d(const void** xsl, const void** csl, const float* xn,
                          const float* cn, float* pd, float* pd2, int* pi,
                          float* dmin, int* amin, float* dmin2, long long m, int n,
                          int d, int nslice, hipStream_t stream) {
  check_nslice(nslice);
  const L2nnEnv& env = l2nn_env();
  const L2nnEngine v = env.bk32      ? L2nnEngine::TwoDBk32
                       : env.adirect ? L2nnEngine::TwoDAd
                       : env.phased && nslice == 2 ? L2nnEngine::TwoDPhased
                                                   : L2nnEngine::TwoD;
  launch_fused_l2nn(l2nn_resolve_engine(nslice, m, n, d, v, 0), xsl, csl, xn, cn, pd,
                    pd2, pi, dmin, amin, dmin2, m, n, d, nslice, stream);
}

bool fused_l2nn_w8_supported(int nslice, int n, int d) {
  return l2nn_w8_wanted(nslice, n, d);
}

void launch_fused_l2nn_w8(const void** xsl, const void** csl, const float* xn,
                          const float* cn, float* dmin, int* amin, float* dmin2,
                          long long m, int n, int d, int nslice, hipStream_t stream) {
  check_nslice(nslice);
  launch_fused_l2nn(l2nn_resolve_engine(nslice, m, n, d, L2nnEngine::W8, 0), xsl, csl,
                    xn, cn, nullptr, nullptr, nullptr, dmin, amin, dmin2, m, n, d,
                    nslice, stream);
}

}  // namespace raft_amd
