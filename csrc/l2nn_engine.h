// Fused L2-NN engine selection: the one place that reads the RAFT_AMD_L2NN_*
// tuning variables and holds every engine's shape predicate. Host-only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "slice_ptrs.h"

namespace raft_amd {

enum class L2nnEngine {
  Auto,        // "auto": environment overrides, then the measured defaults
  V1,          // "v1": fused_l2nn_kernel, col-tile loop inside one block
  V1Db,        // "v1_db": v1 over the BK=32 double-buffered K-loop
  V1Phased,    // "v1_phased": v1 over the 2-slice product-phase K-loop
  TwoD,        // "2d": fused_l2nn_2d_kernel + partials combine
  TwoDPhased,  // "2d_phased": 2d over the 2-slice product-phase K-loop
  TwoDBk32,    // "2d_bk32": fused_l2nn_2d_bk32_kernel (4 blocks/CU)
  TwoDAd,      // "2d_ad": 2d with X fragments loaded global->register
  E256,        // "256": fused_l2nn_256_kernel
  W8,          // "w8": fused_l2nn_w8_kernel (128 x 256 tile, 8 waves)
  Persist,     // "persist": fused_l2nn_persist_kernel (best only)
  TwoDXreg,    // "2d_xreg": fused_l2nn_xreg_kernel (1 slice, X in registers)
  TwoDXring,   // "2d_xring": fused_l2nn_xring_kernel (2d_xreg, counted C ring)
};

const char* l2nn_engine_name(L2nnEngine e);
// Auto for an unknown name
L2nnEngine l2nn_engine_from_name(const std::string& name, bool* known);

struct L2nnPlan {
  L2nnEngine engine;  // never Auto
  int gt;             // col-tiles per block (2d engines), else 0
  int n_groups;       // partial triples per row the engine needs, else 0
  std::string error;  // non-empty: `requested` cannot run this shape
};

// requested == Auto resolves the environment and the defaults; a named engine
// is checked against its shape predicate and never replaced. gt: 0 = the
// environment / per-nslice default, else 1, 2, 4 or 8; it is halved until it
// divides the col-tile count and capped at what the engine instantiates.
L2nnPlan l2nn_resolve_engine(int nslice, long long m, int n, int d,
                             L2nnEngine requested, int gt);

// run a resolved plan; pd/pd2/pi are plan.n_groups * m scratch arrays
void launch_fused_l2nn(const L2nnPlan& plan, const void** xsl, const void** csl,
                       const float* xn, const float* cn, float* pd, float* pd2,
                       int* pi, float* dmin, int* amin, float* dmin2, long long m,
                       int n, int d, int nslice, hipStream_t stream);

// per-file launchers: take the resolved variant, read no environment
void launch_l2nn_v1(const SlicePtrs& p, const float* xn, const float* cn,
                    float* dmin, int* amin, float* dmin2, long long m, int n, int d,
                    int nslice, L2nnEngine variant, hipStream_t stream);
void launch_l2nn_2d(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                    float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                    long long m, int n, int d, int nslice, L2nnEngine variant, int gt,
                    hipStream_t stream);
// writes dmin / amin / dmin2 itself when gt covers all of n (no partials)
void launch_l2nn_xreg(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                      float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                      long long m, int n, int d, int gt, hipStream_t stream);
void launch_l2nn_xring(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                       float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                       long long m, int n, int d, int gt, hipStream_t stream);
void launch_l2nn_256(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                     float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                     long long m, int n, int d, int nslice, hipStream_t stream);
void launch_l2nn_w8(const SlicePtrs& p, const float* xn, const float* cn, float* dmin,
                    int* amin, float* dmin2, long long m, int n, int d, int nslice,
                    hipStream_t stream);
void launch_l2nn_persist(const SlicePtrs& p, const float* xn, const float* cn,
                         float* dmin, int* amin, float* dmin2, long long m, int n,
                         int d, int nslice, hipStream_t stream);

}  // namespace raft_amd
