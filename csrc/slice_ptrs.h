// bf16 slice pointers of a split-bf16 launch, shared by the fused L2-NN and
// the pairwise L2 families. Passed to kernels by value: its x / c arrays are
// what mfma_tile_kloop takes.
#pragma once

#include <hip/hip_runtime.h>

namespace raft_amd {

// a missing slice aliases slice 0 (the kernels never read it)
struct SlicePtrs {
  const __bf16* x[3];
  const __bf16* c[3];
  SlicePtrs(const void** xsl, const void** csl, int nslice) {
    for (int s = 0; s < 3; s++) {
      x[s] = (const __bf16*)xsl[s < nslice ? s : 0];
      c[s] = (const __bf16*)csl[s < nslice ? s : 0];
    }
  }
};

}  // namespace raft_amd
