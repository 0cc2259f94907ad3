// Fused L2 nearest-neighbor engines (csrc/fused_l2nn*.hip) — the k-means
// assignment step. dmin2 (second-best distance) feeds the verified engine's
// provable split-error margin test (see csrc/fused_l2nn.hip header).
#pragma once

#include "core.hpp"

namespace raft_amd {

// v1: one block per row tile, col-tile loop in-kernel
void launch_fused_l2nn_split(const void** xsl, const void** csl, const float* xn,
                             const float* cn, float* dmin, int* amin, float* dmin2,
                             long long m, int n, int d, int nslice, hipStream_t s);
// 2D XCD-swizzled tile-pair grid + partials combine (default at m>=1M):
// pd/pd2/pi are (n/128/GT * m) workspace arrays
bool fused_l2nn_2d_supported(int nslice, long long m, int n, int d);
void launch_fused_l2nn_2d(const void** xsl, const void** csl, const float* xn,
                          const float* cn, float* pd, float* pd2, int* pi,
                          float* dmin, int* amin, float* dmin2,
                          long long m, int n, int d, int nslice, hipStream_t s);
// 8-wave 128x256 variant (default for 3-slice) + persistent-X (env-gated)
bool fused_l2nn_w8_supported(int nslice, int n, int d);
void launch_fused_l2nn_w8(const void** xsl, const void** csl, const float* xn,
                          const float* cn, float* dmin, int* amin, float* dmin2,
                          long long m, int n, int d, int nslice, hipStream_t s);
// exact-fp32 rescan/repair of rows whose margin is inside the split bound;
// lead/tail select the bound for the split mode that produced dmin/dmin2
// (defaults = bf16x2v; bf16x1v passes 2^-7 / 2^-12)
void launch_l2nn_verify_repair(const float* x, const float* c, const float* xn,
                               float* dmin, int* amin, const float* dmin2,
                               const float* cn_max_dev, long long m, int n, int d,
                               hipStream_t s, float lead = 0x1p-13f,
                               float tail = 0x1p-18f);

// Verified epsilon-neighborhood (csrc/eps_neighbors.hip): packed adjacency
// bitmap[i][j] = (||x_i - y_j||^2 <= eps2), n_words 32-bit words per row,
// little-endian bits, tail bits zero. xsl/csl are bf16 slices padded to
// d % 64 == 0. xf/yf (original fp32 rows, leading dim df) enable the exact
// recheck of pairs within 2*(lead*sqrt(xn*yn) + tail*(xn+yn)) of eps2 and
// require the `rechecked` counter; pass nullptr for bf16 input (1 slice).
// eps2 must be finite and >= 0.
void launch_eps_neighbors_l2sq(const void** xsl, const void** csl, const float* xn,
                               const float* yn, const float* xf, const float* yf,
                               unsigned int* bitmap, unsigned long long* rechecked,
                               float eps2, float lead, float tail, long long m,
                               long long n, int d, int df, long long n_words,
                               int nslice, hipStream_t s);
// row-padded bitmap utilities: per-row popcount, CSR fill (sorted int32
// column ids at indptr[row]) and dense bool expansion
void launch_bitmap_row_degrees(const unsigned int* bitmap, long long* deg,
                               long long m, long long n_words, hipStream_t s);
void launch_bitmap_rows_to_csr(const unsigned int* bitmap, const long long* indptr,
                               int* indices, long long m, long long n_words,
                               hipStream_t s);
void launch_bitmap_rows_expand(const unsigned int* bitmap, bool* out, long long m,
                               long long n, long long n_words, hipStream_t s);

// Masked fused L2-NN (csrc/masked_l2nn.hip): per row of x the nearest y row
// among the y GROUPS its mask allows. y_group[n] holds non-decreasing group
// ids in [0, n_groups); a column of group g is allowed for row i iff
// (adj == nullptr or bit g of adj row i is set) and g != x_group[i]
// (x_group == nullptr excludes nothing; one of the two is required). adj has
// adj_words 32-bit words per row. pd/pd2/pi are n_split * m scratch arrays
// (one partial per column split, n_split in [1, ceil(n/128)]); visited and
// skipped tiles are added to counters[0] and counters[1]. Writes the emulated
// (dmin, amin, dmin2 = second best over allowed columns); rows with no
// allowed column get (+inf, -1, +inf).
void launch_masked_l2nn(const void** xsl, const void** csl, const float* xn,
                        const float* yn, const int* y_group,
                        const unsigned int* adj, long long adj_words,
                        const int* x_group, float* pd, float* pd2, int* pi,
                        float* dmin, int* amin, float* dmin2,
                        unsigned long long* counters, long long m, int n, int d,
                        int n_split, int nslice, hipStream_t s);
// exact fp32 verify / repair of that result, in place and without a host
// sync: rows with dmin2 - dmin <= 2*(lead*sqrt(xn*yn_max) + tail*(xn + yn_max))
// rescan their allowed columns with the unexpanded fp32 distance (exact ties
// to the smallest index, or to the smallest y_rank when given — then
// inv_rank[y_rank[j]] == j is required too), every other row recomputes its
// chosen distance. x/y have leading dimension df. Scratch: rescan_rows[m],
// rescan_count[1] (zeroed here) and keys[m]. Rescanned rows are added to
// *rescanned.
void launch_masked_l2nn_verify_repair(const float* x, const float* y, const float* xn,
                                      const int* y_group, const unsigned int* adj,
                                      long long adj_words, const int* x_group,
                                      const int* y_rank, const int* inv_rank,
                                      float* dmin, int* amin, const float* dmin2,
                                      const float* yn_max_dev, int* rescan_rows,
                                      unsigned int* rescan_count,
                                      unsigned long long* keys,
                                      unsigned long long* rescanned, long long m,
                                      int n, int df, float lead, float tail,
                                      hipStream_t s);

// IVF-Flat list scan (csrc/ivf_flat_scan.hip): distances from queries to the
// rows of the lists they probe, list-major. data is the interleaved index
// buffer (fp32, or bf16 with data_bf16): rows in groups of 64, 16-byte chunks,
// d padded to the chunk; list_offsets[n_lists + 1] in rows (multiples of 64);
// indices[total_rows] dataset ids, -1 in pad slots. Work item i < *n_items
// (a DEVICE scalar; the grid's x size max_items is an upper bound) scans list
// item_list[i] for the item_pair_count[i] <= qg sorted pairs starting at
// item_pair_begin[i]; sorted pair p belongs to query row pair_query[p] of
// queries [n_queries, d] and writes its list's padded rows at
// out[pair_out_off[p] + row]. Pad rows and rows whose id has a clear bit in
// filter_words (nullptr: no filter; ids >= filter_bits are rejected) get +inf
// (-inf for inner product). metric: 0 squared L2 (unexpanded sum), 1 its
// square root, 2 inner product. qg in {4, 8, 16, 32} with
// qg <= ivf_flat_scan_max_qg(d_pad); y_split blocks share a list's groups.
int ivf_flat_scan_max_qg(int d_pad);
void launch_ivf_flat_scan(const void* data, bool data_bf16,
                          const long long* list_offsets, const long long* indices,
                          const float* queries, const long long* item_list,
                          const long long* item_pair_begin,
                          const long long* item_pair_count, const long long* n_items,
                          const long long* pair_query, const long long* pair_out_off,
                          const unsigned int* filter_words, long long filter_bits,
                          float* out, long long out_numel, long long n_lists,
                          long long total_rows, long long n_queries, long long n_pairs,
                          long long max_items, int d, int metric, int qg, int y_split,
                          hipStream_t s);

}  // namespace raft_amd
