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
// elem_size is the bytes one staged query element takes in LDS: 4 for this
// launcher, 1 (plus one int norm per query) for launch_ivf_flat_scan_i8.
int ivf_flat_scan_max_qg(int d_pad, int elem_size = 4);
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
// The same scan over int8 (data_signed) or uint8 rows
// (csrc/ivf_flat_scan_i8.hip): 16 one-byte elements per chunk, queries
// [n_queries, d] bytes of the rows' type, d <= 4096. Distances are exact
// integers (8-bit dot4 into int32) converted to fp32 once; metric 1 is the
// fp64 root of the exact squared distance rounded to fp32. qg in
// {4, 8, 16, 32} with qg <= ivf_flat_scan_max_qg(d_pad, 1). Every other
// argument as in launch_ivf_flat_scan.
void launch_ivf_flat_scan_i8(const void* data, bool data_signed,
                             const long long* list_offsets, const long long* indices,
                             const void* queries, const long long* item_list,
                             const long long* item_pair_begin,
                             const long long* item_pair_count, const long long* n_items,
                             const long long* pair_query, const long long* pair_out_off,
                             const unsigned int* filter_words, long long filter_bits,
                             float* out, long long out_numel, long long n_lists,
                             long long total_rows, long long n_queries, long long n_pairs,
                             long long max_items, int d, int metric, int qg, int y_split,
                             hipStream_t s);

// IVF-PQ (csrc/ivf_pq.hip), 8-bit codes. codebooks is fp32
// [pq_dim][pq_len][256] (entry-minor), pq_len = ceil(d / pq_dim), features
// past d are zero; pq_dim_pad = pq_dim rounded up to 16.
//
// Encode: codes[n][pq_dim_pad] (row-major, pad bytes 0) gets, per subspace,
// the entry nearest to the residual x - centroids[labels[row]] (unexpanded
// fp32 sum, exact ties to the smallest entry); a row whose label is outside
// [0, n_lists) gets code 0. pq_len <= 32.
void launch_ivf_pq_encode(const float* x, const long long* labels, const float* centroids,
                          const float* codebooks, unsigned char* codes, long long n,
                          long long n_lists, int d, int pq_dim, int pq_len, hipStream_t s);
// Scan, pair-major: pair p = query p / n_probes, list probes[p], one
// look-up table in LDS per block; ivf_pq_scan_lds_bytes must not exceed
// 160 KiB less 16 bytes, else the launcher throws. codes is the IVF-Flat
// interleaved layout with byte elements (16 codes per chunk, 16-byte aligned);
// list_offsets / indices / filter / out / metric as in launch_ivf_flat_scan,
// with pair_out_off[p] in probe order. Distances are to the reconstructed
// rows centroid + decoded residual. y_split blocks share a list's groups and
// each rebuilds the table.
size_t ivf_pq_scan_lds_bytes(int pq_dim, int pq_len);
void launch_ivf_pq_scan(const unsigned char* codes, const long long* list_offsets,
                        const long long* indices, const float* queries,
                        const float* centroids, const float* codebooks,
                        const long long* probes, const long long* pair_out_off,
                        const unsigned int* filter_words, long long filter_bits, float* out,
                        long long out_numel, long long n_lists, long long total_rows,
                        long long n_queries, int n_probes, int d, int pq_dim, int pq_len,
                        int metric, int y_split, hipStream_t s);

// IVF-PQ with 4-bit codes (csrc/ivf_pq4.hip). codebooks is fp32
// [pq_dim][pq_len][16]; a stored row is row_bytes = ceil(pq_dim / 2) rounded
// up to 16 bytes, byte t holding subspace 2t in bits 0..3 and subspace 2t + 1
// in bits 4..7, pad nibbles and pad bytes 0.
//
// Encode: codes[n][row_bytes] (row-major, 16-byte aligned) by the rule of
// launch_ivf_pq_encode; a row whose label is outside [0, n_lists) gets zeros.
// pq_len <= 32.
void launch_ivf_pq4_encode(const float* x, const long long* labels, const float* centroids,
                           const float* codebooks, unsigned char* codes, long long n,
                           long long n_lists, int d, int pq_dim, int pq_len, hipStream_t s);
// Scan, list-major: the work items, pair arrays, list_offsets / indices /
// filter / out / metric of launch_ivf_flat_scan over the interleaved code
// buffer (row_bytes / 16 chunks of 32 subspaces, 16-byte aligned). A block
// holds the fp32 look-up tables and residuals of qg queries:
// qg * (2048 * row_bytes / 16 + 4 * pq_dim * pq_len) bytes plus 16 + 4 qg
// within 64 KiB. ivf_pq4_scan_max_qg is the largest qg in {8, 4, 2, 1} that
// fits, 0 for pq_dim > 256 or pq_len > 32; a larger qg makes the launcher
// throw. Distances are to the reconstructed rows and do not depend on qg.
int ivf_pq4_scan_max_qg(int pq_dim, int pq_len);
void launch_ivf_pq4_scan(const unsigned char* codes, const long long* list_offsets,
                         const long long* indices, const float* queries,
                         const float* centroids, const float* codebooks,
                         const long long* item_list, const long long* item_pair_begin,
                         const long long* item_pair_count, const long long* n_items,
                         const long long* pair_query, const long long* pair_out_off,
                         const unsigned int* filter_words, long long filter_bits, float* out,
                         long long out_numel, long long n_lists, long long total_rows,
                         long long n_queries, long long n_pairs, long long max_items, int d,
                         int pq_dim, int pq_len, int metric, int qg, int y_split,
                         hipStream_t s);

// refine (csrc/refine.hip): exact re-rank of kNN candidates, one block per
// query. dataset is [n][d] of dtype 0 fp32, 1 bf16 or 2 fp16 with rows
// row_pitch ELEMENTS apart (n < 2^32 - 1); queries fp32 [n_queries][d];
// candidates int64 [n_queries][n_cand]; an id outside [0, n) is no candidate
// and is never dereferenced. dists / ids [n_queries][k] get the k best by
// the exact fp32 distance (metric as in launch_ivf_flat_scan), best first,
// ties to the smaller id, a repeated id repeatedly; a NaN distance becomes
// +inf (-inf for inner product) and keeps its id; missing slots hold that
// value and id -1. Serves d <= 8192, n_cand <= 4096 and
// k <= refine_key_slots(n_cand) (n_cand rounded up to a power of two, at least
// 256), else the launcher throws.
int refine_key_slots(int n_cand);
void launch_refine(const void* dataset, int dtype, long long n, long long row_pitch,
                   const float* queries, const long long* candidates, float* dists,
                   long long* ids, long long n_queries, int d, int n_cand, int k, int metric,
                   hipStream_t s);

// CAGRA (csrc/cagra.hip). launch_cagra_search: greedy graph walk, one block
// per query. dataset as in launch_refine with n < 2^31; graph int32
// [n][graph_degree], -1 or any id outside [0, n) is "no edge"; queries fp32
// [n_queries][d]; seeds int32, n_seeds per query, rows seed_pitch ELEMENTS
// apart (0 = one row for all). The list of the itopk_size best rows by
// (distance, smaller id) is grown from the seeds by expanding the
// search_width best unexpanded entries per round, for at most max_iterations
// rounds; dists / ids [n_queries][k] get its first k entries, missing slots
// +inf (-inf for inner product) and -1. hash_slots sizes the visited table: a
// power of two in [2 * (itopk_size + max(search_width * graph_degree,
// n_seeds)), 8192]. Serves d <= 4096, itopk_size <= 512, search_width *
// graph_degree <= 512, n_seeds <= 512, k <= itopk_size, else the launcher
// throws. cagra_search_lds_bytes is the dynamic LDS of one block (vec = 4 for
// fp32 rows, 8 for bf16 / fp16).
//
// launch_cagra_prune: knn_graph int32 [n][kd] (rows nearest first, distinct
// ids) -> pruned int32 [n][graph_degree], the ranks with the smallest (detour
// count, rank) as ids, -1 for absent. Serves graph_degree <= kd <= 256.
int cagra_search_key_slots(int itopk_size, int n_candidates, int n_seeds);
size_t cagra_search_lds_bytes(int d, int vec, int itopk_size, int n_candidates, int n_seeds,
                              int hash_slots, int search_width);
void launch_cagra_search(const void* dataset, int dtype, long long n, long long row_pitch,
                         const int* graph, int graph_degree, const float* queries,
                         const int* seeds, long long seed_pitch, int n_seeds, float* dists,
                         long long* ids, long long n_queries, int d, int k, int itopk_size,
                         int search_width, int max_iterations, int hash_slots, int metric,
                         hipStream_t s);
void launch_cagra_prune(const int* knn_graph, int* pruned, long long n, int kd, int graph_degree,
                        hipStream_t s);

// NN-descent (csrc/nn_descent.hip). launch_nn_descent_join: one block per node
// gathers the rows of new_ids / old_ids int32 [n_nodes][2 * n_samples] (-1 or
// any id outside [0, n) is no row) from dataset (as in launch_refine, n < 2^31),
// forms the 64 x 128 tile of values (norms[u] + norms[v]) - 2 dot (-dot for
// metric 2) on the bf16 matrix cores and writes, at fixed positions
// [n_nodes][6 * n_samples], (target u, id v, value) of the smallest (value, v):
// every NEW row among NEW, every NEW row among OLD, every OLD row among NEW; -1
// and +inf where there is none. Serves d <= 4096, n_samples <= 32.
//
// launch_nn_descent_merge: one block per target u merges the candidates
// cand_id / cand_val [seg_off[u], seg_off[u + 1]) into the list vals / ids /
// flags [n][k] (ascending (value, id), -1 absent): distinct ids, an id already
// listed keeps its entry and flag, a new one is flagged, u itself never enters.
// counter gains (new flags after - before). Serves k <= 256.
void launch_nn_descent_join(const void* dataset, int dtype, long long n, long long row_pitch,
                            const float* norms, const int* new_ids, const int* old_ids,
                            int* out_target, int* out_id, float* out_val, long long n_nodes, int d,
                            int n_samples, int metric, hipStream_t s);
void launch_nn_descent_merge(float* vals, int* ids, unsigned char* flags, long long n, int k,
                             const long long* seg_off, const int* cand_id, const float* cand_val,
                             unsigned long long* counter, hipStream_t s);

}  // namespace raft_amd
