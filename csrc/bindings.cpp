// Python bindings for the raft_amd native extension (raft_amd._C).
// Torch tensors in, torch tensors out; every launch goes onto the current
// PyTorch HIP stream so the ops compose with torch's own kernels.
// Reference parity: the raft_runtime instantiation layer + pylibraft's
// Cython bridges (cpp/src/*, python/pylibraft/**/*.pyx) collapsed into one
// torch-extension TU.

#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <limits>

#include "l2nn_engine.h"
#include "pairwise_variant.h"

namespace raft_amd {

// from rng.hip (device sampling test driver)
void launch_device_sample_test(const float*, int*, int, uint64_t, hipStream_t);
// from spmv.hip (sddmm)
void launch_sddmm(const float*, const float*, const int*, const int*, float*,
                  long long, long long, hipStream_t);
// from linewise.hip
void launch_linewise(const float*, float*, const float*, const float*,
                     long long, long long, bool, int, int, hipStream_t);
// from histogram.hip
void launch_histogram(const float*, long long, long long, int, float, float,
                      unsigned long long*, hipStream_t);
void launch_bitset_set(unsigned int*, const long long*, long long, int, hipStream_t);
void launch_bitset_test(const unsigned int*, const long long*, bool*, long long,
                        hipStream_t);
void launch_bitset_count(const unsigned int*, long long, unsigned long long*,
                         hipStream_t);
// from solver_kernels.hip
void launch_cholesky_r1_update_f32(float*, float*, int, long long, hipStream_t);
void launch_lanczos_pre(float*, const float*, const float*, const float*,
                        double*, long long, hipStream_t);
void launch_lanczos_sub_alpha(float*, const float*, const double*, float*,
                              long long, hipStream_t);
void launch_lanczos_norm2(const float*, double*, long long, hipStream_t);
void sgemv_rowmajor(const float*, const float*, float*, long long, long long,
                    bool, float, float, void*);
void launch_lanczos_normalize(const float*, float*, const double*, float*,
                              float*, float*, long long, hipStream_t);
void launch_cholesky_r1_update_f64(double*, double*, int, long long, hipStream_t);
// from reductions.hip
template <int OP, typename T>
void launch_reduce_rows(const T*, T*, long long, long long, hipStream_t);
template <int OP, typename T>
void launch_reduce_cols(const T*, T*, long long, long long, hipStream_t);
void launch_row_argmin(const float*, int*, long long, long long, hipStream_t);
void launch_rows_sqnorm_bf16(const void*, float*, long long, long long, hipStream_t);
void launch_row_normalize_l2(const float*, float*, long long, long long, float, hipStream_t);
// from pairwise.hip
void launch_l2_epilogue(float*, const float*, const float*, long long, long long, hipStream_t);
void launch_l2nn_epilogue(const float*, const float*, const float*, float*, int*,
                          long long, long long, hipStream_t);
void launch_pairwise_expanded_epilogue(float*, const float*, const float*, long long,
                                       long long, int, float, hipStream_t);
void launch_pairwise_unexpanded(const float*, const float*, float*, long long, long long,
                                long long, int, float, hipStream_t);
// from rng.hip
void launch_rng_uniform(float*, long long, uint64_t, uint64_t, hipStream_t, int);
void launch_rng_normal(float*, long long, uint64_t, uint64_t, hipStream_t, int);
void launch_make_blobs(float*, int*, const float*, long long, long long, int, float,
                       uint64_t, uint64_t, hipStream_t);
// from spmv.hip
template <typename T>
void launch_csr_spmv(const int*, const int*, const T*, const T*, T*, long long,
                     long long, hipStream_t);
// from sparse_pairwise.hip
void launch_csr_row_stats(const int*, const float*, float*, long long, long long, int,
                          float, hipStream_t);
void launch_csr_pairwise(const int*, const int*, const float*, long long, long long,
                         const int*, const int*, const float*, long long, long long,
                         const float*, const float*, float*, long long, int, float, int,
                         int, hipStream_t);
// from kmeans.hip
void launch_reduce_rows_by_key(const float*, const int*, float*, float*, long long,
                               long long, long long, int, hipStream_t);
void launch_reduce_rows_by_key_sorted(const float*, const int*, const int*, float*,
                                      float*, const float*, float*, long long,
                                      long long, hipStream_t);
void launch_split_bf16_norms(const float*, void*, void*, void*, float*, int,
                             long long, long long, hipStream_t,
                             float* = nullptr);
void launch_kmeans_update_centroids(const float*, const float*, float*, long long,
                                    long long, hipStream_t);
void launch_l2nn_verify_repair(const float*, const float*, const float*, float*, int*,
                               const float*, const float*, long long, int, int,
                               hipStream_t, float, float);
void launch_kmeans_update_verify(const float*, const int*, const int*, const float*,
                                 const float*, float*, int*, const float*,
                                 const float*, float*, float*, float*, long long,
                                 long long, int, hipStream_t, float, float);
// from select_k.hip
long long select_k_workspace_bytes(long long batch);
void launch_select_k(const float*, float*, int*, void*, long long, long long, int,
                     bool, bool, hipStream_t);
void launch_select_k_warpsort(const float*, float*, int*, long long, long long, int,
                              bool, hipStream_t);
template <typename T>
void launch_select_k_generic_t(const T*, const long long*, long long, long long,
                               T*, long long*, long long, long long, bool,
                               hipStream_t);
void launch_eps_neighbors_l2sq(const void**, const void**, const float*, const float*,
                               const float*, const float*, unsigned int*,
                               unsigned long long*, float, float, float, long long,
                               long long, int, int, long long, int, hipStream_t);
void launch_bitmap_row_degrees(const unsigned int*, long long*, long long, long long,
                               hipStream_t);
void launch_bitmap_rows_to_csr(const unsigned int*, const long long*, int*, long long,
                               long long, hipStream_t);
void launch_bitmap_rows_expand(const unsigned int*, bool*, long long, long long,
                               long long, hipStream_t);
void launch_masked_l2nn(const void**, const void**, const float*, const float*,
                        const int*, const unsigned int*, long long, const int*, float*,
                        float*, int*, float*, int*, float*, unsigned long long*,
                        long long, int, int, int, int, hipStream_t);
void launch_masked_l2nn_verify_repair(const float*, const float*, const float*,
                                      const int*, const unsigned int*, long long,
                                      const int*, const int*, const int*, float*, int*,
                                      const float*, const float*, int*, unsigned int*,
                                      unsigned long long*, unsigned long long*,
                                      long long, int, int, float, float, hipStream_t);
// from ivf_flat_scan.hip
int ivf_flat_scan_max_qg(int);
void launch_ivf_flat_scan(const void*, bool, const long long*, const long long*,
                          const float*, const long long*, const long long*,
                          const long long*, const long long*, const long long*,
                          const long long*, const unsigned int*, long long, float*,
                          long long, long long, long long, long long, long long,
                          long long, int, int, int, int, hipStream_t);
// from gemm_rocblas.cpp
void gemm_bf16_f32_rowmajor(const void*, const void*, float*, long long, long long,
                            long long, float, void*);
void gemm_f32_rowmajor(const float*, const float*, float*, long long, long long,
                       long long, float, void*);
void gemm_bf16_f32_rowmajor_lt(const void*, const void*, float*, long long, long long,
                               long long, float, void*);
void gemm_bf16_f32_nt_rowmajor_lt(const void*, const void*, float*, long long, long long,
                                  long long, float, void*);
void gemm_bf16_f32_nt_rowmajor(const void*, const void*, float*, long long, long long,
                               long long, float, void*);
}  // namespace raft_amd

namespace {

hipStream_t cur_stream() {
  return (hipStream_t)c10::hip::getCurrentHIPStream().stream();
}

void check_f32_2d(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 2, name, " must be 2D");
}

void check_reduce_input(const torch::Tensor& x, int64_t op, int64_t reduced) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2,
              "x must be a contiguous 2D GPU tensor");
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 || x.scalar_type() == torch::kFloat64,
              "x must be float32 or float64");
  TORCH_CHECK(op >= 0 && op <= 5, "bad op code ", op);
  // sums over an empty axis are zeros; min/max have no identity to return
  TORCH_CHECK(op <= 2 || reduced > 0, "min/max reduction over an empty axis");
}

torch::Tensor reduce_rows(torch::Tensor x, int64_t op) {
  check_reduce_input(x, op, x.dim() == 2 ? x.size(1) : 1);
  auto out = torch::empty({x.size(0)}, x.options());
  auto s = cur_stream();
  const long long m = x.size(0), d = x.size(1);
#define CASE(OPC)                                                                     \
  case OPC:                                                                           \
    if (x.scalar_type() == torch::kFloat32)                                           \
      raft_amd::launch_reduce_rows<OPC, float>(x.data_ptr<float>(), out.data_ptr<float>(), m, d, s); \
    else                                                                              \
      raft_amd::launch_reduce_rows<OPC, double>(x.data_ptr<double>(), out.data_ptr<double>(), m, d, s); \
    break;
  switch (op) { CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5)
    default: TORCH_CHECK(false, "bad op code"); }
#undef CASE
  return out;
}

torch::Tensor reduce_cols(torch::Tensor x, int64_t op) {
  check_reduce_input(x, op, x.dim() == 2 ? x.size(0) : 1);
  auto out = torch::empty({x.size(1)}, x.options());
  auto s = cur_stream();
  const long long m = x.size(0), d = x.size(1);
#define CASE(OPC)                                                                     \
  case OPC:                                                                           \
    if (x.scalar_type() == torch::kFloat32)                                           \
      raft_amd::launch_reduce_cols<OPC, float>(x.data_ptr<float>(), out.data_ptr<float>(), m, d, s); \
    else                                                                              \
      raft_amd::launch_reduce_cols<OPC, double>(x.data_ptr<double>(), out.data_ptr<double>(), m, d, s); \
    break;
  switch (op) { CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5)
    default: TORCH_CHECK(false, "bad op code"); }
#undef CASE
  return out;
}

torch::Tensor rows_sqnorm_bf16(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 && x.is_contiguous()
              && x.dim() == 2);
  auto out = torch::empty({x.size(0)}, x.options().dtype(torch::kFloat32));
  raft_amd::launch_rows_sqnorm_bf16(x.data_ptr(), out.data_ptr<float>(), x.size(0),
                                    x.size(1), cur_stream());
  return out;
}

torch::Tensor row_argmin(torch::Tensor x) {
  check_f32_2d(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kFloat32, "x must be float32");
  TORCH_CHECK(x.size(1) > 0 && x.size(1) <= 2147483647LL,
              "argmin needs 1 <= row length < 2^31");
  auto out = torch::empty({x.size(0)}, x.options().dtype(torch::kInt32));
  raft_amd::launch_row_argmin(x.data_ptr<float>(), out.data_ptr<int>(), x.size(0),
                              x.size(1), cur_stream());
  return out;
}

torch::Tensor row_normalize_l2(torch::Tensor x, double eps) {
  check_f32_2d(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kFloat32, "x must be float32");
  auto out = torch::empty_like(x);
  raft_amd::launch_row_normalize_l2(x.data_ptr<float>(), out.data_ptr<float>(),
                                    x.size(0), x.size(1), (float)eps, cur_stream());
  return out;
}

torch::Tensor l2_epilogue_(torch::Tensor g, torch::Tensor xn, torch::Tensor yn) {
  check_f32_2d(g, "g");
  raft_amd::launch_l2_epilogue(g.data_ptr<float>(), xn.data_ptr<float>(),
                               yn.data_ptr<float>(), g.size(0), g.size(1), cur_stream());
  return g;
}

void l2nn_epilogue(torch::Tensor g, torch::Tensor xn, torch::Tensor yn,
                   torch::Tensor dmin, torch::Tensor amin) {
  check_f32_2d(g, "g");
  raft_amd::launch_l2nn_epilogue(g.data_ptr<float>(), xn.data_ptr<float>(),
                                 yn.data_ptr<float>(), dmin.data_ptr<float>(),
                                 amin.data_ptr<int>(), g.size(0), g.size(1), cur_stream());
}

torch::Tensor pairwise_unexpanded(torch::Tensor x, torch::Tensor y, int64_t code,
                                  double p) {
  check_f32_2d(x, "x");
  check_f32_2d(y, "y");
  auto out = torch::empty({x.size(0), y.size(0)}, x.options());
  raft_amd::launch_pairwise_unexpanded(x.data_ptr<float>(), y.data_ptr<float>(),
                                       out.data_ptr<float>(), x.size(0), y.size(0),
                                       x.size(1), (int)code, (float)p, cur_stream());
  return out;
}

torch::Tensor pairwise_expanded_epilogue_(torch::Tensor g, torch::Tensor xa,
                                         torch::Tensor ya, int64_t code, double d) {
  check_f32_2d(g, "g");
  TORCH_CHECK(g.scalar_type() == torch::kFloat32, "g must be float32");
  TORCH_CHECK(code >= 0 && code <= 3, "bad expanded-epilogue code ", code);
  const bool norms = code >= 2;  // Jaccard / Dice read the row norms
  for (const auto* t : {&xa, &ya}) {
    TORCH_CHECK(t->is_cuda() && t->device() == g.device(), "xa/ya must be on g's device");
    TORCH_CHECK(t->scalar_type() == torch::kFloat32, "xa/ya must be float32");
    TORCH_CHECK(t->dim() == 1 && t->is_contiguous(), "xa/ya must be contiguous 1-D");
  }
  if (norms) {
    TORCH_CHECK(xa.size(0) == g.size(0), "xa must have g.size(0) entries");
    TORCH_CHECK(ya.size(0) == g.size(1), "ya must have g.size(1) entries");
  }
  if (code == 1) TORCH_CHECK(d > 0, "Russel-Rao needs d > 0");
  raft_amd::launch_pairwise_expanded_epilogue(
      g.data_ptr<float>(), norms ? xa.data_ptr<float>() : nullptr,
      norms ? ya.data_ptr<float>() : nullptr, g.size(0), g.size(1), (int)code,
      (float)d, cur_stream());
  return g;
}

torch::Tensor rng_uniform(int64_t n, int64_t seed, int64_t subseq, int64_t device,
                          int64_t gen = 0) {
  auto out = torch::empty({n}, torch::dtype(torch::kFloat32).device(torch::kCUDA, device));
  raft_amd::launch_rng_uniform(out.data_ptr<float>(), n, (uint64_t)seed,
                               (uint64_t)subseq, cur_stream(), (int)gen);
  return out;
}

torch::Tensor rng_normal(int64_t n, int64_t seed, int64_t subseq, int64_t device,
                         int64_t gen = 0) {
  auto out = torch::empty({n}, torch::dtype(torch::kFloat32).device(torch::kCUDA, device));
  raft_amd::launch_rng_normal(out.data_ptr<float>(), n, (uint64_t)seed,
                              (uint64_t)subseq, cur_stream(), (int)gen);
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> make_blobs(int64_t n_rows, int64_t d,
                                                    torch::Tensor centers, double std_,
                                                    int64_t seed, int64_t subseq) {
  check_f32_2d(centers, "centers");
  auto x = torch::empty({n_rows, d}, centers.options());
  auto labels = torch::empty({n_rows}, centers.options().dtype(torch::kInt32));
  raft_amd::launch_make_blobs(x.data_ptr<float>(), labels.data_ptr<int>(),
                              centers.data_ptr<float>(), n_rows, d,
                              (int)centers.size(0), (float)std_, (uint64_t)seed,
                              (uint64_t)subseq, cur_stream());
  return {x, labels};
}

torch::Tensor csr_spmv(torch::Tensor indptr, torch::Tensor indices, torch::Tensor values,
                       torch::Tensor x, int64_t n_rows, int64_t n_cols) {
  // every tensor becomes a raw device pointer below: reject anything the
  // kernel could not dereference (column ids are the caller's contract)
  TORCH_CHECK(indptr.is_cuda() && indptr.scalar_type() == torch::kInt32 &&
              indptr.is_contiguous(), "indptr must be contiguous int32 on GPU");
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
              indices.is_contiguous(), "indices must be contiguous int32 on GPU");
  TORCH_CHECK(values.is_cuda() && values.is_contiguous() && values.dim() == 1,
              "values must be contiguous 1-D on GPU");
  TORCH_CHECK(values.scalar_type() == torch::kFloat32 ||
              values.scalar_type() == torch::kFloat64, "values must be float32 or float64");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 1,
              "x must be contiguous 1-D on GPU");
  TORCH_CHECK(x.scalar_type() == values.scalar_type(), "x must have the dtype of values");
  TORCH_CHECK(indptr.device() == values.device() && indices.device() == values.device() &&
              x.device() == values.device(), "all operands must be on one device");
  TORCH_CHECK(n_rows >= 0 && indptr.numel() == n_rows + 1, "indptr must have n_rows + 1 entries");
  TORCH_CHECK(indices.numel() == values.numel(), "indices and values must have equal length");
  TORCH_CHECK(n_cols < 0 || x.numel() == n_cols, "x must have n_cols entries");
  TORCH_CHECK(values.numel() == 0 || x.numel() > 0, "x is empty but the matrix is not");
  auto y = torch::empty({n_rows}, values.options());
  if (values.scalar_type() == torch::kFloat32) {
    raft_amd::launch_csr_spmv<float>(indptr.data_ptr<int>(), indices.data_ptr<int>(),
                                     values.data_ptr<float>(), x.data_ptr<float>(),
                                     y.data_ptr<float>(), n_rows, values.numel(),
                                     cur_stream());
  } else {
    raft_amd::launch_csr_spmv<double>(indptr.data_ptr<int>(), indices.data_ptr<int>(),
                                      values.data_ptr<double>(), x.data_ptr<double>(),
                                      y.data_ptr<double>(), n_rows, values.numel(),
                                      cur_stream());
  }
  return y;
}

void check_csr_f32(const torch::Tensor& indptr, const torch::Tensor& indices,
                   const torch::Tensor& values, int64_t n_rows, const char* name) {
  TORCH_CHECK(indptr.is_cuda() && indices.is_cuda() && values.is_cuda(), name,
              " must be on GPU");
  TORCH_CHECK(indptr.scalar_type() == torch::kInt32 &&
              indices.scalar_type() == torch::kInt32, name, " indices must be int32");
  TORCH_CHECK(values.scalar_type() == torch::kFloat32, name, " values must be fp32");
  TORCH_CHECK(indptr.is_contiguous() && indices.is_contiguous() && values.is_contiguous(),
              name, " must be contiguous");
  TORCH_CHECK(n_rows >= 0 && indptr.numel() == n_rows + 1, name,
              " indptr must have n_rows + 1 entries");
  TORCH_CHECK(indices.numel() == values.numel(), name, " indices / values differ in length");
}

// [n_rows, 2] fp32 row statistics of a CSR matrix for a sparse metric code
torch::Tensor csr_row_stats(torch::Tensor indptr, torch::Tensor indices, torch::Tensor values,
                            int64_t n_rows, int64_t metric, double p) {
  check_csr_f32(indptr, indices, values, n_rows, "csr");
  auto stats = torch::zeros({n_rows, 2}, values.options());
  raft_amd::launch_csr_row_stats(indptr.data_ptr<int>(), values.data_ptr<float>(),
                                 stats.data_ptr<float>(), n_rows, values.numel(),
                                 (int)metric, (float)p, cur_stream());
  return stats;
}

// [m, n] fp32 distances between the rows of two CSR matrices over d columns
torch::Tensor csr_pairwise(torch::Tensor a_indptr, torch::Tensor a_indices,
                           torch::Tensor a_values, int64_t m, torch::Tensor b_indptr,
                           torch::Tensor b_indices, torch::Tensor b_values, int64_t n,
                           torch::Tensor a_stats, torch::Tensor b_stats, int64_t d,
                           int64_t metric, double p, int64_t strategy, int64_t param) {
  check_csr_f32(a_indptr, a_indices, a_values, m, "a");
  check_csr_f32(b_indptr, b_indices, b_values, n, "b");
  TORCH_CHECK(a_stats.is_cuda() && a_stats.is_contiguous() && a_stats.numel() == 2 * m &&
              a_stats.scalar_type() == torch::kFloat32, "a_stats must be [m, 2] fp32");
  TORCH_CHECK(b_stats.is_cuda() && b_stats.is_contiguous() && b_stats.numel() == 2 * n &&
              b_stats.scalar_type() == torch::kFloat32, "b_stats must be [n, 2] fp32");
  auto out = torch::empty({m, n}, a_values.options());
  raft_amd::launch_csr_pairwise(
      a_indptr.data_ptr<int>(), a_indices.data_ptr<int>(), a_values.data_ptr<float>(), m,
      a_values.numel(), b_indptr.data_ptr<int>(), b_indices.data_ptr<int>(),
      b_values.data_ptr<float>(), n, b_values.numel(), a_stats.data_ptr<float>(),
      b_stats.data_ptr<float>(), out.data_ptr<float>(), d, (int)metric, (float)p,
      (int)strategy, (int)param, cur_stream());
  return out;
}

torch::Tensor reduce_rows_by_key_sorted(torch::Tensor x, torch::Tensor perm,
                                        torch::Tensor keys_sorted, int64_t n_keys) {
  check_f32_2d(x, "x");
  TORCH_CHECK(perm.scalar_type() == torch::kInt32 && perm.is_contiguous());
  TORCH_CHECK(keys_sorted.scalar_type() == torch::kInt32 && keys_sorted.is_contiguous());
  auto sums = torch::zeros({n_keys, x.size(1)}, x.options());
  raft_amd::launch_reduce_rows_by_key_sorted(x.data_ptr<float>(), perm.data_ptr<int>(),
                                             keys_sorted.data_ptr<int>(),
                                             sums.data_ptr<float>(), nullptr,
                                             nullptr, nullptr,
                                             x.size(0), x.size(1), cur_stream());
  return sums;
}

void reduce_rows_by_key_sorted_into(torch::Tensor x, torch::Tensor perm,
                                    torch::Tensor keys_sorted, torch::Tensor sums,
                                    torch::Tensor counts,
                                    c10::optional<torch::Tensor> dmin,
                                    c10::optional<torch::Tensor> inertia_acc) {
  check_f32_2d(x, "x");
  TORCH_CHECK(perm.scalar_type() == torch::kInt32 && keys_sorted.scalar_type() == torch::kInt32);
  TORCH_CHECK(sums.is_contiguous() && counts.is_contiguous());
  raft_amd::launch_reduce_rows_by_key_sorted(
      x.data_ptr<float>(), perm.data_ptr<int>(), keys_sorted.data_ptr<int>(),
      sums.data_ptr<float>(), counts.data_ptr<float>(),
      dmin.has_value() ? dmin->data_ptr<float>() : nullptr,
      inertia_acc.has_value() ? inertia_acc->data_ptr<float>() : nullptr,
      x.size(0), x.size(1), cur_stream());
}

void split_bf16_norms(torch::Tensor c, std::vector<torch::Tensor> slices,
                      torch::Tensor cn,
                      c10::optional<torch::Tensor> cn_max = c10::nullopt) {
  check_f32_2d(c, "c");
  const int nslice = (int)slices.size();
  TORCH_CHECK(nslice >= 1 && nslice <= 3);
  for (auto& s : slices)
    TORCH_CHECK(s.scalar_type() == torch::kBFloat16 && s.is_contiguous()
                && s.sizes() == c.sizes());
  void* p0 = slices[0].data_ptr();
  void* p1 = nslice > 1 ? slices[1].data_ptr() : p0;
  void* p2 = nslice > 2 ? slices[2].data_ptr() : p0;
  raft_amd::launch_split_bf16_norms(
      c.data_ptr<float>(), p0, p1, p2, cn.data_ptr<float>(), nslice, c.size(0),
      c.size(1), cur_stream(),
      cn_max.has_value() ? cn_max->data_ptr<float>() : nullptr);
}

void kmeans_update_verify(torch::Tensor x, torch::Tensor perm,
                          torch::Tensor keys_sorted, torch::Tensor c,
                          torch::Tensor xn, torch::Tensor dmin, torch::Tensor amin,
                          torch::Tensor dmin2, torch::Tensor cn_max,
                          torch::Tensor sums, torch::Tensor counts,
                          c10::optional<torch::Tensor> inertia_acc,
                          double lead, double tail) {
  check_f32_2d(x, "x");
  check_f32_2d(c, "c");
  // the widest kernel instance holds 16 columns per lane: past 64 * 16 the
  // remaining columns would be dropped from sums, distances and rescans
  TORCH_CHECK(x.size(1) <= 1024, "kmeans_update_verify: d = ", x.size(1),
              " exceeds the 1024 columns the kernel covers");
  TORCH_CHECK(perm.scalar_type() == torch::kInt32 && keys_sorted.scalar_type() == torch::kInt32);
  TORCH_CHECK(sums.is_contiguous() && counts.is_contiguous());
  raft_amd::launch_kmeans_update_verify(
      x.data_ptr<float>(), perm.data_ptr<int>(), keys_sorted.data_ptr<int>(),
      c.data_ptr<float>(), xn.data_ptr<float>(), dmin.data_ptr<float>(),
      amin.data_ptr<int>(), dmin2.data_ptr<float>(), cn_max.data_ptr<float>(),
      sums.data_ptr<float>(), counts.data_ptr<float>(),
      inertia_acc.has_value() ? inertia_acc->data_ptr<float>() : nullptr,
      x.size(0), x.size(1), (int)c.size(0), cur_stream(), (float)lead,
      (float)tail);
}

void kmeans_update_centroids(torch::Tensor sums, torch::Tensor counts,
                             torch::Tensor centroids) {
  check_f32_2d(centroids, "centroids");
  raft_amd::launch_kmeans_update_centroids(sums.data_ptr<float>(),
                                           counts.data_ptr<float>(),
                                           centroids.data_ptr<float>(),
                                           centroids.size(0), centroids.size(1),
                                           cur_stream());
}

torch::Tensor reduce_rows_by_key(torch::Tensor x, torch::Tensor keys, int64_t n_keys) {
  check_f32_2d(x, "x");
  TORCH_CHECK(keys.scalar_type() == torch::kInt32);
  const long long kd = n_keys * x.size(1);
  // replica count: bound the workspace at ~32 MB, contention drop ~= replicas
  int replicas = (int)std::min<long long>(16, std::max<long long>(1, (32ll << 20) / (kd * 4)));
  auto work = torch::zeros({replicas, n_keys, x.size(1)}, x.options());
  auto sums = torch::empty({n_keys, x.size(1)}, x.options());
  raft_amd::launch_reduce_rows_by_key(x.data_ptr<float>(), keys.data_ptr<int>(),
                                      work.data_ptr<float>(), sums.data_ptr<float>(),
                                      x.size(0), x.size(1), n_keys, replicas,
                                      cur_stream());
  return sums;
}

std::tuple<torch::Tensor, torch::Tensor> select_k_generic(
    torch::Tensor x, c10::optional<torch::Tensor> row_off, int64_t k,
    bool select_min) {
  // x: [batch, len] dense, or flat [nnz] values with row_off [batch+1]
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  long long batch, stride, len_fixed;
  const long long* ro = nullptr;
  torch::Tensor ro_t;
  if (row_off.has_value()) {
    ro_t = row_off.value();
    TORCH_CHECK(ro_t.is_cuda() && ro_t.scalar_type() == torch::kInt64 &&
                ro_t.is_contiguous() && x.dim() == 1);
    batch = ro_t.numel() - 1;
    stride = 0;
    len_fixed = 0;
    ro = reinterpret_cast<const long long*>(ro_t.data_ptr<int64_t>());
  } else {
    TORCH_CHECK(x.dim() == 2);
    batch = x.size(0);
    stride = len_fixed = x.size(1);
  }
  auto out_v = torch::empty({batch, k}, x.options());
  auto out_i = torch::empty({batch, k}, x.options().dtype(torch::kInt64));
  auto* oi = reinterpret_cast<long long*>(out_i.data_ptr<int64_t>());
  switch (x.scalar_type()) {
    case torch::kFloat32:
      raft_amd::launch_select_k_generic_t<float>(
          x.data_ptr<float>(), ro, stride, len_fixed, out_v.data_ptr<float>(),
          oi, batch, k, select_min, cur_stream());
      break;
    case torch::kFloat64:
      raft_amd::launch_select_k_generic_t<double>(
          x.data_ptr<double>(), ro, stride, len_fixed,
          out_v.data_ptr<double>(), oi, batch, k, select_min, cur_stream());
      break;
    case torch::kBFloat16:
      raft_amd::launch_select_k_generic_t<__bf16>(
          reinterpret_cast<const __bf16*>(x.data_ptr<at::BFloat16>()), ro,
          stride, len_fixed, reinterpret_cast<__bf16*>(out_v.data_ptr<at::BFloat16>()),
          oi, batch, k, select_min, cur_stream());
      break;
    case torch::kHalf:
      raft_amd::launch_select_k_generic_t<_Float16>(
          reinterpret_cast<const _Float16*>(x.data_ptr<at::Half>()), ro,
          stride, len_fixed, reinterpret_cast<_Float16*>(out_v.data_ptr<at::Half>()),
          oi, batch, k, select_min, cur_stream());
      break;
    default:
      TORCH_CHECK(false, "select_k_generic: fp32/fp64/bf16/fp16 only");
  }
  return {out_v, out_i};
}

std::tuple<torch::Tensor, torch::Tensor> select_k(torch::Tensor x, int64_t k,
                                                  bool select_min, int64_t algo,
                                                  bool do_sort) {
  check_f32_2d(x, "x");
  auto vals = torch::empty({x.size(0), k}, x.options());
  auto idx = torch::empty({x.size(0), k}, x.options().dtype(torch::kInt32));
  // algo: 0 auto, 1 radix, 2 warpsort (k <= 64, wave-register queue)
  if (k <= 64 && algo == 2) {
    raft_amd::launch_select_k_warpsort(x.data_ptr<float>(), vals.data_ptr<float>(),
                                       idx.data_ptr<int>(), x.size(0), x.size(1),
                                       (int)k, select_min, cur_stream());
    return {vals, idx};
  }
  auto ws = torch::empty({raft_amd::select_k_workspace_bytes(x.size(0))},
                         x.options().dtype(torch::kUInt8));
  raft_amd::launch_select_k(x.data_ptr<float>(), vals.data_ptr<float>(),
                            idx.data_ptr<int>(), ws.data_ptr(), x.size(0), x.size(1),
                            (int)k, select_min, do_sort, cur_stream());
  return {vals, idx};
}

// "auto" -> Auto; an unknown name is an error, never a fallback
static raft_amd::L2nnEngine l2nn_engine_arg(const std::string& engine) {
  bool known;
  const auto e = raft_amd::l2nn_engine_from_name(engine, &known);
  TORCH_CHECK(known, "fused_l2nn: unknown engine '", engine, "'");
  return e;
}

static raft_amd::L2nnPlan l2nn_plan(int64_t nslice, int64_t m, int64_t n, int64_t d,
                                    const std::string& engine, int64_t gt) {
  TORCH_CHECK(nslice >= 1 && nslice <= 3, "fused_l2nn: 1 to 3 slices");
  TORCH_CHECK(n % 128 == 0, "fused_l2nn: n must be a multiple of 128");
  TORCH_CHECK(d % 64 == 0, "fused_l2nn: d must be a multiple of 64");
  TORCH_CHECK(gt == 0 || gt == 1 || gt == 2 || gt == 4 || gt == 8,
              "fused_l2nn: gt must be 0 (default), 1, 2, 4 or 8");
  auto plan = raft_amd::l2nn_resolve_engine((int)nslice, m, (int)n, (int)d,
                                            l2nn_engine_arg(engine), (int)gt);
  TORCH_CHECK(plan.error.empty(), plan.error, " (nslice=", nslice, ", m=", m,
              ", n=", n, ", d=", d, ")");
  return plan;
}

// (engine name, gt) that fused_l2nn_split runs for this shape and request
std::tuple<std::string, int64_t> l2nn_resolve_engine(int64_t nslice, int64_t m,
                                                     int64_t n, int64_t d,
                                                     const std::string& engine,
                                                     int64_t gt) {
  const auto plan = l2nn_plan(nslice, m, n, d, engine, gt);
  return {raft_amd::l2nn_engine_name(plan.engine), plan.gt};
}

// the split-bf16 operands of one call: checked slice lists and their shape
struct SliceArgs {
  const void* xsl[3];
  const void* csl[3];
  int nslice;
  long long m, n, d;
};

// 1 to max_nslice bf16 slices per side, equal counts; every slice a contiguous
// 2-D GPU tensor with the sizes of slice 0 of its list; x and y of equal d, a
// multiple of 64 (the launchers index every slice with these sizes)
static SliceArgs checked_slices(const char* who, const std::vector<torch::Tensor>& x_slices,
                                const std::vector<torch::Tensor>& y_slices,
                                int max_nslice) {
  SliceArgs a;
  a.nslice = (int)x_slices.size();
  TORCH_CHECK(a.nslice >= 1 && a.nslice <= max_nslice && y_slices.size() == x_slices.size(),
              who, ": x and y need the same number of slices, 1 to ", max_nslice);
  for (int s = 0; s < a.nslice; s++) {
    for (const auto* list : {&x_slices, &y_slices}) {
      const auto& t = (*list)[s];
      TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.dim() == 2 &&
                  t.is_contiguous() && t.sizes() == (*list)[0].sizes(),
                  who, ": every slice must be a contiguous bf16 [rows, d] GPU tensor "
                  "with the sizes of slice 0");
    }
    a.xsl[s] = x_slices[s].data_ptr();
    a.csl[s] = y_slices[s].data_ptr();
  }
  a.m = x_slices[0].size(0);
  a.n = y_slices[0].size(0);
  a.d = x_slices[0].size(1);
  TORCH_CHECK(y_slices[0].size(1) == a.d, who, ": x and y slices must have the same d");
  TORCH_CHECK(a.d % 64 == 0, who, ": d must be a multiple of 64");
  return a;
}

// row norms and their like: a contiguous fp32 GPU tensor of numel elements
static const float* checked_f32_vec(const char* who, const char* what,
                                    const torch::Tensor& t, long long numel) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
              t.numel() == numel, who, ": ", what,
              " must be a contiguous fp32 GPU tensor of ", numel, " elements");
  return t.data_ptr<float>();
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> fused_l2nn_split(
    std::vector<torch::Tensor> x_slices, std::vector<torch::Tensor> c_slices,
    torch::Tensor xn, torch::Tensor cn, const std::string& engine, int64_t gt) {
  SliceArgs a = checked_slices("fused_l2nn_split", x_slices, c_slices, 3);
  const long long m = a.m, n = a.n, d = a.d;
  const auto plan = l2nn_plan(a.nslice, m, n, d, engine, gt);
  const float* xnp = checked_f32_vec("fused_l2nn_split", "xn", xn, m);
  const float* cnp = checked_f32_vec("fused_l2nn_split", "cn", cn, n);
  auto dmin = torch::empty({m}, xn.options());
  auto amin = torch::empty({m}, xn.options().dtype(torch::kInt32));
  auto dmin2 = torch::empty({m}, xn.options());
  // per-(row, col-tile group) partials of the 2d and 256 engines
  auto pd = torch::empty({plan.n_groups * m}, xn.options());
  auto pd2 = torch::empty({plan.n_groups * m}, xn.options());
  auto pi = torch::empty({plan.n_groups * m}, xn.options().dtype(torch::kInt32));
  raft_amd::launch_fused_l2nn(plan, a.xsl, a.csl, xnp, cnp, pd.data_ptr<float>(),
                              pd2.data_ptr<float>(), pi.data_ptr<int>(),
                              dmin.data_ptr<float>(), amin.data_ptr<int>(),
                              dmin2.data_ptr<float>(), m, (int)n, (int)d, a.nslice,
                              cur_stream());
  return {dmin, amin, dmin2};
}

// one pairwise L2 call: checked bf16 slices, shape, and the kernel `variant`
// resolves to ("auto" -> environment and defaults; an unknown name or a named
// variant that cannot run the shape is an error, never a fallback)
struct PwCall : SliceArgs {
  const float* xn;
  const float* yn;
  raft_amd::PwPlan plan;
};

static PwCall pw_call(raft_amd::PwFamily family, const char* who,
                      const std::vector<torch::Tensor>& x_slices,
                      const std::vector<torch::Tensor>& y_slices,
                      const torch::Tensor& xn, const torch::Tensor& yn,
                      const std::string& variant) {
  PwCall c;
  static_cast<SliceArgs&>(c) = checked_slices(who, x_slices, y_slices, 3);
  c.xn = checked_f32_vec(who, "xn", xn, c.m);
  c.yn = checked_f32_vec(who, "yn", yn, c.n);
  bool known;
  const auto v = raft_amd::pw_variant_from_name(family, variant, &known);
  TORCH_CHECK(known, who, ": unknown variant '", variant, "'");
  c.plan = raft_amd::pw_resolve_variant(family, c.nslice, c.m, c.n, (int)c.d, v);
  TORCH_CHECK(c.plan.error.empty(), c.plan.error, " (nslice=", c.nslice, ", m=", c.m,
              ", n=", c.n, ", d=", c.d, ")");
  return c;
}

torch::Tensor pairwise_l2_mfma(std::vector<torch::Tensor> x_slices,
                               std::vector<torch::Tensor> y_slices,
                               torch::Tensor xn, torch::Tensor yn,
                               c10::optional<torch::Tensor> out, bool sqrt_out,
                               const std::string& variant) {
  PwCall c = pw_call(raft_amd::PwFamily::Tile, "pairwise_l2_mfma", x_slices,
                     y_slices, xn, yn, variant);
  torch::Tensor o;
  if (out.has_value()) {
    o = out.value();
    TORCH_CHECK(o.is_contiguous() && o.size(0) >= c.m && o.size(1) == c.n);
  } else {
    o = torch::empty({c.m, c.n}, xn.options());
  }
  raft_amd::launch_pairwise_l2_tile(c.plan, c.xsl, c.csl, c.xn, c.yn,
                                    o.data_ptr<float>(), c.m, c.n,
                                    (int)c.d, o.size(1), c.nslice, sqrt_out,
                                    cur_stream());
  return o;
}

void l2nn_verify_repair(torch::Tensor x, torch::Tensor c, torch::Tensor xn,
                        torch::Tensor dmin, torch::Tensor amin, torch::Tensor dmin2,
                        torch::Tensor cn_max, double lead, double tail) {
  check_f32_2d(x, "x");
  check_f32_2d(c, "c");
  TORCH_CHECK(cn_max.scalar_type() == torch::kFloat32 && cn_max.numel() >= 1);
  raft_amd::launch_l2nn_verify_repair(x.data_ptr<float>(), c.data_ptr<float>(),
                                      xn.data_ptr<float>(), dmin.data_ptr<float>(),
                                      amin.data_ptr<int>(), dmin2.data_ptr<float>(),
                                      cn_max.data_ptr<float>(), x.size(0),
                                      (int)c.size(0), (int)x.size(1), cur_stream(),
                                      (float)lead, (float)tail);
}

void pairwise_l2_filter(std::vector<torch::Tensor> x_slices,
                        std::vector<torch::Tensor> y_slices, torch::Tensor xn,
                        torch::Tensor yn, torch::Tensor thr, torch::Tensor out_d,
                        torch::Tensor out_i, torch::Tensor cnt, int64_t col_offset,
                        const std::string& variant) {
  PwCall c = pw_call(raft_amd::PwFamily::Filter, "pairwise_l2_filter", x_slices,
                     y_slices, xn, yn, variant);
  const int cap = (int)out_d.size(1);
  TORCH_CHECK(out_d.size(0) == c.m && out_i.sizes() == out_d.sizes());
  TORCH_CHECK(cnt.scalar_type() == torch::kInt32 && cnt.numel() == c.m);
  raft_amd::launch_pairwise_l2_filter(c.plan, c.xsl, c.csl, c.xn, c.yn,
                                      thr.data_ptr<float>(),
                                      out_d.data_ptr<float>(), out_i.data_ptr<int>(),
                                      cnt.data_ptr<int>(), cap, col_offset, c.m, c.n,
                                      (int)c.d, c.nslice, cur_stream());
}

const unsigned int* bitmap_words(const torch::Tensor& bm, const char* who) {
  TORCH_CHECK(bm.is_cuda() && bm.scalar_type() == torch::kInt32 && bm.dim() == 2 &&
              bm.is_contiguous(), who, ": bitmap must be a contiguous int32 [m, words] GPU tensor");
  return reinterpret_cast<const unsigned int*>(bm.data_ptr<int>());
}

// packed eps-neighborhood bitmap of one row block (fills `bitmap` in place).
// xf/yf present -> verified fp32 engine (exact recheck of the band pairs,
// counted into `rechecked`); absent -> single bf16 slice decided by the score.
void eps_neighbors_l2sq(std::vector<torch::Tensor> x_slices,
                        std::vector<torch::Tensor> y_slices, torch::Tensor xn,
                        torch::Tensor yn, c10::optional<torch::Tensor> xf,
                        c10::optional<torch::Tensor> yf, torch::Tensor bitmap,
                        c10::optional<torch::Tensor> rechecked, int64_t n_cols,
                        double eps_sq, double lead, double tail) {
  SliceArgs a = checked_slices("eps_neighbors_l2sq", x_slices, y_slices, 2);
  const int nslice = a.nslice;
  const long long m = a.m, n = a.n, d = a.d;
  TORCH_CHECK(n == n_cols, "eps_neighbors_l2sq: y slices must have n_cols rows");
  TORCH_CHECK(n < (1ll << 31) && m < (1ll << 31), "eps_neighbors_l2sq: m, n < 2^31");
  const float* xnp = checked_f32_vec("eps_neighbors_l2sq", "xn", xn, m);
  const float* ynp = checked_f32_vec("eps_neighbors_l2sq", "yn", yn, n);
  const float eps2 = (float)eps_sq;
  TORCH_CHECK(eps2 >= 0.f && eps2 <= std::numeric_limits<float>::max(),
              "eps_neighbors_l2sq: eps_sq must be finite and >= 0");
  const long long n_words = (n + 31) / 32;
  unsigned int* bm = const_cast<unsigned int*>(bitmap_words(bitmap, "eps_neighbors_l2sq"));
  TORCH_CHECK(bitmap.size(0) == m && bitmap.size(1) == n_words,
              "eps_neighbors_l2sq: bitmap must be [m, ceil(n/32)]");
  const float* xfp = nullptr;
  const float* yfp = nullptr;
  unsigned long long* cnt = nullptr;
  long long df = d;
  TORCH_CHECK(xf.has_value() == yf.has_value());
  if (xf.has_value()) {
    check_f32_2d(xf.value(), "xf");
    check_f32_2d(yf.value(), "yf");
    TORCH_CHECK(xf.value().scalar_type() == torch::kFloat32 &&
                yf.value().scalar_type() == torch::kFloat32);
    df = xf.value().size(1);
    TORCH_CHECK(xf.value().size(0) == m && yf.value().size(0) == n &&
                yf.value().size(1) == df && df <= d,
                "eps_neighbors_l2sq: xf/yf shapes must match the slices");
    TORCH_CHECK(rechecked.has_value() && rechecked.value().is_cuda() &&
                rechecked.value().scalar_type() == torch::kInt64 &&
                rechecked.value().numel() >= 1,
                "eps_neighbors_l2sq: the verified engine needs an int64 counter");
    xfp = xf.value().data_ptr<float>();
    yfp = yf.value().data_ptr<float>();
    cnt = reinterpret_cast<unsigned long long*>(rechecked.value().data_ptr<int64_t>());
  } else {
    TORCH_CHECK(nslice == 1, "eps_neighbors_l2sq: 2 slices need the fp32 recheck");
  }
  raft_amd::launch_eps_neighbors_l2sq(a.xsl, a.csl, xnp, ynp, xfp, yfp, bm, cnt, eps2,
                                      (float)lead, (float)tail, m, n, (int)d, (int)df,
                                      n_words, nslice, cur_stream());
}

static const int* masked_nn_i32(const c10::optional<torch::Tensor>& t, long long numel,
                                const char* what) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t.value().is_cuda() && t.value().scalar_type() == torch::kInt32 &&
              t.value().is_contiguous() && t.value().numel() == numel,
              "masked_l2nn: ", what, " must be a contiguous int32 GPU vector of ",
              numel, " elements");
  return t.value().data_ptr<int>();
}

static const unsigned int* masked_nn_adj(const c10::optional<torch::Tensor>& adj,
                                         long long m, long long n_groups,
                                         long long* words) {
  *words = 0;
  if (!adj.has_value()) return nullptr;
  const unsigned int* p = bitmap_words(adj.value(), "masked_l2nn");
  TORCH_CHECK(adj.value().size(0) == m && adj.value().size(1) == (n_groups + 31) / 32,
              "masked_l2nn: adj must be [m, ceil(n_groups/32)]");
  *words = adj.value().size(1);
  return p;
}

// masked fused L2-NN over one row block. y_group holds ids in [0, n_groups),
// non-decreasing (the Python layer builds it from the group offsets). scratch
// is float32 [3, n_split, m]: the per-split partial (best, second, index).
// counters is int64 [2]: visited and skipped tiles are ADDED to it.
std::vector<torch::Tensor> masked_l2nn(std::vector<torch::Tensor> x_slices,
                                       std::vector<torch::Tensor> y_slices,
                                       torch::Tensor xn, torch::Tensor yn,
                                       torch::Tensor y_group, int64_t n_groups,
                                       c10::optional<torch::Tensor> adj,
                                       c10::optional<torch::Tensor> x_group,
                                       torch::Tensor scratch, torch::Tensor counters) {
  SliceArgs a = checked_slices("masked_l2nn", x_slices, y_slices, 2);
  const long long m = a.m, n = a.n, d = a.d;
  TORCH_CHECK(m >= 1 && n >= 1, "masked_l2nn: empty inputs are handled by the caller");
  TORCH_CHECK(d > 0, "masked_l2nn: d must be positive");
  TORCH_CHECK(n < (1ll << 31) - 128 && m < (1ll << 31), "masked_l2nn: m, n < 2^31");
  const float* xnp = checked_f32_vec("masked_l2nn", "xn", xn, m);
  const float* ynp = checked_f32_vec("masked_l2nn", "yn", yn, n);
  TORCH_CHECK(n_groups >= 1 && n_groups < (1ll << 31), "masked_l2nn: n_groups >= 1");
  const int* yg = masked_nn_i32(y_group, n, "y_group");
  const int* xg = masked_nn_i32(x_group, m, "x_group");
  long long adj_words = 0;
  const unsigned int* ap = masked_nn_adj(adj, m, n_groups, &adj_words);
  TORCH_CHECK(ap != nullptr || xg != nullptr, "masked_l2nn: adj or x_group is required");
  TORCH_CHECK(scratch.is_cuda() && scratch.scalar_type() == torch::kFloat32 &&
              scratch.is_contiguous() && scratch.dim() == 3 && scratch.size(0) == 3 &&
              scratch.size(2) == m,
              "masked_l2nn: scratch must be float32 [3, n_split, m]");
  const long long n_split = scratch.size(1);
  TORCH_CHECK(n_split >= 1 && n_split <= (n + 127) / 128,
              "masked_l2nn: n_split must be in [1, ceil(n/128)]");
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == torch::kInt64 &&
              counters.is_contiguous() && counters.numel() == 2,
              "masked_l2nn: counters must be int64 [2]");
  float* pd = scratch.data_ptr<float>();
  float* pd2 = pd + n_split * m;
  int* pi = reinterpret_cast<int*>(pd + 2 * n_split * m);
  auto dmin = torch::empty({(int64_t)m}, xn.options());
  auto dmin2 = torch::empty({(int64_t)m}, xn.options());
  auto amin = torch::empty({(int64_t)m}, xn.options().dtype(torch::kInt32));
  raft_amd::launch_masked_l2nn(
      a.xsl, a.csl, xnp, ynp, yg, ap, adj_words, xg, pd,
      pd2, pi, dmin.data_ptr<float>(), amin.data_ptr<int>(), dmin2.data_ptr<float>(),
      reinterpret_cast<unsigned long long*>(counters.data_ptr<int64_t>()), m, (int)n,
      (int)d, (int)n_split, a.nslice, cur_stream());
  return {dmin, amin, dmin2};
}

// exact fp32 verify / repair of a masked_l2nn result, in place. y_group is
// the int32 [n] group id of every y row (ids in [0, n_groups)); y_rank
// (optional int32 [n] permutation of 0..n-1) replaces the column index in the
// exact-tie rule of the rescan.
void masked_l2nn_verify_repair(torch::Tensor x, torch::Tensor y, torch::Tensor xn,
                               torch::Tensor y_group, int64_t n_groups,
                               c10::optional<torch::Tensor> adj,
                               c10::optional<torch::Tensor> x_group,
                               c10::optional<torch::Tensor> y_rank, torch::Tensor dmin,
                               torch::Tensor amin, torch::Tensor dmin2,
                               torch::Tensor yn_max, torch::Tensor rescanned,
                               double lead, double tail) {
  check_f32_2d(x, "x");
  check_f32_2d(y, "y");
  const long long m = x.size(0), n = y.size(0), df = x.size(1);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && y.scalar_type() == torch::kFloat32 &&
              y.size(1) == df && df >= 1, "masked_l2nn_verify_repair: x, y fp32 [*, d]");
  TORCH_CHECK(m >= 1 && m < (1ll << 31) && n >= 1 && n < (1ll << 31) - 2048 &&
              df < (1ll << 31), "masked_l2nn_verify_repair: 1 <= m, n < 2^31");
  TORCH_CHECK(n_groups >= 1, "masked_l2nn_verify_repair: at least one group");
  const int* yg = masked_nn_i32(y_group, n, "y_group");
  const int* xg = masked_nn_i32(x_group, m, "x_group");
  const int* yr = masked_nn_i32(y_rank, n, "y_rank");
  long long adj_words = 0;
  const unsigned int* ap = masked_nn_adj(adj, m, n_groups, &adj_words);
  TORCH_CHECK(ap != nullptr || xg != nullptr,
              "masked_l2nn_verify_repair: adj or x_group is required");
  for (const torch::Tensor* t : {&xn, &dmin, &dmin2})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 &&
                t->is_contiguous() && t->numel() == m,
                "masked_l2nn_verify_repair: xn, dmin, dmin2 must be float32 [m]");
  TORCH_CHECK(amin.is_cuda() && amin.scalar_type() == torch::kInt32 &&
              amin.is_contiguous() && amin.numel() == m);
  TORCH_CHECK(yn_max.is_cuda() && yn_max.scalar_type() == torch::kFloat32 &&
              yn_max.numel() >= 1);
  TORCH_CHECK(rescanned.is_cuda() && rescanned.scalar_type() == torch::kInt64 &&
              rescanned.numel() >= 1,
              "masked_l2nn_verify_repair: rescanned must be an int64 counter");
  // rescan list, its length and the per-row (distance, key) minimum
  auto i32 = xn.options().dtype(torch::kInt32);
  auto rows = torch::empty({(int64_t)m}, i32);
  auto count = torch::empty({1}, i32);
  auto keys = torch::empty({(int64_t)m}, xn.options().dtype(torch::kInt64));
  torch::Tensor inv;
  const int* ivp = nullptr;
  if (yr != nullptr) {
    // rank -> column; an out-of-range rank fails here, not in the kernel
    inv = torch::empty({(int64_t)n}, i32);
    inv.index_put_({y_rank.value().to(torch::kInt64)},
                   torch::arange((int64_t)n, i32));
    ivp = inv.data_ptr<int>();
  }
  raft_amd::launch_masked_l2nn_verify_repair(
      x.data_ptr<float>(), y.data_ptr<float>(), xn.data_ptr<float>(), yg, ap, adj_words,
      xg, yr, ivp, dmin.data_ptr<float>(), amin.data_ptr<int>(), dmin2.data_ptr<float>(),
      yn_max.data_ptr<float>(), rows.data_ptr<int>(),
      reinterpret_cast<unsigned int*>(count.data_ptr<int>()),
      reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(rescanned.data_ptr<int64_t>()), m, (int)n,
      (int)df, (float)lead, (float)tail, cur_stream());
}

static const long long* ivf_i64(const torch::Tensor& t, long long numel, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt64 && t.is_contiguous() &&
              t.numel() == numel,
              "ivf_flat_scan: ", what, " must be a contiguous int64 GPU tensor of ",
              numel, " elements");
  return reinterpret_cast<const long long*>(t.data_ptr<int64_t>());
}

// IVF-Flat list scan of one query chunk into the ragged candidate buffer
// `out` (filled in place; the caller pre-fills nothing: every padded row of
// every probed list is written). The item / pair arrays are built on the
// device by raft_amd/neighbors/ivf_flat.py; item_list.numel() is the grid's x
// bound and n_items the device scalar that says how many items are real.
void ivf_flat_scan(torch::Tensor data, torch::Tensor list_offsets, torch::Tensor indices,
                   torch::Tensor queries, torch::Tensor item_list,
                   torch::Tensor item_pair_begin, torch::Tensor item_pair_count,
                   torch::Tensor n_items, torch::Tensor pair_query,
                   torch::Tensor pair_out_off, c10::optional<torch::Tensor> filter_words,
                   int64_t filter_bits, torch::Tensor out, int64_t metric, int64_t qg,
                   int64_t y_split) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous() && data.dim() == 1 &&
              (data.scalar_type() == torch::kFloat32 ||
               data.scalar_type() == torch::kBFloat16),
              "ivf_flat_scan: data must be a flat contiguous fp32 or bf16 GPU tensor");
  const bool bf16 = data.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(queries.is_cuda() && queries.is_contiguous() && queries.dim() == 2 &&
              queries.scalar_type() == torch::kFloat32 && queries.size(1) >= 1,
              "ivf_flat_scan: queries must be contiguous fp32 [q, d]");
  const long long d = queries.size(1);
  const long long v = bf16 ? 8 : 4;
  const long long d_pad = (d + v - 1) / v * v;
  TORCH_CHECK(d_pad <= 4096, "ivf_flat_scan: d_pad must be <= 4096");
  const long long total_rows = indices.numel();
  TORCH_CHECK(total_rows % 64 == 0 && data.numel() == total_rows * d_pad,
              "ivf_flat_scan: data must hold indices.numel() rows of d_pad elements "
              "and the row count must be a multiple of 64");
  const long long n_lists = list_offsets.numel() - 1;
  TORCH_CHECK(n_lists >= 1, "ivf_flat_scan: list_offsets must be int64 [n_lists + 1]");
  const long long n_pairs = pair_query.numel();
  const long long max_items = item_list.numel();
  const long long* lo = ivf_i64(list_offsets, n_lists + 1, "list_offsets");
  const long long* idx = ivf_i64(indices, total_rows, "indices");
  const long long* il = ivf_i64(item_list, max_items, "item_list");
  const long long* ib = ivf_i64(item_pair_begin, max_items, "item_pair_begin");
  const long long* ic = ivf_i64(item_pair_count, max_items, "item_pair_count");
  const long long* ni = ivf_i64(n_items, 1, "n_items");
  const long long* pq = ivf_i64(pair_query, n_pairs, "pair_query");
  const long long* po = ivf_i64(pair_out_off, n_pairs, "pair_out_off");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 1 &&
              out.scalar_type() == torch::kFloat32,
              "ivf_flat_scan: out must be a flat contiguous fp32 GPU tensor");
  const unsigned int* fw = nullptr;
  if (filter_words.has_value()) {
    const torch::Tensor& f = filter_words.value();
    TORCH_CHECK(f.is_cuda() && f.scalar_type() == torch::kInt32 && f.is_contiguous() &&
                f.dim() == 1 && filter_bits >= 0 && f.numel() * 32 >= filter_bits,
                "ivf_flat_scan: filter must be int32 words covering filter_bits");
    fw = reinterpret_cast<const unsigned int*>(f.data_ptr<int>());
  }
  TORCH_CHECK(qg >= 1 && qg <= raft_amd::ivf_flat_scan_max_qg((int)d_pad),
              "ivf_flat_scan: qg too large for d_pad");
  raft_amd::launch_ivf_flat_scan(
      data.data_ptr(), bf16, lo, idx, queries.data_ptr<float>(), il, ib, ic, ni, pq, po,
      fw, filter_bits, out.data_ptr<float>(), out.numel(), n_lists, total_rows,
      queries.size(0), n_pairs, max_items, (int)d, (int)metric, (int)qg, (int)y_split,
      cur_stream());
}

void bitmap_row_degrees(torch::Tensor bitmap, torch::Tensor deg) {
  const unsigned int* bm = bitmap_words(bitmap, "bitmap_row_degrees");
  TORCH_CHECK(deg.is_cuda() && deg.scalar_type() == torch::kInt64 &&
              deg.is_contiguous() && deg.numel() == bitmap.size(0));
  raft_amd::launch_bitmap_row_degrees(bm, reinterpret_cast<long long*>(deg.data_ptr<int64_t>()),
                                      bitmap.size(0), bitmap.size(1), cur_stream());
}

void bitmap_rows_to_csr(torch::Tensor bitmap, torch::Tensor indptr,
                        torch::Tensor indices) {
  const unsigned int* bm = bitmap_words(bitmap, "bitmap_rows_to_csr");
  TORCH_CHECK(indptr.is_cuda() && indptr.scalar_type() == torch::kInt64 &&
              indptr.is_contiguous() && indptr.numel() == bitmap.size(0) + 1,
              "bitmap_rows_to_csr: indptr must be int64 [m+1]");
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
              indices.is_contiguous() && indices.dim() == 1,
              "bitmap_rows_to_csr: indices must be int32 [nnz]");
  TORCH_CHECK(bitmap.size(1) < (1ll << 26), "bitmap_rows_to_csr: n must be < 2^31");
  if (indices.numel() == 0) return;
  raft_amd::launch_bitmap_rows_to_csr(
      bm, reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>()),
      indices.data_ptr<int>(), bitmap.size(0), bitmap.size(1), cur_stream());
}

void bitmap_rows_expand(torch::Tensor bitmap, torch::Tensor out) {
  const unsigned int* bm = bitmap_words(bitmap, "bitmap_rows_expand");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBool && out.dim() == 2 &&
              out.is_contiguous() && out.size(0) == bitmap.size(0) &&
              (out.size(1) + 31) / 32 == bitmap.size(1),
              "bitmap_rows_expand: out must be bool [m, n] with ceil(n/32) words");
  raft_amd::launch_bitmap_rows_expand(bm, out.data_ptr<bool>(), bitmap.size(0),
                                      out.size(1), bitmap.size(1), cur_stream());
}

// backend toggle (reference parity: cublas vs cublasLt wrapper pair) —
// RAFT_AMD_GEMM_BACKEND=hipblaslt routes the bf16->f32 GEMMs through the
// hipBLASLt heuristic path (csrc/gemm_hipblaslt.cpp)
static bool use_hipblaslt() {
  static const bool on = [] {
    const char* e = getenv("RAFT_AMD_GEMM_BACKEND");
    return e && std::string(e) == "hipblaslt";
  }();
  return on;
}

torch::Tensor gemm_bf16_f32(torch::Tensor a, torch::Tensor b,
                            c10::optional<torch::Tensor> out, double beta) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 && a.is_contiguous());
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == torch::kBFloat16 && b.is_contiguous());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(0));
  torch::Tensor c;
  float bt = (float)beta;
  if (out.has_value()) {
    c = out.value();
    TORCH_CHECK(c.scalar_type() == torch::kFloat32 && c.is_contiguous());
  } else {
    c = torch::empty({a.size(0), b.size(1)},
                     a.options().dtype(torch::kFloat32));
    bt = 0.0f;
  }
  if (use_hipblaslt())
    raft_amd::gemm_bf16_f32_rowmajor_lt(a.data_ptr(), b.data_ptr(), c.data_ptr<float>(),
                                        a.size(0), b.size(1), a.size(1), bt,
                                        (void*)cur_stream());
  else
    raft_amd::gemm_bf16_f32_rowmajor(a.data_ptr(), b.data_ptr(), c.data_ptr<float>(),
                                     a.size(0), b.size(1), a.size(1), bt,
                                     (void*)cur_stream());
  return c;
}

torch::Tensor gemm_bf16_f32_nt(torch::Tensor a, torch::Tensor b,
                               c10::optional<torch::Tensor> out, double beta) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 && a.is_contiguous());
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == torch::kBFloat16 && b.is_contiguous());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1));
  torch::Tensor c;
  float bt = (float)beta;
  if (out.has_value()) {
    c = out.value();
    TORCH_CHECK(c.scalar_type() == torch::kFloat32 && c.is_contiguous());
  } else {
    c = torch::empty({a.size(0), b.size(0)}, a.options().dtype(torch::kFloat32));
    bt = 0.0f;
  }
  if (use_hipblaslt())
    raft_amd::gemm_bf16_f32_nt_rowmajor_lt(a.data_ptr(), b.data_ptr(), c.data_ptr<float>(),
                                           a.size(0), b.size(0), a.size(1), bt,
                                           (void*)cur_stream());
  else
    raft_amd::gemm_bf16_f32_nt_rowmajor(a.data_ptr(), b.data_ptr(), c.data_ptr<float>(),
                                        a.size(0), b.size(0), a.size(1), bt,
                                        (void*)cur_stream());
  return c;
}

torch::Tensor gemm_f32(torch::Tensor a, torch::Tensor b) {
  check_f32_2d(a, "a");
  check_f32_2d(b, "b");
  auto c = torch::empty({a.size(0), b.size(1)}, a.options());
  raft_amd::gemm_f32_rowmajor(a.data_ptr<float>(), b.data_ptr<float>(),
                              c.data_ptr<float>(), a.size(0), b.size(1), a.size(1),
                              0.0f, (void*)cur_stream());
  return c;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("reduce_rows", &reduce_rows, "rowwise reduction (op code)");
  m.def("lanczos_pre_", [](torch::Tensor u, torch::Tensor v_i,
                           c10::optional<torch::Tensor> v_prev,
                           c10::optional<torch::Tensor> beta,
                           torch::Tensor alpha_out) {
    raft_amd::launch_lanczos_pre(
        u.data_ptr<float>(), v_i.data_ptr<float>(),
        v_prev.has_value() ? v_prev->data_ptr<float>() : nullptr,
        beta.has_value() ? beta->data_ptr<float>() : nullptr,
        alpha_out.data_ptr<double>(), u.numel(), cur_stream());
  }, "fused: u -= beta*v_prev; alpha_out = dot(v_i, u)");
  m.def("lanczos_sub_alpha_", [](torch::Tensor u, torch::Tensor v_i,
                                 torch::Tensor alpha, torch::Tensor t_diag) {
    raft_amd::launch_lanczos_sub_alpha(u.data_ptr<float>(),
                                       v_i.data_ptr<float>(),
                                       alpha.data_ptr<double>(),
                                       t_diag.data_ptr<float>(), u.numel(),
                                       cur_stream());
  }, "fused: u -= alpha*v_i; t_diag[0] = alpha");
  m.def("lanczos_norm2_", [](torch::Tensor u, torch::Tensor norm2_out) {
    raft_amd::launch_lanczos_norm2(u.data_ptr<float>(),
                                   norm2_out.data_ptr<double>(), u.numel(),
                                   cur_stream());
  }, "norm2_out[0] = ||u||^2 (fp64 accumulate)");
  m.def("lanczos_normalize_", [](torch::Tensor u, torch::Tensor v_next,
                                 torch::Tensor norm2,
                                 c10::optional<torch::Tensor> t_up,
                                 c10::optional<torch::Tensor> t_dn,
                                 c10::optional<torch::Tensor> beta_out) {
    raft_amd::launch_lanczos_normalize(
        u.data_ptr<float>(), v_next.data_ptr<float>(),
        norm2.data_ptr<double>(),
        t_up.has_value() ? t_up->data_ptr<float>() : nullptr,
        t_dn.has_value() ? t_dn->data_ptr<float>() : nullptr,
        beta_out.has_value() ? beta_out->data_ptr<float>() : nullptr,
        u.numel(), cur_stream());
  }, "fused: v_next = u/||u||; t couplings = ||u||");
  m.def("lanczos_cycle_", [](torch::Tensor indptr, torch::Tensor indices,
                             torch::Tensor values, torch::Tensor v,
                             torch::Tensor t_mat, torch::Tensor u,
                             torch::Tensor w, torch::Tensor v_next,
                             torch::Tensor beta_out, torch::Tensor alpha_scal,
                             torch::Tensor norm_scal, int64_t start,
                             int64_t ncv) {
    // Whole ncv-step extension cycle driven from C++: the per-step python
    // dispatch (~1 ms/step measured at 10M rows) disappears — one host call
    // per restart cycle. Mirrors sparse/solver/lanczos.py _extend exactly:
    // SpMV, (arrowhead | beta-recurrence) + alpha dot, alpha subtract,
    // 2-pass CGS reorth (rocBLAS sgemv pairs), norm, normalize.
    TORCH_CHECK(v.is_cuda() && v.is_contiguous() &&
                v.scalar_type() == torch::kFloat32);
    TORCH_CHECK(t_mat.is_contiguous() && t_mat.size(0) == ncv &&
                t_mat.size(1) == ncv);
    TORCH_CHECK(indptr.scalar_type() == torch::kInt32 &&
                indices.scalar_type() == torch::kInt32 &&
                values.scalar_type() == torch::kFloat32);
    TORCH_CHECK(u.numel() == v.size(1) && v_next.numel() == v.size(1) &&
                w.numel() >= ncv);
    const long long n = v.size(1);
    const long long nnz = indices.numel();
    float* vp = v.data_ptr<float>();
    float* tp = t_mat.data_ptr<float>();
    float* up = u.data_ptr<float>();
    float* wp = w.data_ptr<float>();
    double* ap = alpha_scal.data_ptr<double>();
    double* np2 = norm_scal.data_ptr<double>();
    hipStream_t s = cur_stream();
    for (long long i = start; i < ncv; i++) {
      raft_amd::launch_csr_spmv<float>(
          indptr.data_ptr<int>(), indices.data_ptr<int>(),
          values.data_ptr<float>(), vp + i * n, up, n, nnz, s);
      if (i == start && start > 0) {
        // arrowhead couplings: u -= V[:start]^T t_mat[start, :start]
        raft_amd::sgemv_rowmajor(vp, tp + start * ncv, up, start, n,
                                 /*trans=*/true, -1.f, 1.f, s);
        raft_amd::launch_lanczos_pre(up, vp + i * n, nullptr, nullptr, ap, n, s);
      } else if (i > start) {
        raft_amd::launch_lanczos_pre(up, vp + i * n, vp + (i - 1) * n,
                                     tp + i * ncv + (i - 1), ap, n, s);
      } else {
        raft_amd::launch_lanczos_pre(up, vp + i * n, nullptr, nullptr, ap, n, s);
      }
      raft_amd::launch_lanczos_sub_alpha(up, vp + i * n, ap, tp + i * ncv + i,
                                         n, s);
      for (int pass = 0; pass < 2; pass++) {
        raft_amd::sgemv_rowmajor(vp, up, wp, i + 1, n, false, 1.f, 0.f, s);
        raft_amd::sgemv_rowmajor(vp, wp, up, i + 1, n, true, -1.f, 1.f, s);
      }
      raft_amd::launch_lanczos_norm2(up, np2, n, s);
      if (i + 1 < ncv) {
        raft_amd::launch_lanczos_normalize(up, vp + (i + 1) * n, np2,
                                           tp + i * ncv + (i + 1),
                                           tp + (i + 1) * ncv + i, nullptr, n,
                                           s);
      } else {
        raft_amd::launch_lanczos_normalize(up, v_next.data_ptr<float>(), np2,
                                           nullptr, nullptr,
                                           beta_out.data_ptr<float>(), n, s);
      }
    }
  }, "full Lanczos extension cycle (SpMV + CGS reorth + fused steps) in C++");
  m.def("cholesky_r1_update_", [](torch::Tensor l, torch::Tensor x) {
    TORCH_CHECK(l.is_cuda() && l.dim() == 2 && l.size(0) == l.size(1) &&
                l.is_contiguous() && x.is_contiguous() &&
                x.numel() == l.size(0));
    const int n = (int)l.size(0);
    if (l.scalar_type() == torch::kFloat32) {
      raft_amd::launch_cholesky_r1_update_f32(l.data_ptr<float>(),
                                              x.data_ptr<float>(), n, n,
                                              cur_stream());
    } else if (l.scalar_type() == torch::kFloat64) {
      raft_amd::launch_cholesky_r1_update_f64(l.data_ptr<double>(),
                                              x.data_ptr<double>(), n, n,
                                              cur_stream());
    } else {
      TORCH_CHECK(false, "cholesky_r1_update_: fp32/fp64 only");
    }
  }, "in-place rank-1 Cholesky update (single-kernel hyperbolic rotations)");
  m.def("reduce_cols", &reduce_cols, "columnwise reduction (op code)");
  m.def("row_argmin", &row_argmin, "rowwise argmin");
  m.def("rows_sqnorm_bf16", &rows_sqnorm_bf16, "bf16 row squared norms -> f32");
  m.def("row_normalize_l2", &row_normalize_l2, "fused L2 row normalize");
  m.def("l2_epilogue_", &l2_epilogue_, "in-place L2 distance epilogue");
  m.def("l2nn_epilogue", &l2nn_epilogue, "fused argmin epilogue over GEMM tile");
  m.def("pairwise_unexpanded", &pairwise_unexpanded, "tiled unexpanded distances");
  m.def("pairwise_expanded_epilogue_", &pairwise_expanded_epilogue_,
        "in-place Hellinger/Russel-Rao/Jaccard/Dice epilogue over a GEMM result");
  m.def("rng_uniform", &rng_uniform, "counter-based uniform [0,1)",
        pybind11::arg("n"), pybind11::arg("seed"), pybind11::arg("subseq"),
        pybind11::arg("device"), pybind11::arg("gen") = 0);
  m.def("rng_normal", &rng_normal, "counter-based Box-Muller standard normal",
        pybind11::arg("n"), pybind11::arg("seed"), pybind11::arg("subseq"),
        pybind11::arg("device"), pybind11::arg("gen") = 0);
  m.def("make_blobs", &make_blobs, "fused gaussian blob generator");
  m.def("csr_spmv", &csr_spmv, "CSR SpMV (sub-wave per row)",
        pybind11::arg("indptr"), pybind11::arg("indices"), pybind11::arg("values"),
        pybind11::arg("x"), pybind11::arg("n_rows"), pybind11::arg("n_cols") = -1);
  m.def("csr_row_stats", &csr_row_stats,
        "per-row statistics of a CSR matrix for a sparse pairwise metric");
  m.def("csr_pairwise", &csr_pairwise,
        "CSR x CSR pairwise distances (LDS-staged intersection contraction)");
  m.def("reduce_rows_by_key", &reduce_rows_by_key, "keyed row accumulation");
  m.def("reduce_rows_by_key_sorted", &reduce_rows_by_key_sorted,
        "keyed row accumulation over a key-sorted permutation");
  m.def("reduce_rows_by_key_sorted_into", &reduce_rows_by_key_sorted_into,
        pybind11::arg("x"), pybind11::arg("perm"), pybind11::arg("keys_sorted"),
        pybind11::arg("sums"), pybind11::arg("counts"),
        pybind11::arg("dmin") = pybind11::none(),
        pybind11::arg("inertia_acc") = pybind11::none(),
        "keyed row accumulation + counts into caller buffers");
  m.def("split_bf16_norms", &split_bf16_norms,
        pybind11::arg("c"), pybind11::arg("slices"), pybind11::arg("cn"),
        pybind11::arg("cn_max") = pybind11::none(),
        "fused fp32->bf16 slice split + row sq-norms");
  m.def("kmeans_update_verify", &kmeans_update_verify,
        pybind11::arg("x"), pybind11::arg("perm"), pybind11::arg("keys_sorted"),
        pybind11::arg("c"), pybind11::arg("xn"), pybind11::arg("dmin"),
        pybind11::arg("amin"), pybind11::arg("dmin2"), pybind11::arg("cn_max"),
        pybind11::arg("sums"), pybind11::arg("counts"),
        pybind11::arg("inertia_acc") = pybind11::none(),
        pybind11::arg("lead") = 0x1p-13, pybind11::arg("tail") = 0x1p-18,
        "fused centroid-sum accumulation + exact-fp32 verify/refine (one X pass)");
  m.def("kmeans_update_centroids", &kmeans_update_centroids,
        "centroids = counts>0 ? sums/counts : centroids");
  m.def("select_k", &select_k, "batched top-k (radix)");
  m.def("device_sample_test", [](torch::Tensor weights, int64_t n_draws,
                                 int64_t seed) {
    TORCH_CHECK(weights.is_cuda() && weights.numel() == 256 &&
                weights.scalar_type() == torch::kFloat32);
    auto out = torch::empty({n_draws}, weights.options().dtype(torch::kInt32));
    raft_amd::launch_device_sample_test(weights.contiguous().data_ptr<float>(),
                                        out.data_ptr<int>(), (int)n_draws,
                                        (uint64_t)seed, cur_stream());
    return out;
  }, "block_random_sample test driver (weighted in-kernel selection)");
  m.def("sddmm", [](torch::Tensor a, torch::Tensor b, torch::Tensor rows,
                    torch::Tensor cols) {
    TORCH_CHECK(a.is_cuda() && b.is_cuda() && rows.is_cuda() && cols.is_cuda() &&
                b.device() == a.device() && rows.device() == a.device() &&
                cols.device() == a.device(), "sddmm operands must be on one GPU");
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.is_contiguous() && b.is_contiguous() &&
                a.scalar_type() == torch::kFloat32 &&
                b.scalar_type() == torch::kFloat32 &&
                a.size(1) == b.size(1) &&
                rows.scalar_type() == torch::kInt32 &&
                cols.scalar_type() == torch::kInt32 &&
                rows.numel() == cols.numel());
    auto vals = torch::empty({rows.numel()}, a.options());
    raft_amd::launch_sddmm(a.data_ptr<float>(), b.data_ptr<float>(),
                           rows.contiguous().data_ptr<int>(),
                           cols.contiguous().data_ptr<int>(),
                           vals.data_ptr<float>(), rows.numel(), a.size(1),
                           cur_stream());
    return vals;
  }, "sampled dense-dense matmul: vals[e] = dot(a[rows[e]], b[cols[e]])");
  m.def("linewise", [](torch::Tensor x, torch::Tensor v1,
                       c10::optional<torch::Tensor> v2, bool along_rows,
                       int64_t op1, int64_t op2) {
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                x.scalar_type() == torch::kFloat32);
    const long long n = x.size(0), d = x.size(1);
    TORCH_CHECK(op1 >= 0 && op1 <= 3 && op2 >= 0 && op2 <= 3, "bad linewise op code");
    // the vectors become raw device pointers: a host or non-fp32 vector must
    // fail here, not in the kernel
    TORCH_CHECK(v1.is_cuda() && v1.device() == x.device() &&
                v1.scalar_type() == torch::kFloat32,
                "v1 must be float32 on x's device");
    TORCH_CHECK(v1.numel() == (along_rows ? d : n) && v1.is_contiguous());
    const float* v2p = nullptr;
    torch::Tensor v2t;
    if (v2.has_value()) {
      TORCH_CHECK(v2.value().is_cuda() && v2.value().device() == x.device() &&
                  v2.value().scalar_type() == torch::kFloat32,
                  "v2 must be float32 on x's device");
      v2t = v2.value().contiguous();
      TORCH_CHECK(v2t.numel() == v1.numel());
      v2p = v2t.data_ptr<float>();
    }
    auto out = torch::empty_like(x);
    raft_amd::launch_linewise(x.data_ptr<float>(), out.data_ptr<float>(),
                              v1.data_ptr<float>(), v2p, n, d, along_rows,
                              (int)op1, (int)op2, cur_stream());
    return out;
  }, "fused linewise broadcast: out = (x op1 v1) [op2 v2]",
        pybind11::arg("x"), pybind11::arg("v1"),
        pybind11::arg("v2") = pybind11::none(),
        pybind11::arg("along_rows") = true, pybind11::arg("op1") = 0,
        pybind11::arg("op2") = 0);
  m.def("histogram_f32", [](torch::Tensor x, int64_t n_bins, double lo, double hi) {
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                x.scalar_type() == torch::kFloat32);
    TORCH_CHECK(n_bins >= 1 && n_bins <= 2147483647LL, "n_bins must be in [1, 2^31)");
    auto out = torch::zeros({n_bins, x.size(1)},
                            x.options().dtype(torch::kInt64));
    raft_amd::launch_histogram(
        x.data_ptr<float>(), x.size(0), x.size(1), (int)n_bins, (float)lo,
        (float)hi,
        reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
        cur_stream());
    return out;
  }, "per-column histograms (LDS-multi/LDS/gmem strategies by n_bins)");
  m.def("bitset_set_", [](torch::Tensor words, torch::Tensor idx, bool value) {
    TORCH_CHECK(words.is_cuda() && words.scalar_type() == torch::kInt32 &&
                words.is_contiguous() && idx.scalar_type() == torch::kInt64);
    TORCH_CHECK(idx.is_cuda() && idx.device() == words.device(),
                "idx must be on the words' device");
    raft_amd::launch_bitset_set(
        reinterpret_cast<unsigned int*>(words.data_ptr<int>()),
        reinterpret_cast<const long long*>(idx.contiguous().data_ptr<int64_t>()),
        idx.numel(), value ? 1 : 0, cur_stream());
  }, "O(k) bitset scatter set/clear");
  m.def("bitset_test", [](torch::Tensor words, torch::Tensor idx) {
    TORCH_CHECK(words.is_cuda() && words.scalar_type() == torch::kInt32 &&
                words.is_contiguous());
    TORCH_CHECK(idx.is_cuda() && idx.device() == words.device() &&
                idx.scalar_type() == torch::kInt64,
                "idx must be int64 on the words' device");
    auto out = torch::empty({idx.numel()}, words.options().dtype(torch::kBool));
    raft_amd::launch_bitset_test(
        reinterpret_cast<const unsigned int*>(words.data_ptr<int>()),
        reinterpret_cast<const long long*>(idx.contiguous().data_ptr<int64_t>()),
        out.data_ptr<bool>(), idx.numel(), cur_stream());
    return out;
  }, "bitset membership test");
  m.def("bitset_count", [](torch::Tensor words) {
    TORCH_CHECK(words.is_cuda() && words.scalar_type() == torch::kInt32 &&
                words.is_contiguous());
    auto out = torch::zeros({1}, words.options().dtype(torch::kInt64));
    raft_amd::launch_bitset_count(
        reinterpret_cast<const unsigned int*>(words.data_ptr<int>()),
        words.numel(),
        reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
        cur_stream());
    return out;
  }, "bitset popcount");
  m.def("select_k_generic", &select_k_generic,
        "generic top-k: any dtype, unbounded k, int64 idx, CSR row offsets",
        pybind11::arg("x"), pybind11::arg("row_off") = pybind11::none(),
        pybind11::arg("k"), pybind11::arg("select_min") = true);
  m.def("pairwise_l2_filter", &pairwise_l2_filter,
        "threshold-filtered pairwise L2 candidate emission (fused kNN); variant "
        "names one kernel (csrc/pairwise_variant.h) and raises if it cannot run "
        "the shape",
        pybind11::arg("x_slices"), pybind11::arg("y_slices"), pybind11::arg("xn"),
        pybind11::arg("yn"), pybind11::arg("thr"), pybind11::arg("out_d"),
        pybind11::arg("out_i"), pybind11::arg("cnt"), pybind11::arg("col_offset"),
        pybind11::arg("variant") = "auto");
  m.def("eps_neighbors_l2sq", &eps_neighbors_l2sq,
        "verified eps-neighborhood (squared L2) packed adjacency bitmap",
        pybind11::arg("x_slices"), pybind11::arg("y_slices"), pybind11::arg("xn"),
        pybind11::arg("yn"), pybind11::arg("xf"), pybind11::arg("yf"),
        pybind11::arg("bitmap"), pybind11::arg("rechecked"), pybind11::arg("n_cols"),
        pybind11::arg("eps_sq"), pybind11::arg("lead") = 0x1p-13,
        pybind11::arg("tail") = 0x1p-18);
  m.def("masked_l2nn", &masked_l2nn,
        "masked fused L2-NN (group mask, tile skip) -> (dmin, amin, dmin2)",
        pybind11::arg("x_slices"), pybind11::arg("y_slices"), pybind11::arg("xn"),
        pybind11::arg("yn"), pybind11::arg("y_group"), pybind11::arg("n_groups"),
        pybind11::arg("adj"), pybind11::arg("x_group"), pybind11::arg("scratch"),
        pybind11::arg("counters"));
  m.def("masked_l2nn_verify_repair", &masked_l2nn_verify_repair,
        "exact fp32 verify / repair of a masked L2-NN result (in place)",
        pybind11::arg("x"), pybind11::arg("y"), pybind11::arg("xn"),
        pybind11::arg("y_group"), pybind11::arg("n_groups"), pybind11::arg("adj"),
        pybind11::arg("x_group"), pybind11::arg("y_rank"), pybind11::arg("dmin"), pybind11::arg("amin"),
        pybind11::arg("dmin2"), pybind11::arg("yn_max"), pybind11::arg("rescanned"),
        pybind11::arg("lead") = 0x1p-13, pybind11::arg("tail") = 0x1p-18);
  m.def("ivf_flat_scan", &ivf_flat_scan,
        "IVF-Flat list-major scan of the probed lists into a ragged candidate buffer",
        pybind11::arg("data"), pybind11::arg("list_offsets"), pybind11::arg("indices"),
        pybind11::arg("queries"), pybind11::arg("item_list"),
        pybind11::arg("item_pair_begin"), pybind11::arg("item_pair_count"),
        pybind11::arg("n_items"), pybind11::arg("pair_query"),
        pybind11::arg("pair_out_off"), pybind11::arg("filter_words"),
        pybind11::arg("filter_bits"), pybind11::arg("out"), pybind11::arg("metric"),
        pybind11::arg("qg"), pybind11::arg("y_split"));
  m.def("ivf_flat_scan_max_qg", [](int64_t d_pad) {
    return (int64_t)raft_amd::ivf_flat_scan_max_qg((int)d_pad);
  }, "largest query-group size whose staged queries fit the scan kernel's LDS");
  m.def("bitmap_row_degrees", &bitmap_row_degrees,
        "per-row popcount of a row-padded bitmap into an int64 vector");
  m.def("bitmap_rows_to_csr", &bitmap_rows_to_csr,
        "row-padded bitmap -> sorted int32 CSR column ids at indptr[row]");
  m.def("bitmap_rows_expand", &bitmap_rows_expand,
        "row-padded bitmap -> dense bool [m, n]");
  m.def("pairwise_l2_mfma", &pairwise_l2_mfma,
        "fused split-bf16 MFMA pairwise L2 tile (single-write epilogue); variant "
        "names one kernel (csrc/pairwise_variant.h) and raises if it cannot run "
        "the shape",
        pybind11::arg("x_slices"), pybind11::arg("y_slices"), pybind11::arg("xn"),
        pybind11::arg("yn"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("sqrt_out") = false, pybind11::arg("variant") = "auto");
  m.def("l2nn_verify_repair", &l2nn_verify_repair,
        pybind11::arg("x"), pybind11::arg("c"), pybind11::arg("xn"),
        pybind11::arg("dmin"), pybind11::arg("amin"), pybind11::arg("dmin2"),
        pybind11::arg("cn_max"),
        pybind11::arg("lead") = 0x1p-13, pybind11::arg("tail") = 0x1p-18,
        "exact-fp32 verification/repair of split-bf16 L2-NN results");
  m.def("fused_l2nn_split", &fused_l2nn_split,
        "fused split-bf16 MFMA L2-NN (distance + argmin, no materialization); "
        "engine names one kernel (csrc/l2nn_engine.h) and raises if it cannot "
        "run the shape, gt = col-tiles per block of the 2d engines",
        pybind11::arg("x_slices"), pybind11::arg("c_slices"), pybind11::arg("xn"),
        pybind11::arg("cn"), pybind11::arg("engine") = "auto",
        pybind11::arg("gt") = 0);
  m.def("l2nn_resolve_engine", &l2nn_resolve_engine,
        "(engine, gt) that fused_l2nn_split runs for a shape and request",
        pybind11::arg("nslice"), pybind11::arg("m"), pybind11::arg("n"),
        pybind11::arg("d"), pybind11::arg("engine") = "auto", pybind11::arg("gt") = 0);
  m.def("gemm_bf16_f32", &gemm_bf16_f32, "bf16 x bf16 -> f32 rocBLAS gemm_ex",
        pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("beta") = 0.0);
  m.def("gemm_bf16_f32_nt", &gemm_bf16_f32_nt,
        "bf16 A @ B^T -> f32 (both row-major) rocBLAS gemm_ex",
        pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("beta") = 0.0);
  m.def("gemm_f32", &gemm_f32, "fp32 rocBLAS sgemm");
}
