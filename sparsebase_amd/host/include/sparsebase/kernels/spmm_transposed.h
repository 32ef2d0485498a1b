// sparsebase/kernels/spmm_transposed.h — Y = A^T X of a CSR and a dense row-major block of k columns on the device, from
// a plan that is built once per sparsity pattern (include/sbmt.h; additive, as kernels/spmm.h is).
//
//   kernels::TransposePlan<I, N> plan(format)           the pattern of A^T and the position of each of its entries in the
//                                                       CSR arrays: three device arrays, owned by the plan and given
//                                                       back to the host layer's pool when it goes
//   kernels::SpMMTransposed(plan, X, k, vals = null)    Y[c * k + j] = sum of vals[p] * X[i * k + j] over the stored
//                                                       entries p = (i, c) of column c
//
// `format` is a format::HIPCSR<I, N, V> (the plan lives on its device) or a host format::CSR<I, N, V> (staged through the
// default device, once).  The plan holds no values: `vals` are the matrix's values in CSR order, one array per call, so
// one plan serves every step of a training loop; without `vals` the matrix is a pattern, every stored value 1.  X holds
// n * k values and Y comes back with m * k: format::HIPArray<F> operands on the plan's device stay in HBM (the call is
// enqueued and not waited for, an owned HIPArray<F> comes back), host format::Array<F> operands are staged (a host
// Array<F> comes back).  F is float, double or a 32- or 64-bit integer (integers wrap).  The sum is deterministic; its
// bits are those of kernels::SpMM on the materialised transpose (include/sbmt.h).
#ifndef SPARSEBASE_KERNELS_SPMM_TRANSPOSED_H_
#define SPARSEBASE_KERNELS_SPMM_TRANSPOSED_H_
#include <memory>
#include <string>

#include "sbmt.h"
#include "sparsebase/kernels/spmv.h"

namespace sparsebase::kernels {

template <typename I, typename N>
class TransposePlan {
 public:
  template <typename V>
  explicit TransposePlan(format::HIPCSR<I, N, V> *format) {
    Build(reorder::detail::DeviceCsrView<I, N, V>::Borrow(format));
  }
  template <typename V>
  explicit TransposePlan(format::CSR<I, N, V> *format) {
    auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, false);
    utils::detail::CsrViewGuard<I, N, V> guard{v};
    Build(v);
  }
  ~TransposePlan() { Release(); }
  TransposePlan(const TransposePlan &) = delete;
  TransposePlan &operator=(const TransposePlan &) = delete;

  hip::Device &device() const { return *dev_; }
  int64_t rows() const { return n_; }     // of A: the rows of X
  int64_t columns() const { return m_; }  // of A: the rows of Y
  int64_t nnz() const { return nnz_; }
  const N *col_ptr() const { return col_ptr_; }  // device arrays: m + 1 offsets, nnz row ids, nnz positions
  const I *row() const { return row_; }
  const N *perm() const { return perm_; }

 private:
  template <typename V>
  void Build(const reorder::detail::DeviceCsrView<I, N, V> &v) {
    dev_ = v.dev;
    n_ = (int64_t)v.n;
    m_ = (int64_t)v.m;
    nnz_ = v.nnz;
    const size_t entries = nnz_ ? (size_t)nnz_ : 1;
    try {
      col_ptr_ = (N *)dev_->Malloc(((size_t)m_ + 1) * sizeof(N));
      row_ = (I *)dev_->Malloc(entries * sizeof(I));
      perm_ = (N *)dev_->Malloc(entries * sizeof(N));
      dev_->Check(sbmt_csr_transpose_plan(dev_->handle(), hip::IndexTag<I, N>(), n_, m_, nnz_, v.row_ptr, v.col, col_ptr_,
                                          row_, perm_));
    } catch (...) {
      Release();
      throw;
    }
  }
  void Release() {
    if (!dev_) return;
    dev_->Free(col_ptr_);
    dev_->Free(row_);
    dev_->Free(perm_);
    col_ptr_ = perm_ = nullptr;
    row_ = nullptr;
  }

  hip::Device *dev_ = nullptr;
  int64_t n_ = 0, m_ = 0, nnz_ = 0;
  N *col_ptr_ = nullptr, *perm_ = nullptr;
  I *row_ = nullptr;
};

namespace detail {
// one sbmt_csr_spmm_t call, enqueued: d_y gets the plan's m * k values (both leading dimensions are k)
template <typename I, typename N, typename F>
void MultiplyTransposed(const TransposePlan<I, N> &plan, const DeviceVector<F> &x, size_t k, const DeviceVector<F> *vals,
                        F *d_y) {
  static_assert(hip::ValueTag<F>() != SBX_V_NONE && (sizeof(F) == 4 || sizeof(F) == 8),
                "SpMMTransposed: F is a 4- or 8-byte number");
  if (x.count < (size_t)plan.rows() * k)
    throw utils::TypeException("SpMMTransposed: X holds " + std::to_string(x.count) + " values, the matrix has " +
                               std::to_string((long long)plan.rows()) + " rows and k is " + std::to_string(k));
  if (vals && vals->count < (size_t)plan.nnz())
    throw utils::TypeException("SpMMTransposed: the values array holds " + std::to_string(vals->count) +
                               " values, the matrix has " + std::to_string((long long)plan.nnz()) + " entries");
  plan.device().Check(sbmt_csr_spmm_t(plan.device().handle(), hip::IndexTag<I, N>(), hip::ValueTag<F>(), plan.rows(),
                                      plan.columns(), plan.nnz(), (int64_t)k, plan.col_ptr(), plan.row(), plan.perm(),
                                      vals ? vals->ptr : nullptr, x.ptr, (int64_t)k, d_y, (int64_t)k));
}
}  // namespace detail

template <typename I, typename N, typename F>
format::HIPArray<F> *SpMMTransposed(const TransposePlan<I, N> &plan, format::HIPArray<F> *x, size_t k,
                                    format::HIPArray<F> *vals = nullptr) {
  hip::Device &dev = plan.device();
  auto dx = detail::DeviceVector<F>::Borrow(x, dev, "X");
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Borrow(vals, dev, "the values array");
  const size_t count = (size_t)plan.columns() * k;
  F *d_y = (F *)dev.Malloc((count ? count : 1) * sizeof(F));
  try {
    detail::MultiplyTransposed(plan, dx, k, vals ? &dvals : nullptr, d_y);
    return new format::HIPArray<F>((format::DimensionType)count, d_y, context::HIPContext(dev.id()), format::kOwned);
  } catch (...) {
    dev.Free(d_y);
    throw;
  }
}

template <typename I, typename N, typename F>
format::Array<F> *SpMMTransposed(const TransposePlan<I, N> &plan, format::Array<F> *x, size_t k,
                                 format::Array<F> *vals = nullptr) {
  hip::Device &dev = plan.device();
  auto dx = detail::DeviceVector<F>::Stage(x, dev);
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Stage(vals, dev);
  const size_t count = (size_t)plan.columns() * k;
  hip::Staged<F> d_y(dev, count ? count : 1);
  detail::MultiplyTransposed(plan, dx, k, vals ? &dvals : nullptr, d_y.get());
  return new format::Array<F>((format::DimensionType)count, dev.Download(d_y.get(), count ? count : 1), format::kOwned);
}

}  // namespace sparsebase::kernels
#endif
