// sparsebase/kernels/spmm.h — Y = A X of a CSR and a dense row-major block of k columns on the device (include/sbmm.h;
// additive, as kernels/spmv.h is: the reference has no product of its own).
//
//   kernels::SpMM(format, X, k, vals = null)   Y[i * k + j] = sum of vals[p] * X[col[p] * k + j] over the entries p of row i
//
// `format` is a format::HIPCSR<I, N, V> with format::HIPArray<F> operands on the same device (X: m * k values, row-major;
// nothing leaves HBM, the call is enqueued and not waited for, an owned HIPArray<F> of n * k values comes back), or a host
// format::CSR<I, N, V> with format::Array<F> operands (staged through the default device, a host Array<F> comes back).
// The value rules are those of kernels::SpMV: without `vals` the matrix's own values where V is F, otherwise a pattern,
// every stored value 1.  F is float, double or a 32- or 64-bit integer (integers wrap).  The sum is deterministic; its
// order is that of include/sbmm.h: the same for every column, not left to right, and not kernels::SpMV's.
#ifndef SPARSEBASE_KERNELS_SPMM_H_
#define SPARSEBASE_KERNELS_SPMM_H_
#include <memory>
#include <string>

#include "sbmm.h"
#include "sparsebase/kernels/spmv.h"

namespace sparsebase::kernels {

namespace detail {
// one sbmm_csr_spmm call, enqueued: d_y gets the view's n * k values (both leading dimensions are k)
template <typename I, typename N, typename V, typename F>
void MultiplyBlock(const reorder::detail::DeviceCsrView<I, N, V> &v, const DeviceVector<F> &x, size_t k,
                   const DeviceVector<F> *vals, F *d_y) {
  static_assert(hip::ValueTag<F>() != SBX_V_NONE && (sizeof(F) == 4 || sizeof(F) == 8), "SpMM: F is a 4- or 8-byte number");
  if (x.count < (size_t)v.m * k)
    throw utils::TypeException("SpMM: X holds " + std::to_string(x.count) + " values, the matrix has " +
                               std::to_string((long long)v.m) + " columns and k is " + std::to_string(k));
  if (vals && vals->count < (size_t)v.nnz)
    throw utils::TypeException("SpMM: the values array holds " + std::to_string(vals->count) + " values, the matrix has " +
                               std::to_string((long long)v.nnz) + " entries");
  const void *val = nullptr;
  if (vals) val = vals->ptr;
  else if constexpr (std::is_same_v<V, F>) val = v.vals;
  v.dev->Check(sbmm_csr_spmm(v.dev->handle(), hip::IndexTag<I, N>(), hip::ValueTag<F>(), (int64_t)v.n, (int64_t)v.m, v.nnz,
                             (int64_t)k, v.row_ptr, v.col, val, x.ptr, (int64_t)k, d_y, (int64_t)k));
}
}  // namespace detail

template <typename I, typename N, typename V, typename F>
format::HIPArray<F> *SpMM(format::HIPCSR<I, N, V> *format, format::HIPArray<F> *x, size_t k,
                          format::HIPArray<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Borrow(format);
  auto dx = detail::DeviceVector<F>::Borrow(x, *v.dev, "X");
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Borrow(vals, *v.dev, "the values array");
  const size_t count = (size_t)v.n * k;
  F *d_y = (F *)v.dev->Malloc((count ? count : 1) * sizeof(F));
  try {
    detail::MultiplyBlock(v, dx, k, vals ? &dvals : nullptr, d_y);
    return new format::HIPArray<F>((format::DimensionType)count, d_y, context::HIPContext(v.dev->id()), format::kOwned);
  } catch (...) {
    v.dev->Free(d_y);
    throw;
  }
}

template <typename I, typename N, typename V, typename F>
format::Array<F> *SpMM(format::CSR<I, N, V> *format, format::Array<F> *x, size_t k, format::Array<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, vals == nullptr && std::is_same_v<V, F>);
  utils::detail::CsrViewGuard<I, N, V> guard{v};
  auto dx = detail::DeviceVector<F>::Stage(x, *v.dev);
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Stage(vals, *v.dev);
  const size_t count = (size_t)v.n * k;
  hip::Staged<F> d_y(*v.dev, count ? count : 1);
  detail::MultiplyBlock(v, dx, k, vals ? &dvals : nullptr, d_y.get());
  return new format::Array<F>((format::DimensionType)count, v.dev->Download(d_y.get(), count ? count : 1), format::kOwned);
}

}  // namespace sparsebase::kernels
#endif
