// sparsebase/kernels/sddmm.h — the sampled dense-dense product on the pattern of a CSR on the device (include/sbdd.h;
// additive, as kernels/spmv.h and kernels/spmm.h are: the reference has no product of its own).
//
//   kernels::SDDMM(format, U, V, k, vals = null)   out[p] = vals[p] * sum over j < k of U[row(p) * k + j] * V[col[p] * k + j]
//
// `format` is a format::HIPCSR<I, N, V> with format::HIPArray<F> operands on the same device (U: n * k values, V: m * k
// values, both row-major; nothing leaves HBM, the call is enqueued and not waited for, an owned HIPArray<F> of nnz values
// comes back), or a host format::CSR<I, N, V> with format::Array<F> operands (staged through the default device, a host
// Array<F> comes back).  The value rules are those of kernels::SpMM: without `vals` the matrix's own values where V is F,
// otherwise a pattern, every stored value 1.  F is float, double or a 32- or 64-bit integer (integers wrap).  The result
// is deterministic and does not depend on where an entry lies; the order of the sum over j is that of include/sbdd.h, not
// left to right.
#ifndef SPARSEBASE_KERNELS_SDDMM_H_
#define SPARSEBASE_KERNELS_SDDMM_H_
#include <memory>
#include <string>

#include "sbdd.h"
#include "sparsebase/kernels/spmv.h"

namespace sparsebase::kernels {

namespace detail {
// one sbdd_csr_sddmm call, enqueued: d_out gets the view's nnz values (both leading dimensions are k)
template <typename I, typename N, typename V, typename F>
void SampleBlock(const reorder::detail::DeviceCsrView<I, N, V> &v, const DeviceVector<F> &u, const DeviceVector<F> &x,
                 size_t k, const DeviceVector<F> *vals, F *d_out) {
  static_assert(hip::ValueTag<F>() != SBX_V_NONE && (sizeof(F) == 4 || sizeof(F) == 8), "SDDMM: F is a 4- or 8-byte number");
  if (u.count < (size_t)v.n * k)
    throw utils::TypeException("SDDMM: U holds " + std::to_string(u.count) + " values, the matrix has " +
                               std::to_string((long long)v.n) + " rows and k is " + std::to_string(k));
  if (x.count < (size_t)v.m * k)
    throw utils::TypeException("SDDMM: V holds " + std::to_string(x.count) + " values, the matrix has " +
                               std::to_string((long long)v.m) + " columns and k is " + std::to_string(k));
  if (vals && vals->count < (size_t)v.nnz)
    throw utils::TypeException("SDDMM: the values array holds " + std::to_string(vals->count) + " values, the matrix has " +
                               std::to_string((long long)v.nnz) + " entries");
  const void *val = nullptr;
  if (vals) val = vals->ptr;
  else if constexpr (std::is_same_v<V, F>) val = v.vals;
  v.dev->Check(sbdd_csr_sddmm(v.dev->handle(), hip::IndexTag<I, N>(), hip::ValueTag<F>(), (int64_t)v.n, (int64_t)v.m, v.nnz,
                              (int64_t)k, v.row_ptr, v.col, val, u.ptr, (int64_t)k, x.ptr, (int64_t)k, d_out));
}
}  // namespace detail

template <typename I, typename N, typename V, typename F>
format::HIPArray<F> *SDDMM(format::HIPCSR<I, N, V> *format, format::HIPArray<F> *u, format::HIPArray<F> *x, size_t k,
                           format::HIPArray<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Borrow(format);
  auto du = detail::DeviceVector<F>::Borrow(u, *v.dev, "U");
  auto dx = detail::DeviceVector<F>::Borrow(x, *v.dev, "V");
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Borrow(vals, *v.dev, "the values array");
  const size_t count = (size_t)v.nnz;
  F *d_out = (F *)v.dev->Malloc((count ? count : 1) * sizeof(F));
  try {
    detail::SampleBlock(v, du, dx, k, vals ? &dvals : nullptr, d_out);
    return new format::HIPArray<F>((format::DimensionType)count, d_out, context::HIPContext(v.dev->id()), format::kOwned);
  } catch (...) {
    v.dev->Free(d_out);
    throw;
  }
}

template <typename I, typename N, typename V, typename F>
format::Array<F> *SDDMM(format::CSR<I, N, V> *format, format::Array<F> *u, format::Array<F> *x, size_t k,
                        format::Array<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, vals == nullptr && std::is_same_v<V, F>);
  utils::detail::CsrViewGuard<I, N, V> guard{v};
  auto du = detail::DeviceVector<F>::Stage(u, *v.dev);
  auto dx = detail::DeviceVector<F>::Stage(x, *v.dev);
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Stage(vals, *v.dev);
  const size_t count = (size_t)v.nnz;
  hip::Staged<F> d_out(*v.dev, count ? count : 1);
  detail::SampleBlock(v, du, dx, k, vals ? &dvals : nullptr, d_out.get());
  return new format::Array<F>((format::DimensionType)count, v.dev->Download(d_out.get(), count ? count : 1), format::kOwned);
}

}  // namespace sparsebase::kernels
#endif
