// sparsebase/kernels/row_softmax.h — the softmax over the stored values of every row of a CSR on the device and its
// backward (include/sbsm.h; additive, as kernels/spmv.h, kernels/spmm.h and kernels/sddmm.h are: the reference has no
// such operation).
//
//   kernels::RowSoftmax(format, vals = null)     out[p] = exp(vals[p] - max of the row) / sum over the row of the exps
//   kernels::RowSoftmaxBackward(format, s, g)    dz[p] = s[p] * (g[p] - sum over the row of s[q] * g[q])
//
// `format` is a format::HIPCSR<I, N, V> with format::HIPArray<F> operands on the same device (nothing leaves HBM, the
// call is enqueued and not waited for, an owned HIPArray<F> of nnz values comes back), or a host format::CSR<I, N, V> with
// format::Array<F> operands (staged through the default device, a host Array<F> comes back).  The value rules are those
// of kernels::SDDMM: without `vals` the matrix's own values where V is F, otherwise a pattern, every stored value equal
// and out[p] = 1 / (entries of the row); then F is named explicitly: kernels::RowSoftmax<I, N, V, float>(format).  F is
// float (double is not built yet: include/sbsm.h).  -inf masks an entry; the special values and the order of the sums are those of include/sbsm.h.
#ifndef SPARSEBASE_KERNELS_ROW_SOFTMAX_H_
#define SPARSEBASE_KERNELS_ROW_SOFTMAX_H_
#include <memory>
#include <string>
#include <type_traits>

#include "sbsm.h"
#include "sparsebase/kernels/spmv.h"

namespace sparsebase::kernels {

namespace detail {
template <typename F>
void RequireEntries(const DeviceVector<F> &a, int64_t nnz, const char *who, const char *what) {
  if (a.count < (size_t)nnz)
    throw utils::TypeException(std::string(who) + ": " + what + " holds " + std::to_string(a.count) +
                               " values, the matrix has " + std::to_string((long long)nnz) + " entries");
}

// one sbsm_csr_row_softmax call, enqueued: d_out gets the view's nnz values
template <typename I, typename N, typename V, typename F>
void NormalizeRows(const reorder::detail::DeviceCsrView<I, N, V> &v, const DeviceVector<F> *vals, F *d_out) {
  static_assert(std::is_same_v<F, float>, "RowSoftmax: F is float");
  if (vals) RequireEntries(*vals, v.nnz, "RowSoftmax", "the values array");
  const void *val = nullptr;
  if (vals) val = vals->ptr;
  else if constexpr (std::is_same_v<V, F>) val = v.vals;
  v.dev->Check(sbsm_csr_row_softmax(v.dev->handle(), hip::IndexTag<I, N>(), hip::ValueTag<F>(), (int64_t)v.n, v.nnz,
                                    v.row_ptr, val, d_out));
}

// one sbsm_csr_row_softmax_backward call, enqueued: d_dz gets the view's nnz values
template <typename I, typename N, typename V, typename F>
void NormalizeRowsBackward(const reorder::detail::DeviceCsrView<I, N, V> &v, const DeviceVector<F> &s,
                           const DeviceVector<F> &g, F *d_dz) {
  static_assert(std::is_same_v<F, float>, "RowSoftmaxBackward: F is float");
  RequireEntries(s, v.nnz, "RowSoftmaxBackward", "s");
  RequireEntries(g, v.nnz, "RowSoftmaxBackward", "g");
  v.dev->Check(sbsm_csr_row_softmax_backward(v.dev->handle(), hip::IndexTag<I, N>(), hip::ValueTag<F>(), (int64_t)v.n, v.nnz,
                                             v.row_ptr, s.ptr, g.ptr, d_dz));
}

// an owned HIPArray of the view's nnz values that `fill` has enqueued the writing of
template <typename F, typename View, typename Fill>
format::HIPArray<F> *OwnedEntries(const View &v, Fill fill) {
  const size_t count = (size_t)v.nnz;
  F *d_out = (F *)v.dev->Malloc((count ? count : 1) * sizeof(F));
  try {
    fill(d_out);
    return new format::HIPArray<F>((format::DimensionType)count, d_out, context::HIPContext(v.dev->id()), format::kOwned);
  } catch (...) {
    v.dev->Free(d_out);
    throw;
  }
}
}  // namespace detail

template <typename I, typename N, typename V, typename F = V>
format::HIPArray<F> *RowSoftmax(format::HIPCSR<I, N, V> *format, format::HIPArray<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Borrow(format);
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Borrow(vals, *v.dev, "the values array");
  return detail::OwnedEntries<F>(v, [&](F *d_out) { detail::NormalizeRows(v, vals ? &dvals : nullptr, d_out); });
}

template <typename I, typename N, typename V, typename F = V>
format::Array<F> *RowSoftmax(format::CSR<I, N, V> *format, format::Array<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, vals == nullptr && std::is_same_v<V, F>);
  utils::detail::CsrViewGuard<I, N, V> guard{v};
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Stage(vals, *v.dev);
  const size_t count = (size_t)v.nnz;
  hip::Staged<F> d_out(*v.dev, count ? count : 1);
  detail::NormalizeRows(v, vals ? &dvals : nullptr, d_out.get());
  return new format::Array<F>((format::DimensionType)count, v.dev->Download(d_out.get(), count ? count : 1), format::kOwned);
}

template <typename I, typename N, typename V, typename F>
format::HIPArray<F> *RowSoftmaxBackward(format::HIPCSR<I, N, V> *format, format::HIPArray<F> *s, format::HIPArray<F> *g) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Borrow(format);
  auto ds = detail::DeviceVector<F>::Borrow(s, *v.dev, "s");
  auto dg = detail::DeviceVector<F>::Borrow(g, *v.dev, "g");
  return detail::OwnedEntries<F>(v, [&](F *d_dz) { detail::NormalizeRowsBackward(v, ds, dg, d_dz); });
}

template <typename I, typename N, typename V, typename F>
format::Array<F> *RowSoftmaxBackward(format::CSR<I, N, V> *format, format::Array<F> *s, format::Array<F> *g) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, false);
  utils::detail::CsrViewGuard<I, N, V> guard{v};
  auto ds = detail::DeviceVector<F>::Stage(s, *v.dev);
  auto dg = detail::DeviceVector<F>::Stage(g, *v.dev);
  const size_t count = (size_t)v.nnz;
  hip::Staged<F> d_dz(*v.dev, count ? count : 1);
  detail::NormalizeRowsBackward(v, ds, dg, d_dz.get());
  return new format::Array<F>((format::DimensionType)count, v.dev->Download(d_dz.get(), count ? count : 1), format::kOwned);
}

}  // namespace sparsebase::kernels
#endif
