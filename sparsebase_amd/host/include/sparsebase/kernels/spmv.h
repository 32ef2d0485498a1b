// sparsebase/kernels/spmv.h — y = A x of a CSR on the device (include/sbmv.h; additive: the reference has no SpMV of its
// own, only the kernels its experiment example carries along, examples/example_experiment/example_experiment.cu:32-184).
//
//   kernels::CheckCSR(format)              throws utils::HIPDeviceException (the library's message names what failed and
//                                          where) unless the format's row_ptr and col are a well-formed CSR
//   kernels::SpMV(format, x, vals = null)  y[i] = sum of vals[p] * x[col[p]] over the stored entries p of row i
//
// `format` is a format::HIPCSR<I, N, V> with format::HIPArray<F> vectors on the same device (nothing leaves HBM, the call
// is enqueued and not waited for, an owned HIPArray<F> comes back), or a host format::CSR<I, N, V> with format::Array<F>
// vectors (staged through the default device, a host Array<F> comes back).  Without `vals` the matrix's own values are
// used when V is F; otherwise the matrix is a pattern, every stored value 1 — which is how a <unsigned, unsigned,
// unsigned> matrix multiplies a float vector, as in the reference's example.  F is float, double or a 32- or 64-bit
// integer (integers wrap).  The sum is deterministic; its order is that of include/sbmv.h, not left to right.
#ifndef SPARSEBASE_KERNELS_SPMV_H_
#define SPARSEBASE_KERNELS_SPMV_H_
#include <memory>
#include <string>

#include "sbmv.h"
#include "sparsebase/format/array.h"
#include "sparsebase/reorder/reorderer.h"
#include "sparsebase/utils/symmetrize.h"

namespace sparsebase::kernels {

namespace detail {
// a vector on a device: borrowed from an HIPArray, or staged from a host Array (back to the pool when this goes)
template <typename F>
struct DeviceVector {
  const F *ptr = nullptr;
  size_t count = 0;
  std::unique_ptr<hip::Staged<F>> staged;

  static DeviceVector Borrow(format::HIPArray<F> *a, const hip::Device &dev, const char *what) {
    if (a->get_hip_context()->device_id != dev.id())
      throw utils::TypeException(std::string("SpMV: ") + what + " lives on device " +
                                 std::to_string(a->get_hip_context()->device_id) + ", the matrix on device " +
                                 std::to_string(dev.id()));
    DeviceVector v;
    v.ptr = a->get_vals();
    v.count = (size_t)a->get_num_nnz();
    return v;
  }
  static DeviceVector Stage(format::Array<F> *a, const hip::Device &dev) {
    DeviceVector v;
    v.count = (size_t)a->get_num_nnz();
    v.staged = std::make_unique<hip::Staged<F>>(dev, a->get_vals(), v.count ? v.count : 1);
    v.ptr = v.staged->get();
    return v;
  }
};

// one sbmv_csr_spmv call, enqueued: d_y gets the view's n values
template <typename I, typename N, typename V, typename F>
void Multiply(const reorder::detail::DeviceCsrView<I, N, V> &v, const DeviceVector<F> &x, const DeviceVector<F> *vals,
              F *d_y) {
  static_assert(hip::ValueTag<F>() != SBX_V_NONE && (sizeof(F) == 4 || sizeof(F) == 8), "SpMV: F is a 4- or 8-byte number");
  if (x.count < (size_t)v.m)
    throw utils::TypeException("SpMV: x holds " + std::to_string(x.count) + " values, the matrix has " +
                               std::to_string((long long)v.m) + " columns");
  if (vals && vals->count < (size_t)v.nnz)
    throw utils::TypeException("SpMV: the values array holds " + std::to_string(vals->count) + " values, the matrix has " +
                               std::to_string((long long)v.nnz) + " entries");
  const void *val = nullptr;
  if (vals) val = vals->ptr;
  else if constexpr (std::is_same_v<V, F>) val = v.vals;
  v.dev->Check(sbmv_csr_spmv(v.dev->handle(), hip::IndexTag<I, N>(), hip::ValueTag<F>(), (int64_t)v.n, (int64_t)v.m, v.nnz,
                             v.row_ptr, v.col, val, x.ptr, d_y));
}

template <typename I, typename N, typename V>
void Check(reorder::detail::DeviceCsrView<I, N, V> v) {
  utils::detail::CsrViewGuard<I, N, V> guard{v};
  v.dev->Check(sbmv_csr_check(v.dev->handle(), hip::IndexTag<I, N>(), (int64_t)v.n, (int64_t)v.m, v.nnz, v.row_ptr, v.col));
}
}  // namespace detail

template <typename I, typename N, typename V>
void CheckCSR(format::CSR<I, N, V> *format) {
  detail::Check(reorder::detail::DeviceCsrView<I, N, V>::Stage(format, false));
}
template <typename I, typename N, typename V>
void CheckCSR(format::HIPCSR<I, N, V> *format) {
  detail::Check(reorder::detail::DeviceCsrView<I, N, V>::Borrow(format));
}

template <typename I, typename N, typename V, typename F>
format::HIPArray<F> *SpMV(format::HIPCSR<I, N, V> *format, format::HIPArray<F> *x, format::HIPArray<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Borrow(format);
  auto dx = detail::DeviceVector<F>::Borrow(x, *v.dev, "x");
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Borrow(vals, *v.dev, "the values array");
  F *d_y = (F *)v.dev->Malloc((size_t)(v.n ? v.n : 1) * sizeof(F));
  try {
    detail::Multiply(v, dx, vals ? &dvals : nullptr, d_y);
    return new format::HIPArray<F>((format::DimensionType)v.n, d_y, context::HIPContext(v.dev->id()), format::kOwned);
  } catch (...) {
    v.dev->Free(d_y);
    throw;
  }
}

template <typename I, typename N, typename V, typename F>
format::Array<F> *SpMV(format::CSR<I, N, V> *format, format::Array<F> *x, format::Array<F> *vals = nullptr) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, vals == nullptr && std::is_same_v<V, F>);
  utils::detail::CsrViewGuard<I, N, V> guard{v};
  auto dx = detail::DeviceVector<F>::Stage(x, *v.dev);
  detail::DeviceVector<F> dvals;
  if (vals) dvals = detail::DeviceVector<F>::Stage(vals, *v.dev);
  hip::Staged<F> d_y(*v.dev, (size_t)(v.n ? v.n : 1));
  detail::Multiply(v, dx, vals ? &dvals : nullptr, d_y.get());
  return new format::Array<F>((format::DimensionType)v.n, v.dev->Download(d_y.get(), (size_t)(v.n ? v.n : 1)),
                              format::kOwned);
}

}  // namespace sparsebase::kernels
#endif
