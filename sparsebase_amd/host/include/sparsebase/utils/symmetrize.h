// sparsebase/utils/symmetrize.h — the pattern of A ∪ Aᵀ of a square CSR on the device (include/sbsym.h; additive: the
// reference has no such utility, its RCM reads an unsymmetric pattern's stale distances).
//
//   utils::MissingMirrors(format)            entries the format lacks to be structurally symmetric
//   utils::IsStructurallySymmetric(format)   MissingMirrors(format) == 0
//   utils::Symmetrize<I, N, V>(format, no_diagonal = false)
//                                            every stored entry (duplicates, values) plus one entry per missing mirror,
//                                            with the value of the first stored entry it mirrors; rows column-sorted
//
// `format` is a format::CSR (staged through the default device; a host CSR comes back) or a format::HIPCSR (stays in
// HBM; an owned HIPCSR on the same device comes back, its arrays from the pooled hip::Device::Malloc).  The caller owns
// the result.  Temporaries come from the pool and go back to it on every way out.  A rectangular format is refused
// with a utils::TypeException that names both dimensions.
#ifndef SPARSEBASE_UTILS_SYMMETRIZE_H_
#define SPARSEBASE_UTILS_SYMMETRIZE_H_
#include <memory>
#include <string>

#include "sbsym.h"
#include "sparsebase/reorder/reorderer.h"

namespace sparsebase::utils {

namespace detail {
// a DeviceCsrView whose staged arrays return to the pool when the scope ends, whichever way it ends
template <typename I, typename N, typename V>
struct CsrViewGuard {
  reorder::detail::DeviceCsrView<I, N, V> &v;
  ~CsrViewGuard() { v.Release(); }
};

template <typename I, typename N, typename V>
void RequireSquare(const reorder::detail::DeviceCsrView<I, N, V> &v, const char *who) {
  if (v.n != v.m)
    throw TypeException(std::string(who) + " needs a square matrix, got " + std::to_string((long long)v.n) + " x " +
                        std::to_string((long long)v.m));
}

// one sbsym_csr_symmetrize call into pooled blocks of 2 nnz entries (A ∪ Aᵀ never holds more)
template <typename I, typename N>
struct DeviceSymmetrized {
  std::unique_ptr<hip::Staged<N>> row_ptr;
  std::unique_ptr<hip::Staged<I>> col;
  std::unique_ptr<hip::Staged<char>> vals;  // capacity * sizeof(V) bytes; null in pattern mode
  int64_t nnz = 0, added = 0;
};
template <typename I, typename N, typename V>
DeviceSymmetrized<I, N> SymmetrizeOnDevice(const reorder::detail::DeviceCsrView<I, N, V> &v, unsigned flags, bool with_vals) {
  DeviceSymmetrized<I, N> out;
  const size_t cap = v.nnz ? 2 * (size_t)v.nnz : 1;
  constexpr size_t vb = hip::ValueBytes<V>();
  const bool vals = with_vals && vb && v.vals;
  out.row_ptr = std::make_unique<hip::Staged<N>>(*v.dev, (size_t)v.n + 1);
  out.col = std::make_unique<hip::Staged<I>>(*v.dev, cap);
  if (vals) out.vals = std::make_unique<hip::Staged<char>>(*v.dev, cap * vb);
  v.dev->Check(sbsym_csr_symmetrize(v.dev->handle(), hip::IndexTag<I, N>(), vals ? hip::ValueTag<V>() : SBX_V_NONE, v.n,
                                    v.nnz, v.row_ptr, v.col, vals ? (const void *)v.vals : nullptr, flags, (int64_t)cap,
                                    out.row_ptr->get(), out.col->get(), vals ? out.vals->get() : nullptr, &out.nnz,
                                    &out.added));
  return out;
}

template <typename I, typename N, typename V>
int64_t MissingMirrorsOnDevice(reorder::detail::DeviceCsrView<I, N, V> v) {
  CsrViewGuard<I, N, V> guard{v};
  RequireSquare(v, "MissingMirrors");
  int64_t missing = 0;
  v.dev->Check(sbsym_csr_missing_mirrors(v.dev->handle(), hip::IndexTag<I, N>(), v.n, v.nnz, v.row_ptr, v.col, &missing));
  return missing;
}
}  // namespace detail

template <typename I, typename N, typename V>
int64_t MissingMirrors(format::CSR<I, N, V> *format) {
  return detail::MissingMirrorsOnDevice(reorder::detail::DeviceCsrView<I, N, V>::Stage(format, false));
}
template <typename I, typename N, typename V>
int64_t MissingMirrors(format::HIPCSR<I, N, V> *format) {
  return detail::MissingMirrorsOnDevice(reorder::detail::DeviceCsrView<I, N, V>::Borrow(format));
}
template <typename F>
bool IsStructurallySymmetric(F *format) {
  return MissingMirrors(format) == 0;
}

template <typename I, typename N, typename V>
format::CSR<I, N, V> *Symmetrize(format::CSR<I, N, V> *format, bool no_diagonal = false) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Stage(format, true);
  detail::CsrViewGuard<I, N, V> guard{v};
  detail::RequireSquare(v, "Symmetrize");
  auto d = detail::SymmetrizeOnDevice(v, no_diagonal ? SBSYM_NO_DIAGONAL : 0u, true);
  std::unique_ptr<N[]> rp(v.dev->Download(d.row_ptr->get(), (size_t)v.n + 1));
  std::unique_ptr<I[]> col(v.dev->Download(d.col->get(), (size_t)(d.nnz ? d.nnz : 1)));
  V *vals = nullptr;
  if constexpr (!std::is_same_v<V, void>)
    if (d.vals) vals = v.dev->Download((const V *)d.vals->get(), (size_t)(d.nnz ? d.nnz : 1));
  return new format::CSR<I, N, V>(v.n, v.n, rp.release(), col.release(), vals, format::kOwned, true);
}

template <typename I, typename N, typename V>
format::HIPCSR<I, N, V> *Symmetrize(format::HIPCSR<I, N, V> *format, bool no_diagonal = false) {
  auto v = reorder::detail::DeviceCsrView<I, N, V>::Borrow(format);
  detail::RequireSquare(v, "Symmetrize");
  auto d = detail::SymmetrizeOnDevice(v, no_diagonal ? SBSYM_NO_DIAGONAL : 0u, true);
  // blocks of the result's own size: the 2 nnz of capacity go back to the pool
  const size_t k = (size_t)d.nnz;
  constexpr size_t vb = hip::ValueBytes<V>();
  N *rp = nullptr;
  I *col = nullptr;
  V *vals = nullptr;
  try {
    rp = (N *)v.dev->Malloc(((size_t)v.n + 1) * sizeof(N));
    col = (I *)v.dev->Malloc(k * sizeof(I));
    if (d.vals) vals = (V *)v.dev->Malloc(k * vb);
    v.dev->Copy(rp, d.row_ptr->get(), ((size_t)v.n + 1) * sizeof(N));
    if (k) v.dev->Copy(col, d.col->get(), k * sizeof(I));
    if (k && d.vals) v.dev->Copy((void *)vals, d.vals->get(), k * vb);
    return new format::HIPCSR<I, N, V>(v.n, v.n, (N)d.nnz, rp, col, vals,
                                       context::HIPContext(format->get_hip_context()->device_id), format::kOwned, true);
  } catch (...) {
    v.dev->Free(rp);
    v.dev->Free(col);
    v.dev->Free((void *)vals);
    throw;
  }
}

}  // namespace sparsebase::utils
#endif
