// RCMReorder (reference: reorder/rcm_reorder.h:14-45, rcm_reorder.cc:9-166).
// Parity holds for structurally symmetric, column-sorted patterns.
#ifndef SPARSEBASE_REORDER_RCM_REORDER_H_
#define SPARSEBASE_REORDER_RCM_REORDER_H_
#include "sparsebase/reorder/reorderer.h"
#include "sparsebase/utils/symmetrize.h"

namespace sparsebase::reorder {

// symmetrize (additive; the reference's struct is empty): where the pattern is not structurally symmetric, order the
// pattern of A + A^T (utils/symmetrize.h) instead of refusing it.  The default keeps the refusal.
struct RCMReorderParams : utils::Parameters {
  bool symmetrize = false;
  RCMReorderParams() = default;
  explicit RCMReorderParams(bool symmetrize) : symmetrize(symmetrize) {}
};

template <typename IDType, typename NNZType, typename ValueType>
class RCMReorder : public Reorderer<IDType> {
 public:
  typedef RCMReorderParams ParamsType;
  RCMReorder() {
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, GetReorderCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, GetReorderHIPCSR);
  }
  explicit RCMReorder(RCMReorderParams params) : RCMReorder() { this->params_ = std::make_unique<RCMReorderParams>(params); }
  // the order vector stays where sbx_rcm_reorder writes it (see Reorderer::GetReorderDevice)
  format::HIPArray<IDType> *GetReorderDevice(format::Format *format, context::HIPContext *context,
                                             bool convert_input) override {
    typedef format::HIPCSR<IDType, NNZType, ValueType> D;
    if (!format->template IsAbsolute<D>() || format->template AsAbsolute<D>()->get_hip_context()->device_id != context->device_id)
      return Reorderer<IDType>::GetReorderDevice(format, context, convert_input);
    auto v = detail::DeviceCsrView<IDType, NNZType, ValueType>::Borrow(format->template AsAbsolute<D>());
    IDType *d_inv = (IDType *)v.dev->Malloc((size_t)(v.n ? v.n : 1) * sizeof(IDType));
    try {
      Order(v, this->params_.get(), d_inv);
    } catch (...) {
      v.dev->Free(d_inv);
      throw;
    }
    return new format::HIPArray<IDType>((format::DimensionType)v.n, d_inv, *context, format::kOwned);
  }

 protected:
  // sbx_rcm_reorder on the view's pattern, or with params->symmetrize on the pattern of A + A^T where A lacks mirrors
  // (one sbsym_csr_symmetrize call in pattern mode that leaves a symmetric A alone); throws what the library refuses
  static void Order(const detail::DeviceCsrView<IDType, NNZType, ValueType> &v, utils::Parameters *params, IDType *d_inv) {
    const NNZType *row_ptr = v.row_ptr;
    const IDType *col = v.col;
    int64_t nnz = v.nnz;
    utils::detail::DeviceSymmetrized<IDType, NNZType> sym;  // (its blocks return to the pool on every way out)
    if (params && static_cast<RCMReorderParams *>(params)->symmetrize) {
      utils::detail::RequireSquare(v, "RCMReorder with symmetrize");
      sym = utils::detail::SymmetrizeOnDevice(v, SBSYM_SKIP_IF_SYMMETRIC, false);
      if (sym.added) {
        row_ptr = sym.row_ptr->get();
        col = sym.col->get();
        nnz = sym.nnz;
      }
    }
    v.dev->Check(sbx_rcm_reorder(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), v.n, nnz, row_ptr, col, d_inv, nullptr));
  }
  static IDType *Run(detail::DeviceCsrView<IDType, NNZType, ValueType> v, utils::Parameters *params) {
    utils::detail::CsrViewGuard<IDType, NNZType, ValueType> guard{v};  // (staged arrays: back to the pool, failures included)
    hip::Staged<IDType> d_inv(*v.dev, (size_t)v.n);
    Order(v, params, d_inv.get());
    return v.dev->Download(d_inv.get(), (size_t)v.n);
  }
  static IDType *GetReorderCSR(std::vector<format::Format *> formats, utils::Parameters *params) {
    auto *csr = formats[0]->AsAbsolute<format::CSR<IDType, NNZType, ValueType>>();
    return Run(detail::DeviceCsrView<IDType, NNZType, ValueType>::Stage(csr, false), params);
  }
  static IDType *GetReorderHIPCSR(std::vector<format::Format *> formats, utils::Parameters *params) {
    auto *csr = formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
    return Run(detail::DeviceCsrView<IDType, NNZType, ValueType>::Borrow(csr), params);
  }
};

}  // namespace sparsebase::reorder
#endif
