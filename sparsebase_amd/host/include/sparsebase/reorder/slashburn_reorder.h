// SlashburnReorder (reference: reorder/slashburn_reorder.h, slashburn_reorder.cc:20-419) over sbx_slashburn_reorder.
// The rules, and where the device deliberately differs from the reference (flags held per call instead of in process
// globals, k < 1 and out-of-range columns refused, signed greedy degrees), are in include/sbx.h.
#ifndef SPARSEBASE_REORDER_SLASHBURN_REORDER_H_
#define SPARSEBASE_REORDER_SLASHBURN_REORDER_H_
#include "sparsebase/reorder/reorderer.h"

namespace sparsebase::reorder {

struct SlashburnReorderParams : utils::Parameters {
  int k_size;
  bool greedy;
  bool hub_order;
  explicit SlashburnReorderParams() {}
  SlashburnReorderParams(int hubset_k_size, bool greedy_alg, bool hub_ordering)
      : k_size(hubset_k_size), greedy(greedy_alg), hub_order(hub_ordering) {}
};

template <typename IDType, typename NNZType, typename ValueType>
class SlashburnReorder : public Reorderer<IDType> {
 public:
  typedef SlashburnReorderParams ParamsType;
  SlashburnReorder(int k_size, bool greedy, bool hub_order) {
    this->params_ = std::make_unique<SlashburnReorderParams>(k_size, greedy, hub_order);
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, GetReorderCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, GetReorderHIPCSR);
  }
  SlashburnReorder(ParamsType p) : SlashburnReorder(p.k_size, p.greedy, p.hub_order) {}
  // the order vector stays where sbx_slashburn_reorder writes it (see Reorderer::GetReorderDevice)
  format::HIPArray<IDType> *GetReorderDevice(format::Format *format, context::HIPContext *context,
                                             bool convert_input) override {
    typedef format::HIPCSR<IDType, NNZType, ValueType> D;
    if (!format->template IsAbsolute<D>() || format->template AsAbsolute<D>()->get_hip_context()->device_id != context->device_id)
      return Reorderer<IDType>::GetReorderDevice(format, context, convert_input);
    auto v = detail::DeviceCsrView<IDType, NNZType, ValueType>::Borrow(format->template AsAbsolute<D>());
    IDType *d_inv = (IDType *)v.dev->Malloc((size_t)(v.n ? v.n : 1) * sizeof(IDType));
    const int rc = Call(v, static_cast<SlashburnReorderParams *>(this->params_.get()), d_inv);
    if (rc != SBX_OK) {
      v.dev->Free(d_inv);
      v.dev->Check(rc);
    }
    return new format::HIPArray<IDType>((format::DimensionType)v.n, d_inv, *context, format::kOwned);
  }

 protected:
  static int Call(const detail::DeviceCsrView<IDType, NNZType, ValueType> &v, const SlashburnReorderParams *p,
                  IDType *d_inv) {
    const unsigned flags = (p->greedy ? SBX_SB_GREEDY : 0u) | (p->hub_order ? SBX_SB_HUB_ORDER : 0u);
    return sbx_slashburn_reorder(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), v.n, v.nnz, v.row_ptr, v.col,
                                 (int64_t)p->k_size, flags, d_inv, nullptr);
  }
  static IDType *Run(detail::DeviceCsrView<IDType, NNZType, ValueType> v, utils::Parameters *params) {
    hip::Staged<IDType> d_inv(*v.dev, (size_t)v.n);
    const int rc = Call(v, static_cast<SlashburnReorderParams *>(params), d_inv.get());
    IDType *inv = nullptr;
    if (rc == SBX_OK) inv = v.dev->Download(d_inv.get(), (size_t)v.n);
    v.Release();
    v.dev->Check(rc);
    return inv;
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
