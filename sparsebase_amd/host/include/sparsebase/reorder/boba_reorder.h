// BOBAReorder (reference: reorder/boba_reorder.h, boba_reorder.cc:33-138) over sbx_boba_reorder.  The order is one
// closed form for both values of `sequential` (include/sbx.h), and covers the max(n, m) vertices of the COO: every
// path, GetReorderDevice included, returns max(n, m) entries.  Registered for COO (staged through the default device)
// and HIPCOO (borrowed); a CSR reaches it through the converter, as in the reference.
#ifndef SPARSEBASE_REORDER_BOBA_REORDER_H_
#define SPARSEBASE_REORDER_BOBA_REORDER_H_
#include "sparsebase/reorder/reorderer.h"

namespace sparsebase::reorder {

struct BOBAReorderParams : utils::Parameters {
  bool sequential;
  explicit BOBAReorderParams() {}
  BOBAReorderParams(bool sequential_) : sequential(sequential_) {}
};

template <typename IDType, typename NNZType, typename ValueType>
class BOBAReorder : public Reorderer<IDType> {
 public:
  typedef BOBAReorderParams ParamsType;
  explicit BOBAReorder(bool sequential = true) {
    this->params_ = std::make_unique<BOBAReorderParams>(sequential);
    this->RegisterFunction({format::COO<IDType, NNZType, ValueType>::get_id_static()}, GetReorderCOO);
    this->RegisterFunction({format::HIPCOO<IDType, NNZType, ValueType>::get_id_static()}, GetReorderHIPCOO);
  }
  BOBAReorder(ParamsType p) : BOBAReorder(p.sequential) {}
  // the order vector stays where sbx_boba_reorder writes it; other inputs run GetReorder and upload max(n, m) entries
  format::HIPArray<IDType> *GetReorderDevice(format::Format *format, context::HIPContext *context,
                                             bool convert_input) override {
    typedef format::HIPCOO<IDType, NNZType, ValueType> D;
    const size_t nodes = Nodes(format);
    if (!format->template IsAbsolute<D>() || format->template AsAbsolute<D>()->get_hip_context()->device_id != context->device_id) {
      IDType *host = this->GetReorder(format, {context}, convert_input);
      auto &dev = hip::Device::Get(context->device_id);
      IDType *d = nullptr;
      try {
        d = dev.Upload(host, nodes ? nodes : 1);
      } catch (...) {
        delete[] host;
        throw;
      }
      delete[] host;
      return new format::HIPArray<IDType>((format::DimensionType)nodes, d, *context, format::kOwned);
    }
    auto v = detail::DeviceCooView<IDType, NNZType, ValueType>::Borrow(format->template AsAbsolute<D>());
    IDType *d_inv = (IDType *)v.dev->Malloc((nodes ? nodes : 1) * sizeof(IDType));
    const int rc = Call(v, d_inv);
    if (rc != SBX_OK) {
      v.dev->Free(d_inv);
      v.dev->Check(rc);
    }
    return new format::HIPArray<IDType>((format::DimensionType)nodes, d_inv, *context, format::kOwned);
  }

 protected:
  static size_t Nodes(format::Format *f) {
    const auto d = f->get_dimensions();
    return (size_t)(d[0] > d[1] ? d[0] : d[1]);
  }
  static int Call(const detail::DeviceCooView<IDType, NNZType, ValueType> &v, IDType *d_inv) {
    return sbx_boba_reorder(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), (int64_t)v.n, (int64_t)v.m, v.nnz, v.row,
                            v.col, d_inv);
  }
  static IDType *Run(detail::DeviceCooView<IDType, NNZType, ValueType> v) {
    const size_t nodes = (size_t)(v.n > v.m ? v.n : v.m);
    hip::Staged<IDType> d_inv(*v.dev, nodes ? nodes : 1);
    const int rc = Call(v, d_inv.get());
    IDType *inv = nullptr;
    if (rc == SBX_OK) inv = nodes ? v.dev->Download(d_inv.get(), nodes) : new IDType[1];
    v.Release();
    v.dev->Check(rc);
    return inv;
  }
  static IDType *GetReorderCOO(std::vector<format::Format *> formats, utils::Parameters *) {
    auto *coo = formats[0]->AsAbsolute<format::COO<IDType, NNZType, ValueType>>();
    return Run(detail::DeviceCooView<IDType, NNZType, ValueType>::Stage(coo));
  }
  static IDType *GetReorderHIPCOO(std::vector<format::Format *> formats, utils::Parameters *) {
    auto *coo = formats[0]->AsAbsolute<format::HIPCOO<IDType, NNZType, ValueType>>();
    return Run(detail::DeviceCooView<IDType, NNZType, ValueType>::Borrow(coo));
  }
};

}  // namespace sparsebase::reorder
#endif
