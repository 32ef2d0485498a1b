// sparsebase/feature/off_diag_block_nnz.h — feature::OffDiagBlockNNZ (reference: feature/off_diag_block_nnz.h:12-68,
// off_diag_block_nnz.cc:13-116): the number of nonzeros outside the diagonal blocks when the rows are cut into
// blockrowsize contiguous blocks and the columns into blockcolsize (sbxstat_csr_off_diag_block_nnz, include/sbx_stats.h,
// has the rule).  Registered for {CSR}, staged through the default device, and {HIPCSR}, which runs in place.  The
// device counts in 64 bits; the value is narrowed to IDType, as the reference's `IDType cnt` is.
#ifndef SPARSEBASE_FEATURE_OFF_DIAG_BLOCK_NNZ_H_
#define SPARSEBASE_FEATURE_OFF_DIAG_BLOCK_NNZ_H_
#include <tuple>

#include "sbx_stats.h"
#include "sparsebase/feature/feature_preprocess_type.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/reorder/reorderer.h"

namespace sparsebase::feature {

struct OffDiagBlockNNZParams : utils::Parameters {
  int blockrowsize = 1, blockcolsize = 1;
  OffDiagBlockNNZParams() {}
  OffDiagBlockNNZParams(int N) : blockrowsize(N), blockcolsize(N) {}
  OffDiagBlockNNZParams(int blockrowsize, int blockcolsize) : blockrowsize(blockrowsize), blockcolsize(blockcolsize) {}
};

template <typename IDType, typename NNZType, typename ValueType>
class OffDiagBlockNNZ : public FeaturePreprocessType<IDType *> {
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;

 public:
  typedef OffDiagBlockNNZParams ParamsType;
  OffDiagBlockNNZ() {
    Register();
    this->params_ = std::shared_ptr<ParamsType>(new ParamsType());
    this->pmap_.insert({get_id_static(), this->params_});
  }
  OffDiagBlockNNZ(ParamsType p) {
    Register();
    this->params_ = std::shared_ptr<ParamsType>(new ParamsType(p.blockrowsize, p.blockcolsize));
    this->pmap_.insert({get_id_static(), this->params_});
  }
  OffDiagBlockNNZ(const OffDiagBlockNNZ &d) {
    Register();
    this->params_ = d.params_;
    this->pmap_ = d.pmap_;
  }
  OffDiagBlockNNZ(std::shared_ptr<ParamsType> p) {
    Register();
    this->params_ = p;
    this->pmap_[get_id_static()] = p;
  }
  ~OffDiagBlockNNZ() override = default;

  std::unordered_map<std::type_index, std::any> Extract(format::Format *format, std::vector<context::Context *> c,
                                                        bool convert_input) override {
    return {{this->get_id(), std::forward<IDType *>(GetOffDiagBlockNNZ(format, c, convert_input))}};
  }
  std::vector<std::type_index> get_sub_ids() override { return {typeid(OffDiagBlockNNZ<IDType, NNZType, ValueType>)}; }
  std::vector<utils::Extractable *> get_subs() override {
    return {new OffDiagBlockNNZ<IDType, NNZType, ValueType>(*this)};
  }
  static std::type_index get_id_static() { return typeid(OffDiagBlockNNZ<IDType, NNZType, ValueType>); }

  IDType *GetOffDiagBlockNNZ(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Execute(this->params_.get(), c, convert_input, format);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, IDType *> GetOffDiagBlockNNZCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->CachedExecute(this->params_.get(), c, convert_input, false, format);
  }

  // off_diag_block_nnz.cc:94-116; caller frees with delete
  static IDType *Run(View v, utils::Parameters *p) {
    const auto *param = static_cast<OffDiagBlockNNZParams *>(p);
    int64_t count = 0;
    const int rc = sbxstat_csr_off_diag_block_nnz(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), v.n, v.m, v.nnz,
                                                  v.row_ptr, v.col, param->blockrowsize, param->blockcolsize, &count);
    v.Release();
    v.dev->Check(rc);
    return new IDType((IDType)count);
  }
  // the reference's name for the {CSR} implementation (off_diag_block_nnz.h:62)
  static IDType *GetOffDiagBlockNNZCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return OnHostCSR(formats, p);
  }

 protected:
  void Register() {
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, OnHostCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, OnDeviceCSR);
  }
  static IDType *OnHostCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Run(View::Stage(formats[0]->AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), false), p);
  }
  static IDType *OnDeviceCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Run(View::Borrow(formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>()), p);
  }
};

}  // namespace sparsebase::feature
#endif
