// sparsebase/feature/triangle_count.h — feature::TriangleCount (reference: feature/triangle_count.h:12-66,
// triangle_count.cc:11-223).  The interface is the reference's: TriangleCountParams{countDirected}, the count as a
// `new int64_t` the caller deletes.  Registered for {CSR}, staged through the default device like Degrees and
// Bandwidth, and {HIPCSR}, which runs in place; both return the reference's value (sbx_csr_triangle_count without
// SBX_TC_EXACT), which is not the number of triangles on every graph: see include/sbx.h.  The exact count is an
// ABI / Python capability (SBX_TC_EXACT) and not a parameter here: the params stay the reference's.
#ifndef SPARSEBASE_FEATURE_TRIANGLE_COUNT_H_
#define SPARSEBASE_FEATURE_TRIANGLE_COUNT_H_
#include <tuple>

#include "sparsebase/feature/feature_preprocess_type.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/reorder/reorderer.h"

namespace sparsebase::feature {

struct TriangleCountParams : utils::Parameters {
  bool countDirected = 0;
  TriangleCountParams() {}
  TriangleCountParams(bool countDirected) : countDirected(countDirected) {}
};

template <typename IDType, typename NNZType, typename ValueType>
class TriangleCount : public FeaturePreprocessType<int64_t *> {
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;

 public:
  typedef TriangleCountParams ParamsType;
  TriangleCount() {
    Register();
    this->params_ = std::shared_ptr<ParamsType>(new ParamsType());
    this->pmap_.insert({get_id_static(), this->params_});
  }
  TriangleCount(ParamsType p) {
    Register();
    this->params_ = std::shared_ptr<ParamsType>(new ParamsType(p.countDirected));
    this->pmap_.insert({get_id_static(), this->params_});
  }
  TriangleCount(const TriangleCount &d) {
    Register();
    this->params_ = d.params_;
    this->pmap_ = d.pmap_;
  }
  TriangleCount(std::shared_ptr<ParamsType> p) {
    Register();
    this->params_ = p;
    this->pmap_[get_id_static()] = p;
  }
  ~TriangleCount() override = default;

  std::unordered_map<std::type_index, std::any> Extract(format::Format *format, std::vector<context::Context *> c,
                                                        bool convert_input) override {
    return {{this->get_id(), std::forward<int64_t *>(GetTriangleCount(format, c, convert_input))}};
  }
  std::vector<std::type_index> get_sub_ids() override { return {typeid(TriangleCount<IDType, NNZType, ValueType>)}; }
  std::vector<utils::Extractable *> get_subs() override {
    return {new TriangleCount<IDType, NNZType, ValueType>(*this)};
  }
  static std::type_index get_id_static() { return typeid(TriangleCount<IDType, NNZType, ValueType>); }

  int64_t *GetTriangleCount(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Execute(this->params_.get(), c, convert_input, format);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, int64_t *> GetTriangleCountCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->CachedExecute(this->params_.get(), c, convert_input, false, format);
  }

  // the reference's value (triangle_count.cc:142-206); caller frees with delete
  static int64_t *Run(View v, utils::Parameters *p) {
    const bool directed = static_cast<TriangleCountParams *>(p)->countDirected;
    int64_t count = 0;
    const int rc = sbx_csr_triangle_count(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), v.n, v.nnz, v.row_ptr,
                                          v.col, directed ? SBX_TC_DIRECTED : 0u, &count);
    v.Release();
    v.dev->Check(rc);
    return new int64_t(count);
  }
  // the reference's name for the {CSR} implementation (triangle_count.h:61-62)
  static int64_t *GetTriangleCountCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return OnHostCSR(formats, p);
  }

 protected:
  void Register() {
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, OnHostCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, OnDeviceCSR);
  }
  static int64_t *OnHostCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Run(View::Stage(formats[0]->AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), false), p);
  }
  static int64_t *OnDeviceCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Run(View::Borrow(formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>()), p);
  }
};

}  // namespace sparsebase::feature
#endif
