// sparsebase/feature/bandwidth_profile.h — feature::Bandwidth_Profile, a fused class of this project's own (the
// reference has none for this pair): Bandwidth and Profile of a CSR from one pass over its columns,
// sbfx_csr_bandwidth_profile (include/sbfx.h), as a map keyed by the two sub-features' ids.  Each value has the type
// its own class returns: Bandwidth an int *, Profile an IDType *.  This is the class feature::Extractor picks when both
// are asked for.  Registered for {CSR} (staged through the default device, once) and {HIPCSR} (in place).
#ifndef SPARSEBASE_FEATURE_BANDWIDTH_PROFILE_H_
#define SPARSEBASE_FEATURE_BANDWIDTH_PROFILE_H_
#include <algorithm>

#include "sbfx.h"
#include "sparsebase/feature/bandwidth.h"
#include "sparsebase/feature/profile.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType>
class Bandwidth_Profile : public FeaturePreprocessType<std::unordered_map<std::type_index, std::any>> {
  typedef Bandwidth<IDType, NNZType, ValueType> Bw;
  typedef Profile<IDType, NNZType, ValueType> Pr;
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;

 public:
  typedef Params ParamsType;
  Bandwidth_Profile() {
    Register();
    this->params_ = std::shared_ptr<Params>(new Params());
    this->pmap_.insert({get_id_static(), this->params_});
    this->pmap_[Bw::get_id_static()] = std::shared_ptr<utils::Parameters>(new utils::Parameters);
    this->pmap_[Pr::get_id_static()] = std::shared_ptr<utils::Parameters>(new utils::Parameters);
  }
  Bandwidth_Profile(Params) : Bandwidth_Profile() {}
  Bandwidth_Profile(const Bandwidth_Profile &d) {
    Register();
    this->params_ = d.params_;
    this->pmap_ = d.pmap_;
  }
  Bandwidth_Profile(std::shared_ptr<Params> p) {
    Register();
    this->params_ = p;
    this->pmap_[get_id_static()] = p;
  }
  ~Bandwidth_Profile() override = default;

  std::unordered_map<std::type_index, std::any> Extract(format::Format *format, std::vector<context::Context *> c,
                                                        bool convert_input) override {
    return Get(format, c, convert_input);
  }
  std::vector<std::type_index> get_sub_ids() override {
    std::vector<std::type_index> r = {typeid(Bw), typeid(Pr)};
    std::sort(r.begin(), r.end());
    return r;
  }
  // the two sub-features, in the order of get_sub_ids, each with the params this object holds for it
  std::vector<utils::Extractable *> get_subs() override {
    auto *f1 = new Bw();
    auto *f2 = new Pr();
    if (this->pmap_.count(Bw::get_id_static())) f1->set_params(Bw::get_id_static(), this->pmap_[Bw::get_id_static()]);
    if (this->pmap_.count(Pr::get_id_static())) f2->set_params(Pr::get_id_static(), this->pmap_[Pr::get_id_static()]);
    if (this->get_sub_ids()[0] == f1->get_id()) return {f1, f2};
    return {f2, f1};
  }
  static std::type_index get_id_static() { return typeid(Bandwidth_Profile<IDType, NNZType, ValueType>); }

  // {Bandwidth: int *, Profile: IDType *}; the caller frees both with delete
  std::unordered_map<std::type_index, std::any> Get(format::Format *format, std::vector<context::Context *> c,
                                                    bool convert_input) {
    return this->Execute(this->params_.get(), c, convert_input, format);
  }
  static std::unordered_map<std::type_index, std::any> GetCSR(std::vector<format::Format *> formats,
                                                              utils::Parameters *) {
    return Run(View::Stage(formats[0]->AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), false));
  }

 protected:
  void Register() {
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, GetCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, OnDeviceCSR);
  }
  static std::unordered_map<std::type_index, std::any> OnDeviceCSR(std::vector<format::Format *> formats,
                                                                   utils::Parameters *) {
    return Run(View::Borrow(formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>()));
  }
  // the narrowings are those of Bandwidth::Run and Profile::Run
  static std::unordered_map<std::type_index, std::any> Run(View v) {
    int64_t bw = 0, sum = 0;
    const int rc = sbfx_csr_bandwidth_profile(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), v.n, v.nnz, v.row_ptr,
                                              v.col, &bw, &sum);
    v.Release();
    v.dev->Check(rc);
    return {{Bw::get_id_static(), std::any(new int((int)bw))}, {Pr::get_id_static(), std::any(new IDType((IDType)sum))}};
  }
};

}  // namespace sparsebase::feature
#endif
