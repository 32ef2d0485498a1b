// sparsebase/feature/degrees_degree_distribution.h — feature::Degrees_DegreeDistribution (reference:
// feature/degrees_degree_distribution.h, degrees_degree_distribution.cc:15-164): Degrees and DegreeDistribution of a
// CSR's rows from one pass over row_ptr, sbfx_csr_degrees_degree_distribution (include/sbfx.h), as a map keyed by the
// two sub-features' ids.  This is the class feature::Extractor picks when both are asked for.  Registered for {CSR}
// (row_ptr alone is staged through the default device; the columns are never read) and {HIPCSR} (in place).
//
// The reference's Degrees_DegreeDistribution(Params) builds a temporary and leaves the object itself without
// functions and params (.cc:17-20); here it delegates to the default constructor.
#ifndef SPARSEBASE_FEATURE_DEGREES_DEGREE_DISTRIBUTION_H_
#define SPARSEBASE_FEATURE_DEGREES_DEGREE_DISTRIBUTION_H_
#include <algorithm>

#include "sbfx.h"
#include "sparsebase/feature/degree_distribution.h"
#include "sparsebase/feature/degree_stats.h"
#include "sparsebase/feature/degrees.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class Degrees_DegreeDistribution : public FeaturePreprocessType<std::unordered_map<std::type_index, std::any>> {
  typedef Degrees<IDType, NNZType, ValueType> Deg;
  typedef DegreeDistribution<IDType, NNZType, ValueType, FeatureType> Dist;
  typedef detail::DevicePtrView<NNZType> View;

 public:
  typedef Params ParamsType;
  Degrees_DegreeDistribution() {
    Register();
    this->params_ = std::shared_ptr<Params>(new Params());
    this->pmap_.insert({get_id_static(), this->params_});
    this->pmap_[Dist::get_id_static()] = std::shared_ptr<utils::Parameters>(new DegreeDistributionParams);
    this->pmap_[Deg::get_id_static()] = std::shared_ptr<utils::Parameters>(new DegreesParams);
  }
  Degrees_DegreeDistribution(Params) : Degrees_DegreeDistribution() {}
  Degrees_DegreeDistribution(const Degrees_DegreeDistribution &d) {
    Register();
    this->params_ = d.params_;
    this->pmap_ = d.pmap_;
  }
  Degrees_DegreeDistribution(std::shared_ptr<Params> p) {
    Register();
    this->params_ = p;
    this->pmap_[get_id_static()] = p;
  }
  ~Degrees_DegreeDistribution() override = default;

  std::unordered_map<std::type_index, std::any> Extract(format::Format *format, std::vector<context::Context *> c,
                                                        bool convert_input) override {
    return Get(format, c, convert_input);
  }
  std::vector<std::type_index> get_sub_ids() override {
    std::vector<std::type_index> r = {typeid(Deg), typeid(Dist)};
    std::sort(r.begin(), r.end());
    return r;
  }
  // the two sub-features, in the order of get_sub_ids, each with the params this object holds for it
  std::vector<utils::Extractable *> get_subs() override {
    auto *f1 = new Deg();
    auto *f2 = new Dist();
    if (this->pmap_.count(Deg::get_id_static())) f1->set_params(Deg::get_id_static(), this->pmap_[Deg::get_id_static()]);
    if (this->pmap_.count(Dist::get_id_static())) f2->set_params(Dist::get_id_static(), this->pmap_[Dist::get_id_static()]);
    if (this->get_sub_ids()[0] == f1->get_id()) return {f1, f2};
    return {f2, f1};
  }
  static std::type_index get_id_static() {
    return typeid(Degrees_DegreeDistribution<IDType, NNZType, ValueType, FeatureType>);
  }

  // {Degrees: IDType *, DegreeDistribution: FeatureType *}, n values each; the caller frees both with delete[]
  std::unordered_map<std::type_index, std::any> Get(format::Format *format, std::vector<context::Context *> c,
                                                    bool convert_input) {
    return this->Execute(this->params_.get(), c, convert_input, format);
  }
  // the reference's name for the {CSR} implementation (degrees_degree_distribution.h)
  static std::unordered_map<std::type_index, std::any> GetCSR(std::vector<format::Format *> formats,
                                                              utils::Parameters *) {
    auto *csr = formats[0]->AsAbsolute<format::CSR<IDType, NNZType, ValueType>>();
    return Run(View::Stage(csr->get_row_ptr(), (int64_t)csr->get_dimensions()[0]), (int64_t)csr->get_num_nnz());
  }

 protected:
  void Register() {
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, GetCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, OnDeviceCSR);
  }
  static std::unordered_map<std::type_index, std::any> OnDeviceCSR(std::vector<format::Format *> formats,
                                                                   utils::Parameters *) {
    auto *d = formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
    return Run(View::Borrow(d->device(), d->get_row_ptr(), (int64_t)d->get_dimensions()[0]), (int64_t)d->get_num_nnz());
  }
  static std::unordered_map<std::type_index, std::any> Run(View v, int64_t nnz) {
    static_assert(std::is_same_v<FeatureType, float> || std::is_same_v<FeatureType, double>,
                  "FeatureType must be float or double");
    hip::Staged<IDType> d_deg(*v.dev, (size_t)v.n);
    hip::Staged<FeatureType> d_dist(*v.dev, (size_t)v.n);
    const int rc = sbfx_csr_degrees_degree_distribution(v.dev->handle(), hip::IndexTag<IDType, NNZType>(), v.n, nnz, v.ptr,
                                                        (int)sizeof(FeatureType), d_deg.get(), d_dist.get());
    IDType *deg = nullptr;
    FeatureType *dist = nullptr;
    if (rc == SBX_OK) {
      deg = v.dev->Download(d_deg.get(), (size_t)v.n);
      dist = v.dev->Download(d_dist.get(), (size_t)v.n);
    }
    v.Release();
    v.dev->Check(rc);
    return {{Deg::get_id_static(), std::any(deg)}, {Dist::get_id_static(), std::any(dist)}};
  }
};

}  // namespace sparsebase::feature
#endif
