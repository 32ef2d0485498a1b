// sparsebase/feature/min_max_avg_degree.h — feature::MinMaxAvgDegree (reference: feature/min_max_avg_degree.h,
// min_max_avg_degree.cc:15-191): MinDegree, MaxDegree and AvgDegree of a CSR's rows from one call of
// sbxstat_degree_stats, as a map keyed by the three sub-features' ids.  Registered for {CSR} (staged through the
// default device) and {HIPCSR} (in place).
#ifndef SPARSEBASE_FEATURE_MIN_MAX_AVG_DEGREE_H_
#define SPARSEBASE_FEATURE_MIN_MAX_AVG_DEGREE_H_
#include <algorithm>

#include "sparsebase/feature/avg_degree.h"
#include "sparsebase/feature/max_degree.h"
#include "sparsebase/feature/min_degree.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class MinMaxAvgDegree : public FeaturePreprocessType<std::unordered_map<std::type_index, std::any>> {
  typedef MinDegree<IDType, NNZType, ValueType> Min;
  typedef MaxDegree<IDType, NNZType, ValueType> Max;
  typedef AvgDegree<IDType, NNZType, ValueType, FeatureType> Avg;

 public:
  typedef Params ParamsType;
  MinMaxAvgDegree() {
    Register();
    this->params_ = std::shared_ptr<Params>(new Params());
    this->pmap_.insert({get_id_static(), this->params_});
    this->pmap_[Min::get_id_static()] = std::shared_ptr<utils::Parameters>(new utils::Parameters);
    this->pmap_[Max::get_id_static()] = std::shared_ptr<utils::Parameters>(new utils::Parameters);
    this->pmap_[Avg::get_id_static()] = std::shared_ptr<utils::Parameters>(new AvgDegreeParams);
  }
  MinMaxAvgDegree(Params) : MinMaxAvgDegree() {}
  MinMaxAvgDegree(const MinMaxAvgDegree &d) {
    Register();
    this->params_ = d.params_;
    this->pmap_ = d.pmap_;
  }
  MinMaxAvgDegree(std::shared_ptr<Params> p) {
    Register();
    this->params_ = p;
    this->pmap_[get_id_static()] = p;
  }
  ~MinMaxAvgDegree() override = default;

  std::unordered_map<std::type_index, std::any> Extract(format::Format *format, std::vector<context::Context *> c,
                                                        bool convert_input) override {
    return Get(format, c, convert_input);
  }
  std::vector<std::type_index> get_sub_ids() override {
    std::vector<std::type_index> r = {typeid(Min), typeid(Max), typeid(Avg)};
    std::sort(r.begin(), r.end());
    return r;
  }
  // the three sub-features, in the order of get_sub_ids (min_max_avg_degree.cc:94-136)
  std::vector<utils::Extractable *> get_subs() override {
    auto *f1 = new Min();
    auto *f2 = new Max();
    auto *f3 = new Avg();
    if (this->pmap_.count(Min::get_id_static())) f1->set_params(Min::get_id_static(), this->pmap_[Min::get_id_static()]);
    if (this->pmap_.count(Max::get_id_static())) f2->set_params(Max::get_id_static(), this->pmap_[Max::get_id_static()]);
    if (this->pmap_.count(Avg::get_id_static())) f3->set_params(Avg::get_id_static(), this->pmap_[Avg::get_id_static()]);
    std::vector<utils::Extractable *> res(3);
    auto ids = this->get_sub_ids();
    for (int i = 0; i < 3; ++i)
      res[i] = ids[i] == f1->get_id() ? (utils::Extractable *)f1 : ids[i] == f2->get_id() ? (utils::Extractable *)f2 : f3;
    return res;
  }
  static std::type_index get_id_static() { return typeid(MinMaxAvgDegree<IDType, NNZType, ValueType, FeatureType>); }

  // {MinDegree: NNZType *, MaxDegree: NNZType *, AvgDegree: FeatureType *}; the caller deletes the three values
  std::unordered_map<std::type_index, std::any> Get(format::Format *format, std::vector<context::Context *> c,
                                                    bool convert_input) {
    return this->Execute(this->params_.get(), c, convert_input, format);
  }
  // the reference's name for the {CSR} implementation (min_max_avg_degree.h:64)
  static std::unordered_map<std::type_index, std::any> GetCSR(std::vector<format::Format *> formats,
                                                              utils::Parameters *) {
    return Values(detail::OverRows::Stats<IDType, NNZType, ValueType>(formats[0], false, 0));
  }

 protected:
  void Register() {
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static()}, GetCSR);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, OnDeviceCSR);
  }
  static std::unordered_map<std::type_index, std::any> OnDeviceCSR(std::vector<format::Format *> formats,
                                                                   utils::Parameters *) {
    return Values(detail::OverRows::Stats<IDType, NNZType, ValueType>(formats[0], true, 0));
  }
  static std::unordered_map<std::type_index, std::any> Values(const sbxstat_degrees &s) {
    return {{Min::get_id_static(), std::any(new NNZType((NNZType)s.min))},
            {Max::get_id_static(), std::any(new NNZType((NNZType)s.max))},
            {Avg::get_id_static(), std::any(new FeatureType(detail::StatAvg<FeatureType>(s)))}};
  }
};

}  // namespace sparsebase::feature
#endif
