// sparsebase/feature/avg_degree.h — feature::AvgDegree (reference: feature/avg_degree.h, avg_degree.cc:127-137): the
// average degree of a CSR's rows, (F)sum / (F)n.
// The façade and the {CSR} (staged) and {HIPCSR} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_AVG_DEGREE_H_
#define SPARSEBASE_FEATURE_AVG_DEGREE_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

struct AvgDegreeParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class AvgDegree
    : public detail::DegreeStatistic<AvgDegree<IDType, NNZType, ValueType, FeatureType>, detail::OverRows, FeatureType,
                                     AvgDegreeParams, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<AvgDegree<IDType, NNZType, ValueType, FeatureType>, detail::OverRows, FeatureType,
                                  AvgDegreeParams, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  AvgDegree() = default;
  AvgDegree(const AvgDegree &) = default;
  static constexpr unsigned kFlags = 0;
  static FeatureType *Compute(const sbxstat_degrees &s) { return new FeatureType(detail::StatAvg<FeatureType>(s)); }

  FeatureType *GetAvgDegree(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, FeatureType *> GetAvgDegreeCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSR} implementation
  static FeatureType *GetAvgDegreeCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
