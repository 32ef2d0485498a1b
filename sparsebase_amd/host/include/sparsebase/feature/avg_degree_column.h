// sparsebase/feature/avg_degree_column.h — feature::AvgDegreeColumn (reference: feature/avg_degree_column.h,
// avg_degree_column.cc:127-137): the average degree of a CSC's columns, (F)sum / (F)n.
// The façade and the {CSC} (staged) and {HIPCSC} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_AVG_DEGREE_COLUMN_H_
#define SPARSEBASE_FEATURE_AVG_DEGREE_COLUMN_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

struct AvgDegreeColumnParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class AvgDegreeColumn
    : public detail::DegreeStatistic<AvgDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                     AvgDegreeColumnParams, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<AvgDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                  AvgDegreeColumnParams, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  AvgDegreeColumn() = default;
  AvgDegreeColumn(const AvgDegreeColumn &) = default;
  static constexpr unsigned kFlags = 0;
  static FeatureType *Compute(const sbxstat_degrees &s) { return new FeatureType(detail::StatAvg<FeatureType>(s)); }

  FeatureType *GetAvgDegreeColumn(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, FeatureType *> GetAvgDegreeColumnCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSC} implementation
  static FeatureType *GetAvgDegreeColumnCSC(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
