// sparsebase/feature/standard_deviation_degree_column.h — feature::StandardDeviationDegreeColumn (reference:
// feature/standard_deviation_degree_column.h, standard_deviation_degree_column.cc:126-142): the root of the sum of
// squared deviations of a CSC's column degrees (not divided by n, as in the reference), from exact integers.
// The façade and the {CSC} (staged) and {HIPCSC} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_STANDARD_DEVIATION_DEGREE_COLUMN_H_
#define SPARSEBASE_FEATURE_STANDARD_DEVIATION_DEGREE_COLUMN_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

struct StandardDeviationDegreeColumnParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class StandardDeviationDegreeColumn
    : public detail::DegreeStatistic<StandardDeviationDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                     StandardDeviationDegreeColumnParams, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<StandardDeviationDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                  StandardDeviationDegreeColumnParams, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  StandardDeviationDegreeColumn() = default;
  StandardDeviationDegreeColumn(const StandardDeviationDegreeColumn &) = default;
  static constexpr unsigned kFlags = 0;
  static FeatureType *Compute(const sbxstat_degrees &s) { return new FeatureType(detail::StatStandardDeviation<FeatureType>(s)); }

  FeatureType *GetStandardDeviationDegreeColumn(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, FeatureType *> GetStandardDeviationDegreeColumnCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSC} implementation
  static FeatureType *GetStandardDeviationDegreeColumnCSC(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
