// sparsebase/feature/coefficient_of_variation_degree_column.h — feature::CoefficientOfVariationDegreeColumn
// (reference: feature/coefficient_of_variation_degree_column.h, coefficient_of_variation_degree_column.cc:126-142):
// StandardDeviationDegreeColumn over the average degree (NaN without entries, as in the reference).
// The façade and the {CSC} (staged) and {HIPCSC} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_COEFFICIENT_OF_VARIATION_DEGREE_COLUMN_H_
#define SPARSEBASE_FEATURE_COEFFICIENT_OF_VARIATION_DEGREE_COLUMN_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

struct CoefficientOfVariationDegreeColumnParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class CoefficientOfVariationDegreeColumn
    : public detail::DegreeStatistic<CoefficientOfVariationDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                     CoefficientOfVariationDegreeColumnParams, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<CoefficientOfVariationDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                  CoefficientOfVariationDegreeColumnParams, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  CoefficientOfVariationDegreeColumn() = default;
  CoefficientOfVariationDegreeColumn(const CoefficientOfVariationDegreeColumn &) = default;
  static constexpr unsigned kFlags = 0;
  static FeatureType *Compute(const sbxstat_degrees &s) { return new FeatureType(detail::StatCoefficientOfVariation<FeatureType>(s)); }

  FeatureType *GetCoefficientOfVariationDegreeColumn(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, FeatureType *> GetCoefficientOfVariationDegreeColumnCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSC} implementation
  static FeatureType *GetCoefficientOfVariationDegreeColumnCSC(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
