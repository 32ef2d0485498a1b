// sparsebase/feature/geometric_avg_degree_column.h — feature::GeometricAvgDegreeColumn (reference:
// feature/geometric_avg_degree_column.h, geometric_avg_degree_column.cc:126-139): the geometric mean of a CSC's
// column degrees, 0 when a column is empty.
// The façade and the {CSC} (staged) and {HIPCSC} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_GEOMETRIC_AVG_DEGREE_COLUMN_H_
#define SPARSEBASE_FEATURE_GEOMETRIC_AVG_DEGREE_COLUMN_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

struct GeometricAvgDegreeColumnParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class GeometricAvgDegreeColumn
    : public detail::DegreeStatistic<GeometricAvgDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                     GeometricAvgDegreeColumnParams, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<GeometricAvgDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                  GeometricAvgDegreeColumnParams, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  GeometricAvgDegreeColumn() = default;
  GeometricAvgDegreeColumn(const GeometricAvgDegreeColumn &) = default;
  static constexpr unsigned kFlags = SBXSTAT_LOG;
  static FeatureType *Compute(const sbxstat_degrees &s) { return new FeatureType(detail::StatGeometricAvg<FeatureType>(s)); }

  FeatureType *GetGeometricAvgDegreeColumn(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, FeatureType *> GetGeometricAvgDegreeColumnCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSC} implementation
  static FeatureType *GetGeometricAvgDegreeColumnCSC(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
