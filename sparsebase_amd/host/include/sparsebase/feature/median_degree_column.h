// sparsebase/feature/median_degree_column.h — feature::MedianDegreeColumn (reference: feature/median_degree_column.h,
// median_degree_column.cc:131-151): the median degree of a CSC's columns: a radix select on the device where the
// reference sorts.
// The façade and the {CSC} (staged) and {HIPCSC} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_MEDIAN_DEGREE_COLUMN_H_
#define SPARSEBASE_FEATURE_MEDIAN_DEGREE_COLUMN_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

struct MedianDegreeColumnParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class MedianDegreeColumn
    : public detail::DegreeStatistic<MedianDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                     MedianDegreeColumnParams, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<MedianDegreeColumn<IDType, NNZType, ValueType, FeatureType>, detail::OverColumns, FeatureType,
                                  MedianDegreeColumnParams, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  MedianDegreeColumn() = default;
  MedianDegreeColumn(const MedianDegreeColumn &) = default;
  static constexpr unsigned kFlags = SBXSTAT_MEDIAN;
  static FeatureType *Compute(const sbxstat_degrees &s) { return new FeatureType(detail::StatMedian<FeatureType>(s)); }

  FeatureType *GetMedianDegreeColumn(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, FeatureType *> GetMedianDegreeColumnCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSC} implementation
  static FeatureType *GetMedianDegreeColumnCSC(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
