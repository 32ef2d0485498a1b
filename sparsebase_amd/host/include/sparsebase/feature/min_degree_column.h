// sparsebase/feature/min_degree_column.h — feature::MinDegreeColumn (reference: feature/min_degree_column.h,
// min_degree_column.cc:92-104): the smallest degree of a CSC's columns.
// The façade and the {CSC} (staged) and {HIPCSC} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_MIN_DEGREE_COLUMN_H_
#define SPARSEBASE_FEATURE_MIN_DEGREE_COLUMN_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType>
class MinDegreeColumn
    : public detail::DegreeStatistic<MinDegreeColumn<IDType, NNZType, ValueType>, detail::OverColumns, NNZType,
                                     utils::Parameters, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<MinDegreeColumn<IDType, NNZType, ValueType>, detail::OverColumns, NNZType,
                                  utils::Parameters, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  MinDegreeColumn() = default;
  MinDegreeColumn(const MinDegreeColumn &) = default;
  static constexpr unsigned kFlags = 0;
  static NNZType *Compute(const sbxstat_degrees &s) { return new NNZType((NNZType)s.min); }

  NNZType *GetMinDegreeColumn(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, NNZType *> GetMinDegreeColumnCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSC} implementation
  static NNZType *GetMinDegreeColumnCSC(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
