// sparsebase/feature/min_degree.h — feature::MinDegree (reference: feature/min_degree.h, min_degree.cc:92-104): the
// smallest degree of a CSR's rows.
// The façade and the {CSR} (staged) and {HIPCSR} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_MIN_DEGREE_H_
#define SPARSEBASE_FEATURE_MIN_DEGREE_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType>
class MinDegree
    : public detail::DegreeStatistic<MinDegree<IDType, NNZType, ValueType>, detail::OverRows, NNZType,
                                     utils::Parameters, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<MinDegree<IDType, NNZType, ValueType>, detail::OverRows, NNZType,
                                  utils::Parameters, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  MinDegree() = default;
  MinDegree(const MinDegree &) = default;
  static constexpr unsigned kFlags = 0;
  static NNZType *Compute(const sbxstat_degrees &s) { return new NNZType((NNZType)s.min); }

  NNZType *GetMinDegree(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, NNZType *> GetMinDegreeCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSR} implementation
  static NNZType *GetMinDegreeCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
