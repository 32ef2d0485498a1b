// sparsebase/feature/max_degree.h — feature::MaxDegree (reference: feature/max_degree.h, max_degree.cc:92-104): the
// largest degree of a CSR's rows.
// The façade and the {CSR} (staged) and {HIPCSR} (in place) implementations are feature/degree_stats.h's.
#ifndef SPARSEBASE_FEATURE_MAX_DEGREE_H_
#define SPARSEBASE_FEATURE_MAX_DEGREE_H_
#include "sparsebase/feature/degree_stats.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType>
class MaxDegree
    : public detail::DegreeStatistic<MaxDegree<IDType, NNZType, ValueType>, detail::OverRows, NNZType,
                                     utils::Parameters, IDType, NNZType, ValueType> {
  typedef detail::DegreeStatistic<MaxDegree<IDType, NNZType, ValueType>, detail::OverRows, NNZType,
                                  utils::Parameters, IDType, NNZType, ValueType> Base;

 public:
  using Base::Base;
  MaxDegree() = default;
  MaxDegree(const MaxDegree &) = default;
  static constexpr unsigned kFlags = 0;
  static NNZType *Compute(const sbxstat_degrees &s) { return new NNZType((NNZType)s.max); }

  NNZType *GetMaxDegree(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Get(format, c, convert_input);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, NNZType *> GetMaxDegreeCached(
      format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->GetCached(format, c, convert_input);
  }
  // the reference's name for the {CSR} implementation
  static NNZType *GetMaxDegreeCSR(std::vector<format::Format *> formats, utils::Parameters *p) {
    return Base::OnHost(formats, p);
  }
};

}  // namespace sparsebase::feature
#endif
