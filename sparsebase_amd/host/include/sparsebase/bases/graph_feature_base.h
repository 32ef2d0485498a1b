// GraphFeatureBase — static one-liner facade over feature::Degrees and feature::DegreeDistribution (reference:
// bases/graph_feature_base.h:20-133).  Signatures follow the reference so call sites compile unchanged.  The arrays
// have get_dimensions()[0] entries and are the caller's (delete[]); the formats of the cached forms are the ones the
// conversion of the input made, the caller's too.
#ifndef SPARSEBASE_BASES_GRAPH_FEATURE_BASE_H_
#define SPARSEBASE_BASES_GRAPH_FEATURE_BASE_H_
#include <tuple>
#include <utility>
#include <vector>

#include "sparsebase/feature/degree_distribution.h"
#include "sparsebase/feature/degrees.h"

namespace sparsebase::bases {

class GraphFeatureBase {
  template <typename I, typename N, typename V>
  using F2 = format::FormatOrderTwo<I, N, V>;

  template <typename I, typename N, typename V>
  static std::vector<F2<I, N, V> *> Cast(const std::vector<format::Format *> &in) {
    std::vector<F2<I, N, V> *> out;
    for (auto *f : in) out.push_back(static_cast<F2<I, N, V> *>(f));
    return out;
  }

 public:
  template <typename FeatureType, typename AutoIDType, typename AutoNNZType, typename AutoValueType>
  static FeatureType *GetDegreeDistribution(F2<AutoIDType, AutoNNZType, AutoValueType> *format,
                                            std::vector<context::Context *> contexts, bool convert_input) {
    feature::DegreeDistribution<AutoIDType, AutoNNZType, AutoValueType, FeatureType> dist;
    return dist.GetDistribution(format, contexts, convert_input);
  }
  template <typename FeatureType, typename AutoIDType, typename AutoNNZType, typename AutoValueType>
  static std::pair<std::vector<F2<AutoIDType, AutoNNZType, AutoValueType> *>, FeatureType *> GetDegreeDistributionCached(
      F2<AutoIDType, AutoNNZType, AutoValueType> *format, std::vector<context::Context *> contexts) {
    feature::DegreeDistribution<AutoIDType, AutoNNZType, AutoValueType, FeatureType> dist;
    auto out = dist.GetDistributionCached(format, contexts, true);
    return std::make_pair(Cast<AutoIDType, AutoNNZType, AutoValueType>(std::get<0>(out)[0]), std::get<1>(out));
  }
  // (the reference declares AutoNNZType * here and returns what feature::Degrees gives, an IDType array; the two are
  // one type in every tuple it instantiates.  This layer's Degrees returns IDType *, and so does this.)
  template <typename AutoIDType, typename AutoNNZType, typename AutoValueType>
  static AutoIDType *GetDegrees(F2<AutoIDType, AutoNNZType, AutoValueType> *format,
                                std::vector<context::Context *> contexts, bool convert_input) {
    feature::Degrees<AutoIDType, AutoNNZType, AutoValueType> degrees;
    return degrees.GetDegrees(format, contexts, convert_input);
  }
  template <typename AutoIDType, typename AutoNNZType, typename AutoValueType>
  static std::pair<std::vector<F2<AutoIDType, AutoNNZType, AutoValueType> *>, AutoIDType *> GetDegreesCached(
      F2<AutoIDType, AutoNNZType, AutoValueType> *format, std::vector<context::Context *> contexts) {
    feature::Degrees<AutoIDType, AutoNNZType, AutoValueType> degrees;
    auto out = degrees.GetDegreesCached(format, contexts, true);
    return std::make_pair(Cast<AutoIDType, AutoNNZType, AutoValueType>(std::get<0>(out)[0]), std::get<1>(out));
  }
};

}  // namespace sparsebase::bases
#endif
