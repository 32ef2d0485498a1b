// sparsebase/feature/feature_extractor.h — feature::FeatureExtractor (reference: feature/feature_extractor.h,
// feature_extractor.cc:12-25): the Extractor with this layer's feature classes registered.
//
// The reference registers three classes: DegreeDistribution, Degrees and the fused Degrees_DegreeDistribution.  As a
// superset, every other feature class of this layer that is an Extractable and default-constructible from the four
// type parameters is registered too; the fused ones among them are MinMaxAvgDegree and Bandwidth_Profile.
// (JaccardWeights is no Extractable: it returns a format.)  A feature of another FeatureType is not registered, so
// adding a DegreeDistribution<..., float> to a FeatureExtractor<..., double> throws utils::FeatureException, as in the
// reference's example.
#ifndef SPARSEBASE_FEATURE_FEATURE_EXTRACTOR_H_
#define SPARSEBASE_FEATURE_FEATURE_EXTRACTOR_H_
#include "sparsebase/feature/avg_degree.h"
#include "sparsebase/feature/avg_degree_column.h"
#include "sparsebase/feature/bandwidth.h"
#include "sparsebase/feature/bandwidth_profile.h"
#include "sparsebase/feature/coefficient_of_variation_degree_column.h"
#include "sparsebase/feature/degree_distribution.h"
#include "sparsebase/feature/degrees.h"
#include "sparsebase/feature/degrees_degree_distribution.h"
#include "sparsebase/feature/extractor.h"
#include "sparsebase/feature/geometric_avg_degree_column.h"
#include "sparsebase/feature/max_degree.h"
#include "sparsebase/feature/max_degree_column.h"
#include "sparsebase/feature/median_degree_column.h"
#include "sparsebase/feature/min_degree.h"
#include "sparsebase/feature/min_degree_column.h"
#include "sparsebase/feature/min_max_avg_degree.h"
#include "sparsebase/feature/off_diag_block_nnz.h"
#include "sparsebase/feature/profile.h"
#include "sparsebase/feature/standard_deviation_degree_column.h"
#include "sparsebase/feature/triangle_count.h"

namespace sparsebase::feature {

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class FeatureExtractor : public Extractor {
 public:
  FeatureExtractor() {
    // the reference's three (feature_extractor.cc:12-25)
    Register<DegreeDistribution<IDType, NNZType, ValueType, FeatureType>>();
    Register<Degrees<IDType, NNZType, ValueType>>();
    Register<Degrees_DegreeDistribution<IDType, NNZType, ValueType, FeatureType>>();
    // this layer's other feature classes
    Register<Bandwidth<IDType, NNZType, ValueType>>();
    Register<Profile<IDType, NNZType, ValueType>>();
    Register<Bandwidth_Profile<IDType, NNZType, ValueType>>();
    Register<MinDegree<IDType, NNZType, ValueType>>();
    Register<MaxDegree<IDType, NNZType, ValueType>>();
    Register<AvgDegree<IDType, NNZType, ValueType, FeatureType>>();
    Register<MinMaxAvgDegree<IDType, NNZType, ValueType, FeatureType>>();
    Register<MinDegreeColumn<IDType, NNZType, ValueType>>();
    Register<MaxDegreeColumn<IDType, NNZType, ValueType>>();
    Register<AvgDegreeColumn<IDType, NNZType, ValueType, FeatureType>>();
    Register<MedianDegreeColumn<IDType, NNZType, ValueType, FeatureType>>();
    Register<StandardDeviationDegreeColumn<IDType, NNZType, ValueType, FeatureType>>();
    Register<CoefficientOfVariationDegreeColumn<IDType, NNZType, ValueType, FeatureType>>();
    Register<GeometricAvgDegreeColumn<IDType, NNZType, ValueType, FeatureType>>();
    Register<OffDiagBlockNNZ<IDType, NNZType, ValueType>>();
    Register<TriangleCount<IDType, NNZType, ValueType>>();
  }

 private:
  template <typename Class>
  void Register() {
    auto *cls = new Class();
    this->RegisterClass(cls->get_sub_ids(), cls);
  }
};

}  // namespace sparsebase::feature
#endif
