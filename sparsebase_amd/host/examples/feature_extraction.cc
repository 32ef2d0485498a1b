// Feature extraction in one call: read a Matrix Market file, ask feature::FeatureExtractor for Degrees,
// DegreeDistribution, Bandwidth and Profile, print the classes it runs for them (the two fused ones:
// Degrees_DegreeDistribution and Bandwidth_Profile) and the values.  The matrix is moved to the device once; both
// classes then run in place on the HIPCSR.
// Usage: feature_extraction <matrix.mtx>
#include <algorithm>
#include <iostream>

#include "sparsebase/sparsebase.h"

using namespace sparsebase;
using vertex_type = int;
using edge_type = int;
using feature_type = double;
using Deg = feature::Degrees<vertex_type, edge_type, void>;
using Dist = feature::DegreeDistribution<vertex_type, edge_type, void, feature_type>;
using Bw = feature::Bandwidth<vertex_type, edge_type, void>;
using Pr = feature::Profile<vertex_type, edge_type, void>;

int main(int argc, char *argv[]) {
  if (argc < 2) {
    std::cout << "Usage: ./feature_extraction <matrix_market_format>\n";
    return 1;
  }
  context::HIPContext gpu(0);
  auto *coo = bases::IOBase::ReadMTXToCOO<vertex_type, edge_type, void>(argv[1], true);
  auto *dcsr = coo->Convert<format::HIPCSR>(&gpu);
  const vertex_type n = dcsr->get_dimensions()[0];
  std::cout << "Rows: " << n << "\nNonzeros: " << dcsr->get_num_nnz() << std::endl;

  feature::Extractor engine = feature::FeatureExtractor<vertex_type, edge_type, void, feature_type>();
  engine.Add(feature::Feature(Deg{}));
  engine.Add(feature::Feature(Dist{}));
  engine.Add(feature::Feature(Bw{}));
  engine.Add(feature::Feature(Pr{}));
  try {  // a feature of another feature type is not registered
    engine.Add(feature::Feature(feature::DegreeDistribution<vertex_type, edge_type, void, float>{}));
  } catch (utils::FeatureException &ex) {
    std::cout << ex.what() << std::endl;
  }
  std::cout << "Classes used:" << std::endl;
  for (auto *cls : engine.GetClasses()) std::cout << "  " << utils::demangle(cls->get_id()) << std::endl;

  auto raw = engine.Extract(dcsr, {&gpu}, false);
  auto *degrees = std::any_cast<vertex_type *>(raw[Deg::get_id_static()]);
  auto *dist = std::any_cast<feature_type *>(raw[Dist::get_id_static()]);
  auto *bandwidth = std::any_cast<int *>(raw[Bw::get_id_static()]);
  auto *profile = std::any_cast<vertex_type *>(raw[Pr::get_id_static()]);
  const vertex_type hub = (vertex_type)(std::max_element(degrees, degrees + n) - degrees);
  std::cout << "largest degree: " << degrees[hub] << " (row " << hub << ", " << dist[hub] << " of the nonzeros)\n"
            << "bandwidth: " << *bandwidth << "\nprofile: " << *profile << std::endl;
  delete[] degrees;
  delete[] dist;
  delete bandwidth;
  delete profile;
  delete dcsr;
  delete coo;
  return 0;
}
