// Counterpart of examples/example_experiment/example_experiment.cu:195-278: an experiment over two files (a Matrix Market
// file and an edge list), two preprocesses (the data as loaded, and RCM) and the SpMV kernel, once on host formats that
// are staged through the device on every call and once on formats that live in HBM.  The vectors are filled from a fixed
// seed, so two runs print the same results.
// Usage: example_experiment <symmetric.mtx> <symmetric edge list>
#include <algorithm>
#include <iostream>
#include <memory>
#include <random>

#include "sparsebase/sparsebase.h"

using namespace sparsebase;

using row_type = unsigned int;
using nnz_type = unsigned int;
using value_type = unsigned int;

#define NUM_RUNS 2

static float *fill_r(size_t size, unsigned seed) {
  std::mt19937 rnd(seed);
  std::uniform_real_distribution<float> dist(-1, 1);
  float *arr = new float[size];
  for (size_t i = 0; i < size; i++) arr[i] = dist(rnd);
  return arr;
}

template <template <typename, typename, typename> typename ReaderType>
static std::pair<size_t, size_t> shape_of(const std::string &path) {
  std::unique_ptr<format::CSR<row_type, nnz_type, value_type>> csr(ReaderType<row_type, nnz_type, value_type>(path).ReadCSR());
  return {csr->get_dimensions()[1], csr->get_num_nnz()};
}

int main(int argc, char **argv) {
  if (argc < 3) {
    std::cout << "Usage: ./example_experiment <matrix_market_format> <edge_list_format>\n";
    return 1;
  }
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  const auto mtx = shape_of<io::MTXReader>(argv[1]), edges = shape_of<io::EdgeListReader>(argv[2]);

  // the vectors the kernels multiply by, one per file, on the host and in HBM
  format::Array<float> mtx_v(mtx.first, fill_r(mtx.first, 1), format::kOwned);
  format::Array<float> edges_v(edges.first, fill_r(edges.first, 2), format::kOwned);
  format::HIPArray<float> mtx_dv(mtx.first, dev.Upload(mtx_v.get_vals(), mtx.first), gpu);
  format::HIPArray<float> edges_dv(edges.first, dev.Upload(edges_v.get_vals(), edges.first), gpu);
  // values large enough for both files: the matrices are <unsigned, unsigned, unsigned>, the values come with the kernel
  const size_t most = std::max(mtx.second, edges.second);
  format::Array<float> vals_v(most, fill_r(most, 3), format::kOwned);
  format::HIPArray<float> vals_dv(most, dev.Upload(vals_v.get_vals(), most), gpu);

  reorder::RCMReorder<row_type, nnz_type, value_type>::ParamsType params = {};
  std::vector<std::string> files = {argv[1]}, files2 = {argv[2]};

  experiment::ConcreteExperiment staged, resident;
  staged.AddDataLoader(experiment::LoadCSR<io::MTXReader, row_type, nnz_type, value_type>, {std::make_pair(files, mtx_v)});
  staged.AddDataLoader(experiment::LoadCSR<io::EdgeListReader, row_type, nnz_type, value_type>,
                       {std::make_pair(files2, edges_v)});
  staged.AddPreprocess("original", experiment::Pass, {});  // the kernels on the data as it was loaded
  staged.AddPreprocess("RCM",
                       experiment::Reorder<reorder::RCMReorder, format::CSR, context::CPUContext, row_type, nnz_type, value_type>,
                       params);
  staged.AddKernel("hip-staged", experiment::SpMV<row_type, nnz_type, value_type, float>, vals_v);

  resident.AddDataLoader(experiment::LoadHIPCSR<io::MTXReader, row_type, nnz_type, value_type>,
                         {std::make_pair(files, mtx_dv)});
  resident.AddDataLoader(experiment::LoadHIPCSR<io::EdgeListReader, row_type, nnz_type, value_type>,
                         {std::make_pair(files2, edges_dv)});
  resident.AddPreprocess("original", experiment::Pass, {});
  resident.AddPreprocess("RCM", experiment::ReorderHIP<reorder::RCMReorder, row_type, nnz_type, value_type>, params);
  resident.AddKernel("hip-resident", experiment::SpMV<row_type, nnz_type, value_type, float>, vals_dv);

  staged.Run(NUM_RUNS, true);
  resident.Run(NUM_RUNS, true);

  for (auto *exp : {&staged, &resident}) {
    std::cout << "Results: " << std::endl;
    for (auto &r : exp->GetResults()) {
      std::cout << r.first << ": ";
      auto result = std::any_cast<float *>(r.second[0]);
      for (unsigned int t = 0; t < 8; t++) std::cout << result[t] << " ";
      std::cout << std::endl;
      delete[] result;
    }
    std::cout << std::endl << "Auxiliary Data: " << std::endl;
    for (const auto &a : exp->GetAuxiliary()) std::cout << a.first << std::endl;
    std::cout << std::endl << "Runtimes: " << std::endl;
    for (const auto &s : exp->GetRunTimes()) {
      std::cout << s.first << ": ";
      for (auto sr : s.second) std::cout << sr << " ";
      std::cout << std::endl;
    }
    std::cout << std::endl;
  }
  return 0;
}
