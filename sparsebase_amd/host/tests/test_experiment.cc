// experiment:: — ConcreteExperiment, the loaders and preprocess functions of experiment_helper.h, the SpMV kernel function
// and kernels/spmv.h.  Usage: test_experiment <ash958.mtx> [filter]
//
// The first part restates what the reference's suites assert (tests/suites/sparsebase/experiment/): the sizes of the three
// maps after Run(2, true), Run() and Run(3, true), the exact id strings, the `incomplete` sequence, one "format" entry of
// the right type per loader, "processed_format" from every preprocess function.  One difference is this project's own:
// its RCM refuses a pattern that is not structurally symmetric and ash958 is 958 x 292, so ReorderCSR and
// Reorder run on a symmetric graph this program writes next to the file it was given.
// The second part is this project's ground: SpMV through the harness host-staged against device-resident against a plain
// loop, the LoadHIPCSR -> ReorderHIP<RCMReorder> -> SpMV pipeline, duplicate ids, kernels::SpMV and kernels::CheckCSR.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;
using namespace sparsebase::experiment;

namespace {

using vertex_type = unsigned int;
using edge_type = unsigned int;
using value_type = unsigned int;
typedef format::CSR<vertex_type, edge_type, value_type> HostCSR;
typedef format::HIPCSR<vertex_type, edge_type, value_type> DevCSR;

std::string FILE_NAME;  // argv[1]
std::string SYM_NAME;   // a symmetric graph of SYM_N vertices, written by main()
constexpr unsigned SYM_N = 600;

void WriteSymmetricGraph(const std::string &path) {
  std::set<std::pair<unsigned, unsigned>> e;
  for (unsigned i = 0; i < SYM_N; i++)
    for (unsigned j : {(i + 1) % SYM_N, (i * 7 + 3) % SYM_N, (i * i + 11) % SYM_N})
      if (i != j) {
        e.insert({i, j});
        e.insert({j, i});
      }
  FILE *f = std::fopen(path.c_str(), "w");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate pattern general\n%u %u %zu\n", SYM_N, SYM_N, e.size());
  for (auto &p : e) std::fprintf(f, "%u %u\n", p.first + 1, p.second + 1);
  std::fclose(f);
}

DataMap load_data_f(std::vector<std::string> &file_names) {
  return {{"format", io::MTXReader<vertex_type, edge_type, value_type>(FILE_NAME).ReadCSR()}};
}
void preprocess_f(DataMap &data, std::any &fparams, std::any &params) { data.emplace("new_format", data["format"]); }
std::any kernel_f(DataMap &data, std::any &fparams, std::any &pparams, std::any &kparams) { return {}; }

struct Fixture {
  ConcreteExperiment exp;
  std::any fparams;
  std::vector<std::string> files = {FILE_NAME};
  Fixture() {
    exp.AddDataLoader(load_data_f, {std::make_pair(files, fparams)});
    exp.AddPreprocess("pid", preprocess_f, {});
    exp.AddKernel("kid", kernel_f, {});
  }
};

// integer-valued floats: every sum below is exact in float, whatever its order
std::vector<float> SmallInts(size_t count, unsigned seed) {
  std::vector<float> v(count);
  for (auto &t : v) t = (float)((int)((seed = seed * 1664525u + 1013904223u) >> 24) % 17 - 8);
  return v;
}

// the plain loop of the reference example's single-threaded kernel
std::vector<float> PlainLoop(HostCSR *a, const float *x, const float *vals) {
  const vertex_type n = a->get_dimensions()[0];
  std::vector<float> y(n);
  for (vertex_type i = 0; i < n; i++) {
    float s = 0;
    for (edge_type p = a->get_row_ptr()[i]; p < a->get_row_ptr()[i + 1]; p++) s += (vals ? vals[p] : 1.0f) * x[a->get_col()[p]];
    y[i] = s;
  }
  return y;
}

bool Same(const float *got, const std::vector<float> &want) {
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != want[i]) {
      std::printf("  row %zu: %g for %g\n", i, (double)got[i], (double)want[i]);
      return false;
    }
  return true;
}

}  // namespace

// ---- the reference's suites
TEST(Experiment, basics) {
  Fixture f;
  f.exp.Run(2, true);
  EXPECT_EQ(f.exp.GetAuxiliary().size(), 2u);
  EXPECT_EQ(f.exp.GetResults().size(), 2u);
  EXPECT_EQ(f.exp.GetRunTimes().size(), 2u);
}

TEST(Experiment, basics2) {
  Fixture f;
  f.exp.Run();
  EXPECT_EQ(f.exp.GetAuxiliary().size(), 0u);
  EXPECT_EQ(f.exp.GetResults().size(), 1u);
  EXPECT_EQ(f.exp.GetRunTimes().size(), 1u);
}

TEST(Experiment, identifiers) {
  Fixture f;
  f.exp.Run(3, true);
  auto aux = f.exp.GetAuxiliary();
  auto res = f.exp.GetResults();
  auto rtimes = f.exp.GetRunTimes();
  EXPECT_EQ(aux.size(), 2u);
  EXPECT_TRUE(aux.count("format,-" + FILE_NAME) == 1);
  EXPECT_TRUE(aux.count("new_format,-" + FILE_NAME + ",pid") == 1);
  EXPECT_TRUE(std::any_cast<format::Format *>(aux["format,-" + FILE_NAME])->IsAbsolute<HostCSR>());
  EXPECT_EQ(res.size(), 3u);
  EXPECT_EQ(rtimes.size(), 3u);
  for (int i = 0; i < 3; i++) {
    const std::string id = "-" + FILE_NAME + ",pid,kid," + std::to_string(i);
    EXPECT_TRUE(res.count(id) == 1 && res[id].size() == 1);
    EXPECT_TRUE(rtimes.count(id) == 1 && rtimes[id].size() == 1 && rtimes[id][0] >= 0.0);
  }
  // a second Run appends to the same keys; two file names give "-a-b"
  f.exp.Run(1);
  EXPECT_EQ(f.exp.GetResults()["-" + FILE_NAME + ",pid,kid,0"].size(), 2u);
  EXPECT_EQ(f.exp.GetResults().size(), 3u);
  ConcreteExperiment two;
  two.AddDataLoader(load_data_f, {std::make_pair(std::vector<std::string>{"a", "b"}, std::any())});
  two.AddPreprocess("p", preprocess_f, {});
  two.AddKernel("k", kernel_f, {});
  two.Run(1, true);
  EXPECT_TRUE(two.GetResults().count("-a-b,p,k,0") == 1);
  EXPECT_TRUE(two.GetAuxiliary().count("format,-a-b") == 1 && two.GetAuxiliary().count("new_format,-a-b,p") == 1);
}

TEST(Experiment, incomplete) {
  ConcreteExperiment exp;
  std::any fparams;
  std::vector<std::string> files = {FILE_NAME};
  exp.AddDataLoader(load_data_f, {std::make_pair(files, fparams)});
  exp.Run(3, true);
  EXPECT_EQ(exp.GetAuxiliary().size(), 1u);
  EXPECT_EQ(exp.GetResults().size(), 0u);
  exp.AddPreprocess("id", preprocess_f, {});
  exp.Run(3);
  EXPECT_EQ(exp.GetAuxiliary().size(), 1u);
  exp.Run(3, true);
  EXPECT_EQ(exp.GetAuxiliary().size(), 2u);
}

TEST(Helper, Loaders) {
  std::vector<std::string> files = {FILE_NAME};
  auto csr = LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>(files);
  EXPECT_EQ(csr.size(), 1u);
  EXPECT_TRUE(csr.count("format") == 1 && csr["format"]->IsAbsolute<HostCSR>());
  EXPECT_EQ(csr["format"]->get_dimensions()[0], 958u);
  EXPECT_EQ(csr["format"]->get_num_nnz(), 1916u);
  auto coo = LoadCOO<io::MTXReader, vertex_type, edge_type, value_type>(files);
  EXPECT_EQ(coo.size(), 1u);
  EXPECT_TRUE(coo.count("format") == 1 && (coo["format"]->IsAbsolute<format::COO<vertex_type, edge_type, value_type>>()));
  auto csc = LoadCSC<io::MTXReader, vertex_type, edge_type, value_type>(files);
  EXPECT_EQ(csc.size(), 1u);
  EXPECT_TRUE(csc.count("format") == 1 && (csc["format"]->IsAbsolute<format::CSC<vertex_type, edge_type, value_type>>()));
  auto any = LoadFormat<format::CSR, io::MTXReader, vertex_type, edge_type, value_type>(files);
  EXPECT_EQ(any.size(), 1u);
  EXPECT_TRUE(any.count("format") == 1 && any["format"]->IsAbsolute<HostCSR>());
  auto same = LoadFormat<format::COO, io::MTXReader, vertex_type, edge_type, value_type>(files);
  EXPECT_TRUE((same["format"]->IsAbsolute<format::COO<vertex_type, edge_type, value_type>>()));
  auto dev = LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>(files);
  EXPECT_EQ(dev.size(), 1u);
  EXPECT_TRUE(dev.count("format") == 1 && dev["format"]->IsAbsolute<DevCSR>());
  EXPECT_EQ(dev["format"]->get_num_nnz(), 1916u);
  for (auto *m : {&csr, &coo, &csc, &any, &same, &dev}) delete (*m)["format"];
}

TEST(Helper, PreprocessFunctions) {
  std::vector<std::string> sym = {SYM_NAME}, files = {FILE_NAME};
  std::any p1;
  reorder::RCMReorder<vertex_type, edge_type, value_type>::ParamsType p2 = {};
  auto data = LoadFormat<format::CSR, io::MTXReader, vertex_type, edge_type, value_type>(sym);
  ReorderCSR<reorder::RCMReorder, context::CPUContext, vertex_type, edge_type, value_type>(data, p1, p2);
  EXPECT_EQ(data.size(), 2u);
  EXPECT_TRUE(data.count("processed_format") == 1 && data["processed_format"]->IsAbsolute<HostCSR>());
  EXPECT_TRUE(data["processed_format"] != data["format"]);
  EXPECT_EQ(data["processed_format"]->get_num_nnz(), data["format"]->get_num_nnz());
  delete data["processed_format"];
  data.erase("processed_format");
  Reorder<reorder::RCMReorder, format::CSR, context::CPUContext, vertex_type, edge_type, value_type>(data, p1, p2);
  EXPECT_EQ(data.size(), 2u);
  EXPECT_TRUE(data.count("processed_format") == 1 && data["processed_format"]->IsAbsolute<HostCSR>());
  delete data["processed_format"];
  delete data["format"];
  // as PreprocessFunctions, with DegreeReorder's parameters
  PreprocessFunction fn = Reorder<reorder::DegreeReorder, format::CSR, context::CPUContext, vertex_type, edge_type, value_type>;
  data = LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>(sym);
  std::any degree_params = reorder::DegreeReorderParams(true);
  fn(data, p1, degree_params);
  EXPECT_TRUE(data["processed_format"]->IsAbsolute<HostCSR>());
  delete data["processed_format"];
  delete data["format"];
  // Pass, on the file the reference uses
  data = LoadFormat<format::CSR, io::MTXReader, vertex_type, edge_type, value_type>(files);
  std::any none;
  Pass(data, p1, none);
  EXPECT_EQ(data.size(), 2u);
  EXPECT_TRUE(data.count("processed_format") == 1 && data["processed_format"] == data["format"]);
  delete data["format"];
}

// ---- this project's ground
TEST(SpMV, StagedAgainstResidentAgainstAPlainLoop) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {FILE_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(FILE_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0], m = a->get_dimensions()[1], nnz = a->get_num_nnz();
  auto x = SmallInts(m, 3), vals = SmallInts(nnz, 5);
  const auto want = PlainLoop(a.get(), x.data(), vals.data()), want_pattern = PlainLoop(a.get(), x.data(), nullptr);
  format::Array<float> x_host(m, x.data()), vals_host(nnz, vals.data());
  format::HIPArray<float> x_dev(m, dev.Upload(x.data(), m), gpu), vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);

  ConcreteExperiment staged, resident;
  staged.AddDataLoader(LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_host)});
  resident.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  for (auto *e : {&staged, &resident}) e->AddPreprocess("original", Pass, {});
  staged.AddKernel("spmv", SpMV<vertex_type, edge_type, value_type, float>, vals_host);
  resident.AddKernel("spmv", SpMV<vertex_type, edge_type, value_type, float>, vals_dev);
  for (auto *e : {&staged, &resident}) {
    e->AddKernel("pattern", SpMV<vertex_type, edge_type, value_type, float>, {});
    e->Run(2, true);
    auto res = e->GetResults();
    EXPECT_EQ(res.size(), 4u);
    for (int i = 0; i < 2; i++) {
      float *y = std::any_cast<float *>(res["-" + FILE_NAME + ",original,spmv," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(y, want));
      delete[] y;
      y = std::any_cast<float *>(res["-" + FILE_NAME + ",original,pattern," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(y, want_pattern));
      delete[] y;
    }
    auto aux = e->GetAuxiliary();
    EXPECT_EQ(aux.size(), 2u);  // ("format" from the loader, "processed_format" — the same object — under the preprocess)
    delete std::any_cast<format::Format *>(aux["format,-" + FILE_NAME]);
    EXPECT_TRUE(e->GetRunTimes()["-" + FILE_NAME + ",original,spmv,1"][0] > 0.0);
  }
  EXPECT_EQ(n, want.size());
  // mixed: a resident matrix with host arrays, a host matrix with device arrays
  {
    DataMap data = {{"processed_format", a.get()}};
    std::any fp = x_dev, pp, kp = vals_dev;
    float *y = std::any_cast<float *>(SpMV<vertex_type, edge_type, value_type, float>(data, fp, pp, kp));
    EXPECT_TRUE(Same(y, want));
    delete[] y;
    std::any wrong = format::Array<double>(0, nullptr);
    EXPECT_THROW((SpMV<vertex_type, edge_type, value_type, float>(data, wrong, pp, kp)), utils::TypeException);
  }
}

TEST(SpMV, AuxiliaryOfPass) {
  // Pass stores the loader's own pointer under "processed_format": name,file_id is absent, so it is kept under the pid
  ConcreteExperiment exp;
  std::vector<std::string> files = {FILE_NAME};
  exp.AddDataLoader(LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, std::any())});
  exp.AddPreprocess("original", Pass, {});
  exp.Run(1, true);
  auto aux = exp.GetAuxiliary();
  EXPECT_EQ(aux.size(), 2u);
  EXPECT_TRUE(aux.count("format,-" + FILE_NAME) == 1 && aux.count("processed_format,-" + FILE_NAME + ",original") == 1);
  delete std::any_cast<format::Format *>(aux["format,-" + FILE_NAME]);
}

TEST(SpMV, RcmPipelineOnTheDevice) {
  context::CPUContext cpu;
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0];
  EXPECT_EQ(n, (size_t)SYM_N);
  std::unique_ptr<vertex_type[]> order(bases::ReorderBase::Reorder<reorder::RCMReorder>({}, a.get(), {&cpu}, true));
  // x' is what the kernel gets; the permuted product is y'[order[i]] = sum over row i of x'[order[j]]
  auto xp = SmallInts(n, 9);
  std::vector<float> x(n), want(n);
  for (size_t j = 0; j < n; j++) x[j] = xp[order[j]];
  const auto y = PlainLoop(a.get(), x.data(), nullptr);
  for (size_t i = 0; i < n; i++) want[order[i]] = y[i];
  format::HIPArray<float> x_dev(n, dev.Upload(xp.data(), n), gpu);

  ConcreteExperiment exp;
  exp.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  reorder::RCMReorder<vertex_type, edge_type, value_type>::ParamsType params = {};
  exp.AddPreprocess("RCM", ReorderHIP<reorder::RCMReorder, vertex_type, edge_type, value_type>, params);
  exp.AddKernel("spmv", SpMV<vertex_type, edge_type, value_type, float>, {});
  exp.Run(1, true);
  auto res = exp.GetResults();
  EXPECT_EQ(res.size(), 1u);
  float *got = std::any_cast<float *>(res["-" + SYM_NAME + ",RCM,spmv,0"][0]);
  EXPECT_TRUE(Same(got, want));
  delete[] got;
  auto aux = exp.GetAuxiliary();
  EXPECT_EQ(aux.size(), 2u);
  auto *processed = std::any_cast<format::Format *>(aux["processed_format,-" + SYM_NAME + ",RCM"]);
  EXPECT_TRUE(processed->IsAbsolute<DevCSR>());
  EXPECT_NO_THROW(kernels::CheckCSR(processed->AsAbsolute<DevCSR>()));
  delete processed;
  delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
}

TEST(Experiment, DuplicateIdsKeepTheFirstFunction) {
  ConcreteExperiment exp;
  std::vector<std::string> files = {FILE_NAME};
  exp.AddDataLoader(load_data_f, {std::make_pair(files, std::any())});
  exp.AddPreprocess("pid", preprocess_f, {});
  exp.AddPreprocess("pid", [](DataMap &data, std::any &, std::any &) { data.emplace("second", data["format"]); }, {});
  exp.AddKernel("kid", [](DataMap &, std::any &, std::any &, std::any &) -> std::any { return 1; }, {});
  exp.AddKernel("kid", [](DataMap &, std::any &, std::any &, std::any &) -> std::any { return 2; }, {});
  exp.Run(1, true);
  auto res = exp.GetResults();
  EXPECT_EQ(res.size(), 1u);
  EXPECT_EQ(std::any_cast<int>(res["-" + FILE_NAME + ",pid,kid,0"][0]), 1);
  auto aux = exp.GetAuxiliary();
  EXPECT_TRUE(aux.count("new_format,-" + FILE_NAME + ",pid") == 1 && aux.count("second,-" + FILE_NAME + ",pid") == 0);
  delete std::any_cast<format::Format *>(aux["format,-" + FILE_NAME]);
}

TEST(Kernels, SpMVAndCheckCSR) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  // 3 x 4 with its own float values, an empty row, a duplicate column
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, x[] = {1, 10, 100, 1000}, other[] = {1, 1, 1, 1, 1};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  format::Array<float> x_host(4, x), other_host(5, other);
  std::unique_ptr<format::Array<float>> y(kernels::SpMV(&a, &x_host));
  EXPECT_EQ(y->get_num_nnz(), 3u);
  EXPECT_TRUE(y->get_vals()[0] == 302.0f && y->get_vals()[1] == 0.0f && y->get_vals()[2] == 5030.0f);
  y.reset(kernels::SpMV(&a, &x_host, &other_host));
  EXPECT_TRUE(y->get_vals()[0] == 201.0f && y->get_vals()[1] == 0.0f && y->get_vals()[2] == 1010.0f);
  std::unique_ptr<format::HIPCSR<int, int, float>> d(a.Convert<format::HIPCSR>(&gpu));
  format::HIPArray<float> x_dev(4, dev.Upload(x, 4), gpu);
  std::unique_ptr<format::HIPArray<float>> yd(kernels::SpMV(d.get(), &x_dev));
  std::unique_ptr<float[]> back(dev.Download(yd->get_vals(), 3));
  EXPECT_TRUE(back[0] == 302.0f && back[1] == 0.0f && back[2] == 5030.0f);
  // a pattern matrix of another value type, and doubles
  format::CSR<int, int, int> pattern(3, 4, rp, col, nullptr, format::kNotOwned, true);
  double xd[] = {1, 10, 100, 1000};
  format::Array<double> xd_host(4, xd);
  std::unique_ptr<format::Array<double>> yp(kernels::SpMV(&pattern, &xd_host));
  EXPECT_TRUE(yp->get_vals()[0] == 201.0 && yp->get_vals()[2] == 1010.0);
  format::Array<float> short_x(3, x);
  EXPECT_THROW(delete kernels::SpMV(&a, &short_x), utils::TypeException);
  // CheckCSR: the well-formed matrix passes, a column outside the matrix is named with its position
  EXPECT_NO_THROW(kernels::CheckCSR(&a));
  EXPECT_NO_THROW(kernels::CheckCSR(d.get()));
  int bad_col[] = {0, 2, 2, 4, 3};
  format::CSR<int, int, float> bad(3, 4, rp, bad_col, vals, format::kNotOwned, true);
  bool named = false;
  try {
    kernels::CheckCSR(&bad);
  } catch (utils::HIPDeviceException &e) {
    named = std::string(e.what()).find("position 3 lies outside [0, 4)") != std::string::npos;
  }
  EXPECT_TRUE(named);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("Usage: test_experiment <ash958.mtx> [filter]\n");
    return 2;
  }
  FILE_NAME = argv[1];
  SYM_NAME = FILE_NAME + ".symmetric.mtx";
  WriteSymmetricGraph(SYM_NAME);
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
