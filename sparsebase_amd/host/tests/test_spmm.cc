// kernels::SpMM (kernels/spmm.h) and the experiment::SpMM kernel function.  Usage: test_spmm <path of a file to write> [filter]
//
// The program writes its own matrix to the path it is given: a structurally symmetric graph of SYM_N vertices (RCM takes
// it) of more entries than one span of the device kernel.  Values and X are small integers, so every sum is exact in float
// whatever its order and the comparisons are equalities: host-staged against device-resident against a plain loop for
// k = 1, 3, 64 and 130, every operand-size and device-mismatch exception, and experiment::SpMM through ConcreteExperiment
// with Pass and with RCMReorder on the device, where P (A X) is compared.
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

std::string SYM_NAME;  // argv[1]
constexpr unsigned SYM_N = 600;
const size_t KS[] = {1, 3, 64, 130};

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

// integer-valued floats: every sum below is exact in float, whatever its order
std::vector<float> SmallInts(size_t count, unsigned seed) {
  std::vector<float> v(count);
  for (auto &t : v) t = (float)((int)((seed = seed * 1664525u + 1013904223u) >> 24) % 17 - 8);
  return v;
}

std::vector<float> PlainLoop(HostCSR *a, const float *x, size_t k, const float *vals) {
  const vertex_type n = a->get_dimensions()[0];
  std::vector<float> y((size_t)n * k, 0.0f);
  for (vertex_type i = 0; i < n; i++)
    for (edge_type p = a->get_row_ptr()[i]; p < a->get_row_ptr()[i + 1]; p++)
      for (size_t j = 0; j < k; j++) y[i * k + j] += (vals ? vals[p] : 1.0f) * x[(size_t)a->get_col()[p] * k + j];
  return y;
}

bool Same(const float *got, const std::vector<float> &want, size_t k) {
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != want[i]) {
      std::printf("  row %zu column %zu: %g for %g\n", i / k, i % k, (double)got[i], (double)want[i]);
      return false;
    }
  return true;
}

}  // namespace

TEST(Kernels, SpMMStagedAgainstResidentAgainstAPlainLoop) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  std::unique_ptr<DevCSR> d(a->Convert<format::HIPCSR>(&gpu));
  const size_t n = a->get_dimensions()[0], m = a->get_dimensions()[1], nnz = a->get_num_nnz();
  EXPECT_TRUE(nnz > 2048);
  auto vals = SmallInts(nnz, 5);
  format::Array<float> vals_host(nnz, vals.data());
  format::HIPArray<float> vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);
  for (size_t k : KS) {
    auto x = SmallInts(m * k, 3 + (unsigned)k);
    const auto want = PlainLoop(a.get(), x.data(), k, vals.data()), want_pattern = PlainLoop(a.get(), x.data(), k, nullptr);
    format::Array<float> x_host(m * k, x.data());
    format::HIPArray<float> x_dev(m * k, dev.Upload(x.data(), m * k), gpu);
    std::unique_ptr<format::Array<float>> y(kernels::SpMM(a.get(), &x_host, k, &vals_host));
    EXPECT_EQ(y->get_num_nnz(), n * k);
    EXPECT_TRUE(Same(y->get_vals(), want, k));
    y.reset(kernels::SpMM(a.get(), &x_host, k));  // unsigned values, float operands: a pattern
    EXPECT_TRUE(Same(y->get_vals(), want_pattern, k));
    std::unique_ptr<format::HIPArray<float>> yd(kernels::SpMM(d.get(), &x_dev, k, &vals_dev));
    EXPECT_EQ(yd->get_num_nnz(), n * k);
    std::unique_ptr<float[]> back(dev.Download(yd->get_vals(), n * k));
    EXPECT_TRUE(Same(back.get(), want, k));
    yd.reset(kernels::SpMM(d.get(), &x_dev, k));
    back.reset(dev.Download(yd->get_vals(), n * k));
    EXPECT_TRUE(Same(back.get(), want_pattern, k));
  }
}

TEST(Kernels, SpMMOwnValuesAndDoubles) {
  context::HIPContext gpu(hip::DefaultDevice());
  // 3 x 4 with its own float values, an empty row, a duplicate column; X is 4 x 2
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, x[] = {1, 2, 10, 20, 100, 200, 1000, 2000}, other[] = {1, 1, 1, 1, 1};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  format::Array<float> x_host(8, x), other_host(5, other);
  std::unique_ptr<format::Array<float>> y(kernels::SpMM(&a, &x_host, 2));
  EXPECT_EQ(y->get_num_nnz(), 6u);
  const float want[] = {302, 604, 0, 0, 5030, 10060}, want_other[] = {201, 402, 0, 0, 1010, 2020};
  for (int i = 0; i < 6; i++) EXPECT_TRUE(y->get_vals()[i] == want[i]);
  y.reset(kernels::SpMM(&a, &x_host, 2, &other_host));
  for (int i = 0; i < 6; i++) EXPECT_TRUE(y->get_vals()[i] == want_other[i]);
  format::CSR<int, int, int> pattern(3, 4, rp, col, nullptr, format::kNotOwned, true);
  double xd[] = {1, 2, 10, 20, 100, 200, 1000, 2000};
  format::Array<double> xd_host(8, xd);
  std::unique_ptr<format::Array<double>> yp(kernels::SpMM(&pattern, &xd_host, 2));
  for (int i = 0; i < 6; i++) EXPECT_TRUE(yp->get_vals()[i] == (double)want_other[i]);
  // k = 0: an empty product
  std::unique_ptr<format::Array<float>> none(kernels::SpMM(&a, &x_host, 0));
  EXPECT_EQ(none->get_num_nnz(), 0u);
}

TEST(Kernels, SpMMExceptions) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, x[] = {1, 2, 10, 20, 100, 200, 1000, 2000};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  std::unique_ptr<format::HIPCSR<int, int, float>> d(a.Convert<format::HIPCSR>(&gpu));
  // operand sizes, host and device: X below m * k values, a values array below nnz
  format::Array<float> x_host(8, x), short_x(7, x), short_vals(4, vals);
  EXPECT_THROW(delete kernels::SpMM(&a, &short_x, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMM(&a, &x_host, 3), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMM(&a, &x_host, 2, &short_vals), utils::TypeException);
  float *dx = dev.Upload(x, 8), *dv = dev.Upload(vals, 5);
  format::HIPArray<float> x_dev(8, dx, gpu, format::kNotOwned), x_dev_short(7, dx, gpu, format::kNotOwned);
  format::HIPArray<float> vals_dev(5, dv, gpu, format::kNotOwned), vals_dev_short(4, dv, gpu, format::kNotOwned);
  EXPECT_THROW(delete kernels::SpMM(d.get(), &x_dev_short, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMM(d.get(), &x_dev, 2, &vals_dev_short), utils::TypeException);
  EXPECT_NO_THROW(delete kernels::SpMM(d.get(), &x_dev, 2, &vals_dev));
  // device mismatch: an operand whose context names another device than the matrix's
  format::HIPArray<float> x_elsewhere(8, dx, gpu, format::kNotOwned), vals_elsewhere(5, dv, gpu, format::kNotOwned);
  x_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  vals_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  EXPECT_THROW(delete kernels::SpMM(d.get(), &x_elsewhere, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMM(d.get(), &x_dev, 2, &vals_elsewhere), utils::TypeException);
  // the kernel function: a parameter that is no SpMMParams, an X of another type, a values array of another type
  DataMap data = {{"processed_format", &a}};
  std::any fp = x_host, pp, kp = SpMMParams{2, {}}, not_params = 2, wrong_x = format::Array<double>(0, nullptr);
  std::any wrong_vals = SpMMParams{2, format::Array<double>(0, nullptr)};
  EXPECT_THROW((SpMM<int, int, float, float>(data, fp, pp, not_params)), utils::TypeException);
  EXPECT_THROW((SpMM<int, int, float, float>(data, wrong_x, pp, kp)), utils::TypeException);
  EXPECT_THROW((SpMM<int, int, float, float>(data, fp, pp, wrong_vals)), utils::TypeException);
  float *y = std::any_cast<float *>(SpMM<int, int, float, float>(data, fp, pp, kp));
  EXPECT_TRUE(y[0] == 302.0f && y[1] == 604.0f && y[2] == 0.0f && y[5] == 10060.0f);
  delete[] y;
  dev.Free(dx);
  dev.Free(dv);
}

TEST(Experiment, SpMMWithPass) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t m = a->get_dimensions()[1], nnz = a->get_num_nnz(), k = 3;
  auto x = SmallInts(m * k, 13), vals = SmallInts(nnz, 15);
  const auto want = PlainLoop(a.get(), x.data(), k, vals.data()), want_pattern = PlainLoop(a.get(), x.data(), k, nullptr);
  format::Array<float> x_host(m * k, x.data()), vals_host(nnz, vals.data());
  format::HIPArray<float> x_dev(m * k, dev.Upload(x.data(), m * k), gpu), vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);

  ConcreteExperiment staged, resident;
  staged.AddDataLoader(LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_host)});
  resident.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  for (auto *e : {&staged, &resident}) e->AddPreprocess("original", Pass, {});
  staged.AddKernel("spmm", SpMM<vertex_type, edge_type, value_type, float>, SpMMParams{k, vals_host});
  resident.AddKernel("spmm", SpMM<vertex_type, edge_type, value_type, float>, SpMMParams{k, vals_dev});
  for (auto *e : {&staged, &resident}) {
    e->AddKernel("pattern", SpMM<vertex_type, edge_type, value_type, float>, SpMMParams{k, {}});
    e->Run(2, true);
    auto res = e->GetResults();
    EXPECT_EQ(res.size(), 4u);
    for (int i = 0; i < 2; i++) {
      float *y = std::any_cast<float *>(res["-" + SYM_NAME + ",original,spmm," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(y, want, k));
      delete[] y;
      y = std::any_cast<float *>(res["-" + SYM_NAME + ",original,pattern," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(y, want_pattern, k));
      delete[] y;
    }
    auto aux = e->GetAuxiliary();
    EXPECT_EQ(aux.size(), 2u);
    delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
    EXPECT_TRUE(e->GetRunTimes()["-" + SYM_NAME + ",original,spmm,1"][0] > 0.0);
  }
}

TEST(Experiment, SpMMRcmPipelineOnTheDevice) {
  context::CPUContext cpu;
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0], k = 64;
  EXPECT_EQ(n, (size_t)SYM_N);
  std::unique_ptr<vertex_type[]> order(bases::ReorderBase::Reorder<reorder::RCMReorder>({}, a.get(), {&cpu}, true));
  // X' = P X is what the kernel gets; the permuted product is Y'[order[i], :] = sum over row i of X'[order[j], :]
  auto xp = SmallInts(n * k, 19);
  std::vector<float> x(n * k), want(n * k);
  for (size_t r = 0; r < n; r++)
    for (size_t j = 0; j < k; j++) x[r * k + j] = xp[(size_t)order[r] * k + j];
  const auto y = PlainLoop(a.get(), x.data(), k, nullptr);
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < k; j++) want[(size_t)order[i] * k + j] = y[i * k + j];
  format::HIPArray<float> x_dev(n * k, dev.Upload(xp.data(), n * k), gpu);

  ConcreteExperiment exp;
  exp.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  reorder::RCMReorder<vertex_type, edge_type, value_type>::ParamsType params = {};
  exp.AddPreprocess("RCM", ReorderHIP<reorder::RCMReorder, vertex_type, edge_type, value_type>, params);
  exp.AddKernel("spmm", SpMM<vertex_type, edge_type, value_type, float>, SpMMParams{k, {}});
  exp.Run(1, true);
  auto res = exp.GetResults();
  EXPECT_EQ(res.size(), 1u);
  float *got = std::any_cast<float *>(res["-" + SYM_NAME + ",RCM,spmm,0"][0]);
  EXPECT_TRUE(Same(got, want, k));
  delete[] got;
  auto aux = exp.GetAuxiliary();
  EXPECT_EQ(aux.size(), 2u);
  delete std::any_cast<format::Format *>(aux["processed_format,-" + SYM_NAME + ",RCM"]);
  delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("Usage: test_spmm <path of a file to write> [filter]\n");
    return 2;
  }
  SYM_NAME = argv[1];
  WriteSymmetricGraph(SYM_NAME);
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
