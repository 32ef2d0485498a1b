// kernels::TransposePlan, kernels::SpMMTransposed (kernels/spmm_transposed.h) and the experiment::SpMMTransposed kernel
// function.  Usage: test_spmm_t <path of a file to write> [filter]
//
// The program writes its own matrix to the path it is given: a graph of GRAPH_N vertices whose rows are NOT those of its
// transpose (every arc i -> j is stored one way), of more entries than one span of the device kernel.  Values and X are
// small integers, so every sum is exact in float whatever its order and the comparisons are equalities: a plan built from
// the host CSR against one built from the HIPCSR against a plain loop for k = 1, 3, 64 and 130, one plan reused for two
// value arrays, a small rectangle with its plan's arrays spelled out, the operand-size and device-mismatch exceptions,
// and experiment::SpMMTransposed through ConcreteExperiment with and without a plan in its parameter.
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
typedef kernels::TransposePlan<vertex_type, edge_type> Plan;

std::string GRAPH_NAME;  // argv[1]
constexpr unsigned GRAPH_N = 900;
const size_t KS[] = {1, 3, 64, 130};

void WriteGraph(const std::string &path) {
  std::set<std::pair<unsigned, unsigned>> e;
  for (unsigned i = 0; i < GRAPH_N; i++)
    for (unsigned j : {(i + 1) % GRAPH_N, (i * 7 + 3) % GRAPH_N, (i * i + 11) % GRAPH_N, 5u})  // (column 5: a long one)
      if (i != j) e.insert({i, j});
  FILE *f = std::fopen(path.c_str(), "w");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate pattern general\n%u %u %zu\n", GRAPH_N, GRAPH_N, e.size());
  for (auto &p : e) std::fprintf(f, "%u %u\n", p.first + 1, p.second + 1);
  std::fclose(f);
}

// integer-valued floats: every sum below is exact in float, whatever its order
std::vector<float> SmallInts(size_t count, unsigned seed) {
  std::vector<float> v(count);
  for (auto &t : v) t = (float)((int)((seed = seed * 1664525u + 1013904223u) >> 24) % 17 - 8);
  return v;
}

// Y = A^T X: every stored entry (i, c) adds vals[p] * X[i, :] to Y[c, :]
std::vector<float> PlainLoop(HostCSR *a, const float *x, size_t k, const float *vals) {
  const vertex_type n = a->get_dimensions()[0], m = a->get_dimensions()[1];
  std::vector<float> y((size_t)m * k, 0.0f);
  for (vertex_type i = 0; i < n; i++)
    for (edge_type p = a->get_row_ptr()[i]; p < a->get_row_ptr()[i + 1]; p++)
      for (size_t j = 0; j < k; j++) y[(size_t)a->get_col()[p] * k + j] += (vals ? vals[p] : 1.0f) * x[(size_t)i * k + j];
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

TEST(Kernels, SpMMTransposedFromAHostPlanAndADevicePlanAgainstAPlainLoop) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(GRAPH_NAME).ReadCSR());
  std::unique_ptr<DevCSR> d(a->Convert<format::HIPCSR>(&gpu));
  const size_t n = a->get_dimensions()[0], m = a->get_dimensions()[1], nnz = a->get_num_nnz();
  EXPECT_TRUE(nnz > 2048);
  Plan from_host(a.get()), from_device(d.get());
  EXPECT_EQ((size_t)from_host.rows(), n);
  EXPECT_EQ((size_t)from_host.columns(), m);
  EXPECT_EQ((size_t)from_device.nnz(), nnz);
  // one plan, two value arrays: the plan holds none
  auto vals1 = SmallInts(nnz, 5), vals2 = SmallInts(nnz, 6);
  format::Array<float> vals1_host(nnz, vals1.data()), vals2_host(nnz, vals2.data());
  format::HIPArray<float> vals1_dev(nnz, dev.Upload(vals1.data(), nnz), gpu), vals2_dev(nnz, dev.Upload(vals2.data(), nnz), gpu);
  for (size_t k : KS) {
    auto x = SmallInts(n * k, 3 + (unsigned)k);
    const auto want1 = PlainLoop(a.get(), x.data(), k, vals1.data()), want2 = PlainLoop(a.get(), x.data(), k, vals2.data());
    const auto want_pattern = PlainLoop(a.get(), x.data(), k, nullptr);
    format::Array<float> x_host(n * k, x.data());
    format::HIPArray<float> x_dev(n * k, dev.Upload(x.data(), n * k), gpu);
    for (Plan *plan : {&from_host, &from_device}) {
      std::unique_ptr<format::Array<float>> y(kernels::SpMMTransposed(*plan, &x_host, k, &vals1_host));
      EXPECT_EQ(y->get_num_nnz(), m * k);
      EXPECT_TRUE(Same(y->get_vals(), want1, k));
      y.reset(kernels::SpMMTransposed(*plan, &x_host, k, &vals2_host));
      EXPECT_TRUE(Same(y->get_vals(), want2, k));
      y.reset(kernels::SpMMTransposed(*plan, &x_host, k));  // no values: a pattern
      EXPECT_TRUE(Same(y->get_vals(), want_pattern, k));
      std::unique_ptr<format::HIPArray<float>> yd(kernels::SpMMTransposed(*plan, &x_dev, k, &vals1_dev));
      EXPECT_EQ(yd->get_num_nnz(), m * k);
      std::unique_ptr<float[]> back(dev.Download(yd->get_vals(), m * k));
      EXPECT_TRUE(Same(back.get(), want1, k));
      yd.reset(kernels::SpMMTransposed(*plan, &x_dev, k, &vals2_dev));
      back.reset(dev.Download(yd->get_vals(), m * k));
      EXPECT_TRUE(Same(back.get(), want2, k));
      yd.reset(kernels::SpMMTransposed(*plan, &x_dev, k));
      back.reset(dev.Download(yd->get_vals(), m * k));
      EXPECT_TRUE(Same(back.get(), want_pattern, k));
    }
  }
}

TEST(Kernels, TransposePlanOfARectangle) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  // 3 x 4: an empty row, a duplicated entry (0, 2), row 0's columns unsorted
  int rp[] = {0, 3, 3, 5}, col[] = {2, 0, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, x[] = {1, 2, 10, 20, 100, 200};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  kernels::TransposePlan<int, int> plan(&a);
  std::unique_ptr<int[]> cp(dev.Download(plan.col_ptr(), 5)), row(dev.Download(plan.row(), 5)), perm(dev.Download(plan.perm(), 5));
  const int want_cp[] = {0, 1, 2, 4, 5}, want_row[] = {0, 2, 0, 0, 2}, want_perm[] = {1, 3, 0, 2, 4};
  for (int i = 0; i < 5; i++) EXPECT_TRUE(cp[i] == want_cp[i] && row[i] == want_row[i] && perm[i] == want_perm[i]);
  format::Array<float> x_host(6, x), vals_host(5, vals);
  std::unique_ptr<format::Array<float>> y(kernels::SpMMTransposed(plan, &x_host, 2, &vals_host));
  EXPECT_EQ(y->get_num_nnz(), 8u);
  const float want[] = {-1, -2, 300, 600, 6, 12, 500, 1000};
  for (int i = 0; i < 8; i++) EXPECT_TRUE(y->get_vals()[i] == want[i]);
  // 64-bit offsets over 32-bit ids, doubles, a pattern
  long long rp64[] = {0, 3, 3, 5};
  format::CSR<int, long long, int> b(3, 4, rp64, col, nullptr, format::kNotOwned, true);
  kernels::TransposePlan<int, long long> plan64(&b);
  double xd[] = {1, 2, 10, 20, 100, 200};
  format::Array<double> xd_host(6, xd);
  std::unique_ptr<format::Array<double>> yp(kernels::SpMMTransposed(plan64, &xd_host, 2));
  const double want_pattern[] = {1, 2, 100, 200, 2, 4, 100, 200};
  for (int i = 0; i < 8; i++) EXPECT_TRUE(yp->get_vals()[i] == want_pattern[i]);
  // k = 0: an empty product
  std::unique_ptr<format::Array<float>> none(kernels::SpMMTransposed(plan, &x_host, 0));
  EXPECT_EQ(none->get_num_nnz(), 0u);
}

TEST(Kernels, SpMMTransposedExceptions) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, x[] = {1, 2, 10, 20, 100, 200};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  std::unique_ptr<format::HIPCSR<int, int, float>> d(a.Convert<format::HIPCSR>(&gpu));
  kernels::TransposePlan<int, int> plan(d.get());
  // operand sizes, host and device: X below n * k values, a values array below nnz
  format::Array<float> x_host(6, x), short_x(5, x), short_vals(4, vals), vals_host(5, vals);
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &short_x, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &x_host, 3), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &x_host, 2, &short_vals), utils::TypeException);
  float *dx = dev.Upload(x, 6), *dv = dev.Upload(vals, 5);
  format::HIPArray<float> x_dev(6, dx, gpu, format::kNotOwned), x_dev_short(5, dx, gpu, format::kNotOwned);
  format::HIPArray<float> vals_dev(5, dv, gpu, format::kNotOwned), vals_dev_short(4, dv, gpu, format::kNotOwned);
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &x_dev_short, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &x_dev, 2, &vals_dev_short), utils::TypeException);
  EXPECT_NO_THROW(delete kernels::SpMMTransposed(plan, &x_dev, 2, &vals_dev));
  // device mismatch: an operand whose context names another device than the plan's
  format::HIPArray<float> x_elsewhere(6, dx, gpu, format::kNotOwned), vals_elsewhere(5, dv, gpu, format::kNotOwned);
  x_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  vals_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &x_elsewhere, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SpMMTransposed(plan, &x_dev, 2, &vals_elsewhere), utils::TypeException);
  // a column outside [0, m): the plan is refused by the library
  int bad_col[] = {0, 2, 4, 1, 3};
  format::CSR<int, int, float> bad(3, 4, rp, bad_col, vals, format::kNotOwned, true);
  EXPECT_THROW((kernels::TransposePlan<int, int>(&bad)), utils::HIPDeviceException);
  // the kernel function: a parameter that is no SpMMTransposedParams, an X of another type, values or a plan of another type
  DataMap data = {{"processed_format", &a}};
  std::any fp = x_host, pp, kp = SpMMTransposedParams{2, vals_host, {}}, not_params = 2;
  std::any wrong_x = format::Array<double>(0, nullptr);
  std::any wrong_vals = SpMMTransposedParams{2, format::Array<double>(0, nullptr), {}};
  long long rp64[] = {0, 3, 3, 5};
  format::CSR<int, long long, float> a64(3, 4, rp64, col, vals, format::kNotOwned, true);
  std::any wrong_plan = SpMMTransposedParams{2, {}, std::make_shared<kernels::TransposePlan<int, long long>>(&a64)};
  EXPECT_THROW((SpMMTransposed<int, int, float, float>(data, fp, pp, not_params)), utils::TypeException);
  EXPECT_THROW((SpMMTransposed<int, int, float, float>(data, wrong_x, pp, kp)), utils::TypeException);
  EXPECT_THROW((SpMMTransposed<int, int, float, float>(data, fp, pp, wrong_vals)), utils::TypeException);
  EXPECT_THROW((SpMMTransposed<int, int, float, float>(data, fp, pp, wrong_plan)), utils::TypeException);
  float *y = std::any_cast<float *>(SpMMTransposed<int, int, float, float>(data, fp, pp, kp));
  // columns: 0 <- 2 * row 0; 1 <- 3 * row 2; 2 <- (-1 + 4) * row 0; 3 <- 5 * row 2
  EXPECT_TRUE(y[0] == 2.0f && y[1] == 4.0f && y[2] == 300.0f && y[4] == 3.0f && y[7] == 1000.0f);
  delete[] y;
  dev.Free(dx);
  dev.Free(dv);
}

TEST(Experiment, SpMMTransposedWithPass) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {GRAPH_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(GRAPH_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0], nnz = a->get_num_nnz(), k = 3;
  auto x = SmallInts(n * k, 13), vals = SmallInts(nnz, 15);
  const auto want = PlainLoop(a.get(), x.data(), k, vals.data()), want_pattern = PlainLoop(a.get(), x.data(), k, nullptr);
  format::Array<float> x_host(n * k, x.data()), vals_host(nnz, vals.data());
  format::HIPArray<float> x_dev(n * k, dev.Upload(x.data(), n * k), gpu), vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);
  auto plan = std::make_shared<Plan>(a.get());  // Pass leaves the matrix as it is: one plan serves both experiments

  ConcreteExperiment staged, resident;
  staged.AddDataLoader(LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_host)});
  resident.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  for (auto *e : {&staged, &resident}) e->AddPreprocess("original", Pass, {});
  staged.AddKernel("spmm_t", SpMMTransposed<vertex_type, edge_type, value_type, float>, SpMMTransposedParams{k, vals_host, plan});
  resident.AddKernel("spmm_t", SpMMTransposed<vertex_type, edge_type, value_type, float>, SpMMTransposedParams{k, vals_dev, {}});
  for (auto *e : {&staged, &resident}) {
    e->AddKernel("pattern", SpMMTransposed<vertex_type, edge_type, value_type, float>, SpMMTransposedParams{k, {}, plan});
    e->Run(2, true);
    auto res = e->GetResults();
    EXPECT_EQ(res.size(), 4u);
    for (int i = 0; i < 2; i++) {
      float *y = std::any_cast<float *>(res["-" + GRAPH_NAME + ",original,spmm_t," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(y, want, k));
      delete[] y;
      y = std::any_cast<float *>(res["-" + GRAPH_NAME + ",original,pattern," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(y, want_pattern, k));
      delete[] y;
    }
    auto aux = e->GetAuxiliary();
    EXPECT_EQ(aux.size(), 2u);
    delete std::any_cast<format::Format *>(aux["format,-" + GRAPH_NAME]);
    EXPECT_TRUE(e->GetRunTimes()["-" + GRAPH_NAME + ",original,spmm_t,1"][0] > 0.0);
  }
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("Usage: test_spmm_t <path of a file to write> [filter]\n");
    return 2;
  }
  GRAPH_NAME = argv[1];
  WriteGraph(GRAPH_NAME);
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
