// kernels::SDDMM (kernels/sddmm.h) and the experiment::SDDMM kernel function.  Usage: test_sddmm <path of a file to write> [filter]
//
// The program writes its own matrix to the path it is given: a structurally symmetric graph of SYM_N vertices (RCM takes
// it) of more entries than one span of the device kernel.  Values, U and V are small integers, so every dot is exact in
// float whatever its order and the comparisons are equalities: host-staged against device-resident against a plain loop
// for k = 1, 3, 64 and 130, every operand-size and device-mismatch exception, and experiment::SDDMM through
// ConcreteExperiment with Pass and with RCMReorder on the device, where the entries of P A P^T are compared with P U, P V.
#include <cstdint>
#include <cstdio>
#include <map>
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

// integer-valued floats: every dot below is exact in float, whatever its order
std::vector<float> SmallInts(size_t count, unsigned seed) {
  std::vector<float> v(count);
  for (auto &t : v) t = (float)((int)((seed = seed * 1664525u + 1013904223u) >> 24) % 17 - 8);
  return v;
}

std::vector<float> PlainLoop(HostCSR *a, const float *u, const float *x, size_t k, const float *vals) {
  const vertex_type n = a->get_dimensions()[0];
  std::vector<float> out(a->get_num_nnz(), 0.0f);
  for (vertex_type i = 0; i < n; i++)
    for (edge_type p = a->get_row_ptr()[i]; p < a->get_row_ptr()[i + 1]; p++) {
      float dot = 0.0f;
      for (size_t j = 0; j < k; j++) dot += u[(size_t)i * k + j] * x[(size_t)a->get_col()[p] * k + j];
      out[p] = vals ? vals[p] * dot : dot;
    }
  return out;
}

bool Same(const float *got, const std::vector<float> &want) {
  for (size_t p = 0; p < want.size(); p++)
    if (got[p] != want[p]) {
      std::printf("  entry %zu: %g for %g\n", p, (double)got[p], (double)want[p]);
      return false;
    }
  return true;
}

}  // namespace

TEST(Kernels, SDDMMStagedAgainstResidentAgainstAPlainLoop) {
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
    auto u = SmallInts(n * k, 7 + (unsigned)k), x = SmallInts(m * k, 3 + (unsigned)k);
    const auto want = PlainLoop(a.get(), u.data(), x.data(), k, vals.data());
    const auto want_pattern = PlainLoop(a.get(), u.data(), x.data(), k, nullptr);
    format::Array<float> u_host(n * k, u.data()), x_host(m * k, x.data());
    format::HIPArray<float> u_dev(n * k, dev.Upload(u.data(), n * k), gpu), x_dev(m * k, dev.Upload(x.data(), m * k), gpu);
    std::unique_ptr<format::Array<float>> o(kernels::SDDMM(a.get(), &u_host, &x_host, k, &vals_host));
    EXPECT_EQ(o->get_num_nnz(), nnz);
    EXPECT_TRUE(Same(o->get_vals(), want));
    o.reset(kernels::SDDMM(a.get(), &u_host, &x_host, k));  // unsigned values, float operands: a pattern
    EXPECT_TRUE(Same(o->get_vals(), want_pattern));
    std::unique_ptr<format::HIPArray<float>> od(kernels::SDDMM(d.get(), &u_dev, &x_dev, k, &vals_dev));
    EXPECT_EQ(od->get_num_nnz(), nnz);
    std::unique_ptr<float[]> back(dev.Download(od->get_vals(), nnz));
    EXPECT_TRUE(Same(back.get(), want));
    od.reset(kernels::SDDMM(d.get(), &u_dev, &x_dev, k));
    back.reset(dev.Download(od->get_vals(), nnz));
    EXPECT_TRUE(Same(back.get(), want_pattern));
  }
}

TEST(Kernels, SDDMMOwnValuesAndDoubles) {
  context::HIPContext gpu(hip::DefaultDevice());
  // 3 x 4 with its own float values, an empty row, a duplicate column; U is 3 x 2, V is 4 x 2
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, u[] = {1, 2, 7, 7, 3, -1}, x[] = {1, 2, 10, 20, 100, 200, 1000, 2000};
  float other[] = {1, 1, 1, 1, 1};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  format::Array<float> u_host(6, u), x_host(8, x), other_host(5, other);
  std::unique_ptr<format::Array<float>> o(kernels::SDDMM(&a, &u_host, &x_host, 2));
  EXPECT_EQ(o->get_num_nnz(), 5u);
  // dots: row 0 with columns 0, 2, 2: 5, 500, 500; row 2 with columns 1, 3: 10, 1000
  const float want[] = {10, -500, 2000, 30, 5000}, want_other[] = {5, 500, 500, 10, 1000};
  for (int i = 0; i < 5; i++) EXPECT_TRUE(o->get_vals()[i] == want[i]);
  o.reset(kernels::SDDMM(&a, &u_host, &x_host, 2, &other_host));
  for (int i = 0; i < 5; i++) EXPECT_TRUE(o->get_vals()[i] == want_other[i]);
  format::CSR<int, int, int> pattern(3, 4, rp, col, nullptr, format::kNotOwned, true);
  double ud[] = {1, 2, 7, 7, 3, -1}, xd[] = {1, 2, 10, 20, 100, 200, 1000, 2000};
  format::Array<double> ud_host(6, ud), xd_host(8, xd);
  std::unique_ptr<format::Array<double>> op(kernels::SDDMM(&pattern, &ud_host, &xd_host, 2));
  for (int i = 0; i < 5; i++) EXPECT_TRUE(op->get_vals()[i] == (double)want_other[i]);
  // k = 0: every entry is the empty sum
  std::unique_ptr<format::Array<float>> none(kernels::SDDMM(&a, &u_host, &x_host, 0));
  EXPECT_EQ(none->get_num_nnz(), 5u);
  for (int i = 0; i < 5; i++) EXPECT_TRUE(none->get_vals()[i] == 0.0f);
}

TEST(Kernels, SDDMMExceptions) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, u[] = {1, 2, 7, 7, 3, -1}, x[] = {1, 2, 10, 20, 100, 200, 1000, 2000};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  std::unique_ptr<format::HIPCSR<int, int, float>> d(a.Convert<format::HIPCSR>(&gpu));
  // operand sizes, host and device: U below n * k values, V below m * k, a values array below nnz
  format::Array<float> u_host(6, u), x_host(8, x), short_u(5, u), short_x(7, x), short_vals(4, vals);
  EXPECT_THROW(delete kernels::SDDMM(&a, &short_u, &x_host, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(&a, &u_host, &short_x, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(&a, &u_host, &x_host, 3), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(&a, &u_host, &x_host, 2, &short_vals), utils::TypeException);
  float *du = dev.Upload(u, 6), *dx = dev.Upload(x, 8), *dv = dev.Upload(vals, 5);
  format::HIPArray<float> u_dev(6, du, gpu, format::kNotOwned), u_dev_short(5, du, gpu, format::kNotOwned);
  format::HIPArray<float> x_dev(8, dx, gpu, format::kNotOwned), x_dev_short(7, dx, gpu, format::kNotOwned);
  format::HIPArray<float> vals_dev(5, dv, gpu, format::kNotOwned), vals_dev_short(4, dv, gpu, format::kNotOwned);
  EXPECT_THROW(delete kernels::SDDMM(d.get(), &u_dev_short, &x_dev, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(d.get(), &u_dev, &x_dev_short, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(d.get(), &u_dev, &x_dev, 2, &vals_dev_short), utils::TypeException);
  EXPECT_NO_THROW(delete kernels::SDDMM(d.get(), &u_dev, &x_dev, 2, &vals_dev));
  // device mismatch: an operand whose context names another device than the matrix's
  format::HIPArray<float> u_elsewhere(6, du, gpu, format::kNotOwned), x_elsewhere(8, dx, gpu, format::kNotOwned);
  format::HIPArray<float> vals_elsewhere(5, dv, gpu, format::kNotOwned);
  u_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  x_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  vals_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  EXPECT_THROW(delete kernels::SDDMM(d.get(), &u_elsewhere, &x_dev, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(d.get(), &u_dev, &x_elsewhere, 2), utils::TypeException);
  EXPECT_THROW(delete kernels::SDDMM(d.get(), &u_dev, &x_dev, 2, &vals_elsewhere), utils::TypeException);
  // the kernel function: a parameter that is no SDDMMParams, a V of another type, no U, a values array of another type
  DataMap data = {{"processed_format", &a}};
  std::any fp = x_host, pp, kp = SDDMMParams{2, u_host, {}}, not_params = 2, wrong_x = format::Array<double>(0, nullptr);
  std::any no_u = SDDMMParams{2, {}, {}}, wrong_u = SDDMMParams{2, format::Array<double>(0, nullptr), {}};
  std::any wrong_vals = SDDMMParams{2, u_host, format::Array<double>(0, nullptr)};
  EXPECT_THROW((SDDMM<int, int, float, float>(data, fp, pp, not_params)), utils::TypeException);
  EXPECT_THROW((SDDMM<int, int, float, float>(data, wrong_x, pp, kp)), utils::TypeException);
  EXPECT_THROW((SDDMM<int, int, float, float>(data, fp, pp, no_u)), utils::TypeException);
  EXPECT_THROW((SDDMM<int, int, float, float>(data, fp, pp, wrong_u)), utils::TypeException);
  EXPECT_THROW((SDDMM<int, int, float, float>(data, fp, pp, wrong_vals)), utils::TypeException);
  float *out = std::any_cast<float *>(SDDMM<int, int, float, float>(data, fp, pp, kp));
  EXPECT_TRUE(out[0] == 10.0f && out[1] == -500.0f && out[2] == 2000.0f && out[4] == 5000.0f);
  delete[] out;
  dev.Free(du);
  dev.Free(dx);
  dev.Free(dv);
}

TEST(Experiment, SDDMMWithPass) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0], m = a->get_dimensions()[1], nnz = a->get_num_nnz(), k = 3;
  auto u = SmallInts(n * k, 11), x = SmallInts(m * k, 13), vals = SmallInts(nnz, 15);
  const auto want = PlainLoop(a.get(), u.data(), x.data(), k, vals.data());
  const auto want_pattern = PlainLoop(a.get(), u.data(), x.data(), k, nullptr);
  format::Array<float> u_host(n * k, u.data()), x_host(m * k, x.data()), vals_host(nnz, vals.data());
  format::HIPArray<float> u_dev(n * k, dev.Upload(u.data(), n * k), gpu), x_dev(m * k, dev.Upload(x.data(), m * k), gpu);
  format::HIPArray<float> vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);

  ConcreteExperiment staged, resident;
  staged.AddDataLoader(LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_host)});
  resident.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  for (auto *e : {&staged, &resident}) e->AddPreprocess("original", Pass, {});
  staged.AddKernel("sddmm", SDDMM<vertex_type, edge_type, value_type, float>, SDDMMParams{k, u_host, vals_host});
  resident.AddKernel("sddmm", SDDMM<vertex_type, edge_type, value_type, float>, SDDMMParams{k, u_dev, vals_dev});
  staged.AddKernel("pattern", SDDMM<vertex_type, edge_type, value_type, float>, SDDMMParams{k, u_host, {}});
  resident.AddKernel("pattern", SDDMM<vertex_type, edge_type, value_type, float>, SDDMMParams{k, u_dev, {}});
  for (auto *e : {&staged, &resident}) {
    e->Run(2, true);
    auto res = e->GetResults();
    EXPECT_EQ(res.size(), 4u);
    for (int i = 0; i < 2; i++) {
      float *o = std::any_cast<float *>(res["-" + SYM_NAME + ",original,sddmm," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(o, want));
      delete[] o;
      o = std::any_cast<float *>(res["-" + SYM_NAME + ",original,pattern," + std::to_string(i)][0]);
      EXPECT_TRUE(Same(o, want_pattern));
      delete[] o;
    }
    auto aux = e->GetAuxiliary();
    EXPECT_EQ(aux.size(), 2u);
    delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
    EXPECT_TRUE(e->GetRunTimes()["-" + SYM_NAME + ",original,sddmm,1"][0] > 0.0);
  }
}

TEST(Experiment, SDDMMRcmPipelineOnTheDevice) {
  context::CPUContext cpu;
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0], nnz = a->get_num_nnz(), k = 64;
  EXPECT_EQ(n, (size_t)SYM_N);
  std::unique_ptr<vertex_type[]> order(bases::ReorderBase::Reorder<reorder::RCMReorder>({}, a.get(), {&cpu}, true));
  // U' = P U and V' = P V are what the kernel gets; entry (order[i], order[j]) of P A P^T carries U[i] . V[j]
  auto up = SmallInts(n * k, 19), xp = SmallInts(n * k, 23);
  std::vector<float> u(n * k), x(n * k);
  for (size_t r = 0; r < n; r++)
    for (size_t j = 0; j < k; j++) {
      u[r * k + j] = up[(size_t)order[r] * k + j];
      x[r * k + j] = xp[(size_t)order[r] * k + j];
    }
  const auto dots = PlainLoop(a.get(), u.data(), x.data(), k, nullptr);
  std::map<std::pair<vertex_type, vertex_type>, float> want;  // by the permuted (row, column): the graph has no duplicates
  for (vertex_type i = 0; i < n; i++)
    for (edge_type p = a->get_row_ptr()[i]; p < a->get_row_ptr()[i + 1]; p++)
      want[{order[i], order[a->get_col()[p]]}] = dots[p];
  EXPECT_EQ(want.size(), nnz);
  format::HIPArray<float> u_dev(n * k, dev.Upload(up.data(), n * k), gpu), x_dev(n * k, dev.Upload(xp.data(), n * k), gpu);

  ConcreteExperiment exp;
  exp.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, x_dev)});
  reorder::RCMReorder<vertex_type, edge_type, value_type>::ParamsType params = {};
  exp.AddPreprocess("RCM", ReorderHIP<reorder::RCMReorder, vertex_type, edge_type, value_type>, params);
  exp.AddKernel("sddmm", SDDMM<vertex_type, edge_type, value_type, float>, SDDMMParams{k, u_dev, {}});
  exp.Run(1, true);
  auto res = exp.GetResults();
  EXPECT_EQ(res.size(), 1u);
  float *got = std::any_cast<float *>(res["-" + SYM_NAME + ",RCM,sddmm,0"][0]);
  auto aux = exp.GetAuxiliary();
  EXPECT_EQ(aux.size(), 2u);
  auto *permuted = std::any_cast<format::Format *>(aux["processed_format,-" + SYM_NAME + ",RCM"]);
  std::unique_ptr<HostCSR> b(permuted->AsAbsolute<DevCSR>()->Convert<format::CSR>(&cpu));
  EXPECT_EQ((size_t)b->get_num_nnz(), nnz);
  size_t wrong = 0;
  for (vertex_type i = 0; i < n; i++)
    for (edge_type p = b->get_row_ptr()[i]; p < b->get_row_ptr()[i + 1]; p++) {
      auto it = want.find({i, b->get_col()[p]});
      if (it == want.end() || it->second != got[p]) wrong++;
    }
  EXPECT_EQ(wrong, 0u);
  delete[] got;
  delete permuted;
  delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("Usage: test_sddmm <path of a file to write> [filter]\n");
    return 2;
  }
  SYM_NAME = argv[1];
  WriteSymmetricGraph(SYM_NAME);
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
