// kernels::RowSoftmax, kernels::RowSoftmaxBackward (kernels/row_softmax.h) and the experiment::RowSoftmax kernel function.
// Usage: test_row_softmax <path of a file to write> [filter]
//
// The program writes its own matrix to the path it is given: a structurally symmetric graph of SYM_N vertices (RCM takes
// it) with a hub row and more entries than one span of the device kernel, and a real value for every entry that is a
// function of its (row, column).  Host-staged against device-resident (the same bits) against a plain loop in long double
// (within the bounds of tests/softmax_restate.py), the own-values, explicit-values and pattern forms, every operand-size
// and device-mismatch exception, and experiment::RowSoftmax through ConcreteExperiment with Pass and with RCMReorder on
// the device, where the entries of P A P^T carry their values with them.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
using value_type = float;
typedef format::CSR<vertex_type, edge_type, value_type> HostCSR;
typedef format::HIPCSR<vertex_type, edge_type, value_type> DevCSR;

std::string SYM_NAME;  // argv[1]
constexpr unsigned SYM_N = 600;
constexpr long double EXP_ULPS = 3;  // EXP_ULPS of tests/softmax_restate.py (tests/test_row_softmax_hostlayer.py compares the two)
constexpr long double U32 = 5.9604644775390625e-8L;  // 2^-24

float ValueOf(unsigned i, unsigned j) { return (float)((int)((i * 31u + j * 17u) % 41u) - 20) * 0.37f; }

void WriteSymmetricGraph(const std::string &path) {
  std::set<std::pair<unsigned, unsigned>> e;
  for (unsigned i = 0; i < SYM_N; i++)
    for (unsigned j : {(i + 1) % SYM_N, (i * 7 + 3) % SYM_N, (i * i + 11) % SYM_N, 0u})  // (0: the hub)
      if (i != j) {
        e.insert({i, j});
        e.insert({j, i});
      }
  FILE *f = std::fopen(path.c_str(), "w");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate real general\n%u %u %zu\n", SYM_N, SYM_N, e.size());
  for (auto &p : e) std::fprintf(f, "%u %u %.9g\n", p.first + 1, p.second + 1, (double)ValueOf(p.first, p.second));
  std::fclose(f);
}

std::vector<float> Uniform(size_t count, unsigned seed, float scale) {  // in (-scale, scale)
  std::vector<float> v(count);
  for (auto &t : v) t = scale * ((float)((seed = seed * 1664525u + 1013904223u) >> 8) / 8388608.0f - 1.0f);
  return v;
}

// the forward in long double and, per entry, the bound |out - ref| <= B u ref + tiny of tests/softmax_restate.py
void PlainForward(HostCSR *a, const float *vals, std::vector<long double> &ref, std::vector<long double> &bound) {
  const vertex_type n = a->get_dimensions()[0];
  ref.assign(a->get_num_nnz(), 0);
  bound.assign(a->get_num_nnz(), 0);
  for (vertex_type i = 0; i < n; i++) {
    const edge_type lo = a->get_row_ptr()[i], hi = a->get_row_ptr()[i + 1];
    if (lo == hi) continue;
    long double m = vals ? vals[lo] : 0, least = m, sum = 0;
    for (edge_type p = lo; p < hi; p++) {
      m = std::fmax(m, vals ? (long double)vals[p] : 0);
      least = std::fmin(least, vals ? (long double)vals[p] : 0);
    }
    for (edge_type p = lo; p < hi; p++) sum += std::exp((vals ? (long double)vals[p] : 0) - m);
    const long double B = (long double)(hi - lo) + 4 * (std::fmin(m - least, -std::log((long double)FLT_TRUE_MIN)) + EXP_ULPS) + 16;
    for (edge_type p = lo; p < hi; p++) {
      ref[p] = std::exp((vals ? (long double)vals[p] : 0) - m) / sum;
      bound[p] = B * U32 * ref[p] + (long double)FLT_MIN;
    }
  }
}

// the backward in long double and the bound gamma(len + 4, u) |s| (|g| + sum |s g|), at float's u and at long double's
void PlainBackward(HostCSR *a, const float *s, const float *g, std::vector<long double> &ref, std::vector<long double> &bound) {
  const vertex_type n = a->get_dimensions()[0];
  ref.assign(a->get_num_nnz(), 0);
  bound.assign(a->get_num_nnz(), 0);
  for (vertex_type i = 0; i < n; i++) {
    const edge_type lo = a->get_row_ptr()[i], hi = a->get_row_ptr()[i + 1];
    long double d = 0, mag = 0;
    for (edge_type p = lo; p < hi; p++) {
      d += (long double)s[p] * g[p];
      mag += std::fabs((long double)s[p] * g[p]);
    }
    const long double k = (long double)(hi - lo) + 4;
    const long double gam = k * U32 / (1 - k * U32) + k * LDBL_EPSILON / (1 - k * LDBL_EPSILON);
    for (edge_type p = lo; p < hi; p++) {
      ref[p] = (long double)s[p] * ((long double)g[p] - d);
      bound[p] = gam * std::fabs((long double)s[p]) * (std::fabs((long double)g[p]) + mag);
    }
  }
}

bool Within(const float *got, const std::vector<long double> &ref, const std::vector<long double> &bound) {
  for (size_t p = 0; p < ref.size(); p++)
    if (!(std::fabs((long double)got[p] - ref[p]) <= bound[p])) {
      std::printf("  entry %zu: %.9g for %.12Lg, bound %.3Lg\n", p, (double)got[p], ref[p], bound[p]);
      return false;
    }
  return true;
}

bool SameBits(const float *a, const float *b, size_t count) {
  for (size_t p = 0; p < count; p++)
    if (std::memcmp(a + p, b + p, sizeof(float)) != 0) {
      std::printf("  entry %zu: %.9g and %.9g\n", p, (double)a[p], (double)b[p]);
      return false;
    }
  return true;
}

}  // namespace

TEST(Kernels, RowSoftmaxStagedAgainstResidentAgainstAPlainLoop) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  std::unique_ptr<DevCSR> d(a->Convert<format::HIPCSR>(&gpu));
  const size_t nnz = a->get_num_nnz();
  EXPECT_TRUE(nnz > 2048);
  EXPECT_TRUE(a->get_row_ptr()[1] - a->get_row_ptr()[0] == SYM_N - 1);  // the hub
  std::vector<long double> ref, bound;
  // the matrix's own values
  PlainForward(a.get(), a->get_vals(), ref, bound);
  std::unique_ptr<format::Array<float>> o(kernels::RowSoftmax(a.get()));
  EXPECT_EQ(o->get_num_nnz(), nnz);
  EXPECT_TRUE(Within(o->get_vals(), ref, bound));
  std::unique_ptr<format::HIPArray<float>> od(kernels::RowSoftmax(d.get()));
  EXPECT_EQ(od->get_num_nnz(), nnz);
  std::unique_ptr<float[]> back(dev.Download(od->get_vals(), nnz));
  EXPECT_TRUE(SameBits(back.get(), o->get_vals(), nnz));
  // a values array of the caller's
  auto vals = Uniform(nnz, 5, 9.0f);
  format::Array<float> vals_host(nnz, vals.data());
  format::HIPArray<float> vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);
  PlainForward(a.get(), vals.data(), ref, bound);
  o.reset(kernels::RowSoftmax(a.get(), &vals_host));
  EXPECT_TRUE(Within(o->get_vals(), ref, bound));
  od.reset(kernels::RowSoftmax(d.get(), &vals_dev));
  back.reset(dev.Download(od->get_vals(), nnz));
  EXPECT_TRUE(SameBits(back.get(), o->get_vals(), nnz));
  // the backward, s from the forward
  auto g = Uniform(nnz, 9, 1.0f);
  format::Array<float> g_host(nnz, g.data());
  format::HIPArray<float> g_dev(nnz, dev.Upload(g.data(), nnz), gpu);
  PlainBackward(a.get(), o->get_vals(), g.data(), ref, bound);
  std::unique_ptr<format::Array<float>> dz(kernels::RowSoftmaxBackward(a.get(), o.get(), &g_host));
  EXPECT_EQ(dz->get_num_nnz(), nnz);
  EXPECT_TRUE(Within(dz->get_vals(), ref, bound));
  std::unique_ptr<format::HIPArray<float>> dzd(kernels::RowSoftmaxBackward(d.get(), od.get(), &g_dev));
  back.reset(dev.Download(dzd->get_vals(), nnz));
  EXPECT_TRUE(SameBits(back.get(), dz->get_vals(), nnz));
}

TEST(Kernels, RowSoftmaxMaskAndPattern) {
  // 4 x 4 with its own float values, an empty row, a masked entry and a row of masked entries alone
  const float inf = INFINITY;
  int rp[] = {0, 3, 3, 5, 7}, col[] = {0, 2, 3, 1, 3, 0, 1};
  float vals[] = {1, -inf, 1, 3e38f, 3e38f, -inf, -inf};
  format::CSR<int, int, float> a(4, 4, rp, col, vals, format::kNotOwned, true);
  std::unique_ptr<format::Array<float>> o(kernels::RowSoftmax(&a));
  EXPECT_EQ(o->get_num_nnz(), 7u);
  const float want[] = {0.5f, 0.0f, 0.5f, 0.5f, 0.5f, 0.0f, 0.0f};
  for (int i = 0; i < 7; i++) EXPECT_TRUE(o->get_vals()[i] == want[i] && !std::signbit(o->get_vals()[i]));
  // integer values, float operands: a pattern, 1 / the entries of the row
  format::CSR<int, int, int> pattern(4, 4, rp, col, nullptr, format::kNotOwned, true);
  std::unique_ptr<format::Array<float>> op(kernels::RowSoftmax<int, int, int, float>(&pattern));
  const float want_pattern[] = {1.0f / 3, 1.0f / 3, 1.0f / 3, 0.5f, 0.5f, 0.5f, 0.5f};
  for (int i = 0; i < 7; i++) EXPECT_TRUE(op->get_vals()[i] == want_pattern[i]);
  // the backward on integers: d = 1 * 2 + 2 * 3 + 3 * 4 = 20 in row 0
  float s[] = {1, 2, 3, 1, 1, 2, 0}, g[] = {2, 3, 4, 5, 7, 1, 9};
  format::Array<float> s_host(7, s), g_host(7, g);
  std::unique_ptr<format::Array<float>> dz(kernels::RowSoftmaxBackward(&pattern, &s_host, &g_host));
  const float want_dz[] = {-18, -34, -48, -7, -5, -2, 0};
  for (int i = 0; i < 7; i++) EXPECT_TRUE(dz->get_vals()[i] == want_dz[i]);
}

TEST(Kernels, RowSoftmaxExceptions) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  int rp[] = {0, 3, 3, 5}, col[] = {0, 2, 2, 1, 3};
  float vals[] = {2, -1, 4, 3, 5}, g[] = {1, 2, 3, 4, 5};
  format::CSR<int, int, float> a(3, 4, rp, col, vals, format::kNotOwned, true);
  std::unique_ptr<format::HIPCSR<int, int, float>> d(a.Convert<format::HIPCSR>(&gpu));
  // operand sizes, host and device: an array below nnz values
  format::Array<float> v_host(5, vals), g_host(5, g), short_v(4, vals), short_g(4, g);
  EXPECT_THROW(delete kernels::RowSoftmax(&a, &short_v), utils::TypeException);
  EXPECT_THROW(delete kernels::RowSoftmaxBackward(&a, &short_v, &g_host), utils::TypeException);
  EXPECT_THROW(delete kernels::RowSoftmaxBackward(&a, &v_host, &short_g), utils::TypeException);
  EXPECT_NO_THROW(delete kernels::RowSoftmaxBackward(&a, &v_host, &g_host));
  float *dv = dev.Upload(vals, 5), *dg = dev.Upload(g, 5);
  format::HIPArray<float> v_dev(5, dv, gpu, format::kNotOwned), v_dev_short(4, dv, gpu, format::kNotOwned);
  format::HIPArray<float> g_dev(5, dg, gpu, format::kNotOwned), g_dev_short(4, dg, gpu, format::kNotOwned);
  EXPECT_THROW(delete kernels::RowSoftmax(d.get(), &v_dev_short), utils::TypeException);
  EXPECT_THROW(delete kernels::RowSoftmaxBackward(d.get(), &v_dev_short, &g_dev), utils::TypeException);
  EXPECT_THROW(delete kernels::RowSoftmaxBackward(d.get(), &v_dev, &g_dev_short), utils::TypeException);
  EXPECT_NO_THROW(delete kernels::RowSoftmax(d.get(), &v_dev));
  EXPECT_NO_THROW(delete kernels::RowSoftmaxBackward(d.get(), &v_dev, &g_dev));
  // device mismatch: an operand whose context names another device than the matrix's
  format::HIPArray<float> v_elsewhere(5, dv, gpu, format::kNotOwned), g_elsewhere(5, dg, gpu, format::kNotOwned);
  v_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  g_elsewhere.get_hip_context()->device_id = gpu.device_id + 1;
  EXPECT_THROW(delete kernels::RowSoftmax(d.get(), &v_elsewhere), utils::TypeException);
  EXPECT_THROW(delete kernels::RowSoftmaxBackward(d.get(), &v_elsewhere, &g_dev), utils::TypeException);
  EXPECT_THROW(delete kernels::RowSoftmaxBackward(d.get(), &v_dev, &g_elsewhere), utils::TypeException);
  // the kernel function: values of another type
  DataMap data = {{"processed_format", &a}};
  std::any fp, pp, kp = v_host, none, wrong = format::Array<double>(0, nullptr), not_an_array = 2;
  EXPECT_THROW((RowSoftmax<int, int, float, float>(data, fp, pp, wrong)), utils::TypeException);
  EXPECT_THROW((RowSoftmax<int, int, float, float>(data, fp, pp, not_an_array)), utils::TypeException);
  float *out = std::any_cast<float *>(RowSoftmax<int, int, float, float>(data, fp, pp, kp));
  float *own = std::any_cast<float *>(RowSoftmax<int, int, float, float>(data, fp, pp, none));
  EXPECT_TRUE(SameBits(out, own, 5) && std::fabs(out[0] + out[1] + out[2] - 1.0f) < 1e-6f && out[3] + out[4] > 0.999f);
  delete[] out;
  delete[] own;
  dev.Free(dv);
  dev.Free(dg);
}

TEST(Experiment, RowSoftmaxWithPass) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto &dev = hip::Device::Get(gpu.device_id);
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t nnz = a->get_num_nnz();
  auto vals = Uniform(nnz, 15, 9.0f);
  std::vector<long double> ref, bound, ref_own, bound_own;
  PlainForward(a.get(), vals.data(), ref, bound);
  PlainForward(a.get(), a->get_vals(), ref_own, bound_own);
  format::Array<float> vals_host(nnz, vals.data());
  format::HIPArray<float> vals_dev(nnz, dev.Upload(vals.data(), nnz), gpu);

  ConcreteExperiment staged, resident;
  staged.AddDataLoader(LoadCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, std::any())});
  resident.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, std::any())});
  for (auto *e : {&staged, &resident}) e->AddPreprocess("original", Pass, {});
  staged.AddKernel("softmax", RowSoftmax<vertex_type, edge_type, value_type, float>, vals_host);
  resident.AddKernel("softmax", RowSoftmax<vertex_type, edge_type, value_type, float>, vals_dev);
  for (auto *e : {&staged, &resident}) e->AddKernel("own", RowSoftmax<vertex_type, edge_type, value_type, float>, {});
  for (auto *e : {&staged, &resident}) {
    e->Run(2, true);
    auto res = e->GetResults();
    EXPECT_EQ(res.size(), 4u);
    for (int i = 0; i < 2; i++) {
      float *o = std::any_cast<float *>(res["-" + SYM_NAME + ",original,softmax," + std::to_string(i)][0]);
      EXPECT_TRUE(Within(o, ref, bound));
      delete[] o;
      o = std::any_cast<float *>(res["-" + SYM_NAME + ",original,own," + std::to_string(i)][0]);
      EXPECT_TRUE(Within(o, ref_own, bound_own));
      delete[] o;
    }
    auto aux = e->GetAuxiliary();
    EXPECT_EQ(aux.size(), 2u);
    delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
    EXPECT_TRUE(e->GetRunTimes()["-" + SYM_NAME + ",original,softmax,1"][0] > 0.0);
  }
}

TEST(Experiment, RowSoftmaxRcmPipelineOnTheDevice) {
  context::CPUContext cpu;
  context::HIPContext gpu(hip::DefaultDevice());
  std::vector<std::string> files = {SYM_NAME};
  std::unique_ptr<HostCSR> a(io::MTXReader<vertex_type, edge_type, value_type>(SYM_NAME).ReadCSR());
  const size_t n = a->get_dimensions()[0], nnz = a->get_num_nnz();
  EXPECT_EQ(n, (size_t)SYM_N);
  std::vector<long double> ref, bound;
  PlainForward(a.get(), a->get_vals(), ref, bound);

  ConcreteExperiment exp;
  exp.AddDataLoader(LoadHIPCSR<io::MTXReader, vertex_type, edge_type, value_type>, {std::make_pair(files, std::any())});
  reorder::RCMReorder<vertex_type, edge_type, value_type>::ParamsType params = {};
  exp.AddPreprocess("RCM", ReorderHIP<reorder::RCMReorder, vertex_type, edge_type, value_type>, params);
  exp.AddKernel("softmax", RowSoftmax<vertex_type, edge_type, value_type, float>, {});  // the permuted matrix's own values
  exp.Run(1, true);
  auto res = exp.GetResults();
  EXPECT_EQ(res.size(), 1u);
  float *got = std::any_cast<float *>(res["-" + SYM_NAME + ",RCM,softmax,0"][0]);
  auto aux = exp.GetAuxiliary();
  EXPECT_EQ(aux.size(), 2u);
  auto *permuted = std::any_cast<format::Format *>(aux["processed_format,-" + SYM_NAME + ",RCM"]);
  std::unique_ptr<HostCSR> b(permuted->AsAbsolute<DevCSR>()->Convert<format::CSR>(&cpu));
  EXPECT_EQ((size_t)b->get_num_nnz(), nnz);
  // a row of P A P^T holds the values of a row of A in another order: the same lengths, the softmax of its own values
  std::vector<unsigned> len_a(n), len_b(n);
  for (vertex_type i = 0; i < n; i++) {
    len_a[i] = a->get_row_ptr()[i + 1] - a->get_row_ptr()[i];
    len_b[i] = b->get_row_ptr()[i + 1] - b->get_row_ptr()[i];
  }
  std::multiset<unsigned> la(len_a.begin(), len_a.end()), lb(len_b.begin(), len_b.end());
  EXPECT_TRUE(la == lb);
  std::vector<long double> ref_b, bound_b;
  PlainForward(b.get(), b->get_vals(), ref_b, bound_b);
  EXPECT_TRUE(Within(got, ref_b, bound_b));
  // and the permuted matrix is the original one: every row of it holds the values of a row of A
  std::multiset<std::vector<float>> rows_a, rows_b;
  for (vertex_type i = 0; i < n; i++) {
    std::vector<float> ra(a->get_vals() + a->get_row_ptr()[i], a->get_vals() + a->get_row_ptr()[i + 1]);
    std::vector<float> rb(b->get_vals() + b->get_row_ptr()[i], b->get_vals() + b->get_row_ptr()[i + 1]);
    std::sort(ra.begin(), ra.end());
    std::sort(rb.begin(), rb.end());
    rows_a.insert(ra);
    rows_b.insert(rb);
  }
  EXPECT_TRUE(rows_a == rows_b);
  delete[] got;
  delete permuted;
  delete std::any_cast<format::Format *>(aux["format,-" + SYM_NAME]);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("Usage: test_row_softmax <path of a file to write> [filter]\n");
    return 2;
  }
  SYM_NAME = argv[1];
  WriteSymmetricGraph(SYM_NAME);
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
