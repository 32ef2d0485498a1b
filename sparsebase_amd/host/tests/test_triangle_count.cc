// Host-layer tests of feature::TriangleCount: the reference's own test (feature/triangle_count_tests.cc) on its two
// graphs, walked through every entry of the interface, the device-resident key, a COO input, an <int64_t, int64_t,
// void> instantiation, and the graphs where the reference's value is not the number of triangles.
// Needs a GPU (the {CSR} implementation stages the arrays through the default device).
#include <cstdint>
#include <memory>
#include <typeindex>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

// triangle_count_tests.cc: DirectedTriangleTests (answer 4) and UndirectedTriangleTests (answer 2), n = 10
static int dir_rp[11] = {0, 0, 1, 2, 3, 4, 5, 6, 8, 10, 12}, dir_col[12] = {2, 3, 1, 6, 4, 5, 8, 9, 7, 9, 7, 8};
static int und_rp[11] = {0, 0, 2, 4, 6, 8, 10, 12, 13, 15, 16},
           und_col[16] = {2, 3, 1, 3, 1, 2, 5, 6, 4, 6, 4, 5, 8, 7, 9, 8};

template <typename I, typename N>
static void reference_flow(int n, const int *rp, const int *col, bool directed, int64_t ans) {
  const int nnz = rp[n];
  std::vector<N> r(rp, rp + n + 1);
  std::vector<I> c(col, col + nnz);
  format::CSR<I, N, void> csr(n, n, r.data(), c.data(), nullptr, format::kNotOwned);
  feature::TriangleCountParams p(directed);
  feature::TriangleCount<I, N, void> feature(p);
  EXPECT_EQ(feature.get_sub_ids().size(), (size_t)1);
  EXPECT_TRUE(feature.get_sub_ids()[0] == std::type_index(typeid(feature)));
  auto subs = feature.get_subs();
  EXPECT_EQ(subs.size(), (size_t)1);
  EXPECT_TRUE(std::type_index(typeid(*subs[0])) == std::type_index(typeid(feature)));
  EXPECT_NE(subs[0], (utils::Extractable *)&feature);
  delete subs[0];
  int64_t *t = feature::TriangleCount<I, N, void>::GetTriangleCountCSR({&csr}, &p);
  EXPECT_EQ(*t, ans);
  delete t;
  for (bool convert : {true, false, true}) {
    t = feature.GetTriangleCount(&csr, {&cpu_context}, convert);
    EXPECT_EQ(*t, ans);
    delete t;
  }
  auto cached = feature.GetTriangleCountCached(&csr, {&cpu_context}, true);
  EXPECT_EQ(*std::get<1>(cached), ans);
  delete std::get<1>(cached);
  auto fmap = feature.Extract(&csr, {&cpu_context}, true);
  EXPECT_EQ(fmap.size(), (size_t)1);
  for (auto &kv : fmap) EXPECT_TRUE(kv.first == std::type_index(typeid(feature)));
  int64_t *e = std::any_cast<int64_t *>(fmap[feature.get_id()]);
  EXPECT_EQ(*e, ans);
  delete e;
  // device-resident input: the {HIPCSR} implementation, nothing staged
  auto *dcsr = csr.template Convert<format::HIPCSR>(hip_context.get());
  EXPECT_TRUE(dcsr->get_id() == (format::HIPCSR<I, N, void>::get_id_static()));
  t = feature.GetTriangleCount(dcsr, {hip_context.get()}, false);
  EXPECT_EQ(*t, ans);
  delete t;
  delete dcsr;
}

TEST(TriangleCount, ReferenceDirected) { reference_flow<int, int>(10, dir_rp, dir_col, true, 4); }
TEST(TriangleCount, ReferenceUndirected) { reference_flow<int, int>(10, und_rp, und_col, false, 2); }
TEST(TriangleCount, Int64Directed) { reference_flow<int64_t, int64_t>(10, dir_rp, dir_col, true, 4); }
TEST(TriangleCount, Int64Undirected) { reference_flow<int64_t, int64_t>(10, und_rp, und_col, false, 2); }
TEST(TriangleCount, MixedWidthUndirected) { reference_flow<int, int64_t>(10, und_rp, und_col, false, 2); }

TEST(TriangleCount, DefaultParamsAreUndirected) {
  format::CSR<int, int, void> csr(10, 10, und_rp, und_col, nullptr, format::kNotOwned);
  feature::TriangleCount<int, int, void> feature;
  int64_t *t = feature.GetTriangleCount(&csr, {&cpu_context}, true);
  EXPECT_EQ(*t, 2);
  delete t;
  auto shared = std::make_shared<feature::TriangleCountParams>(true);
  format::CSR<int, int, void> dcsr(10, 10, dir_rp, dir_col, nullptr, format::kNotOwned);
  feature::TriangleCount<int, int, void> directed(shared);
  t = directed.GetTriangleCount(&dcsr, {&cpu_context}, true);
  EXPECT_EQ(*t, 4);
  delete t;
}

TEST(TriangleCount, CooNeedsConversion) {
  // the undirected graph as a COO: no {COO} implementation, so it runs after conversion only
  std::vector<int> row, col(und_col, und_col + 16);
  for (int i = 0; i < 10; i++)
    for (int j = und_rp[i]; j < und_rp[i + 1]; j++) row.push_back(i);
  format::COO<int, int, void> coo(10, 10, 16, row.data(), col.data(), nullptr, format::kNotOwned);
  feature::TriangleCount<int, int, void> feature;
  EXPECT_THROW(feature.GetTriangleCount(&coo, {&cpu_context}, false),
               utils::DirectExecutionNotAvailableException<std::vector<std::type_index>>);
  int64_t *t = feature.GetTriangleCount(&coo, {&cpu_context}, true);
  EXPECT_EQ(*t, 2);
  delete t;
}

TEST(TriangleCount, ReferenceValueIsNotATriangleCount) {
  // 4-cycle 1-2-3-4 with vertex 0 isolated: 1; triangle 0-1-2: 0; directed cycle 0 -> 1 -> 2 -> 0: 0 (include/sbx.h)
  int c4_rp[6] = {0, 0, 2, 4, 6, 8}, c4_col[8] = {2, 4, 1, 3, 2, 4, 3, 1};
  int k3_rp[4] = {0, 2, 4, 6}, k3_col[6] = {1, 2, 0, 2, 0, 1};
  int d3_rp[4] = {0, 1, 2, 3}, d3_col[3] = {1, 2, 0};
  format::CSR<int, int, void> c4(5, 5, c4_rp, c4_col, nullptr, format::kNotOwned);
  format::CSR<int, int, void> k3(3, 3, k3_rp, k3_col, nullptr, format::kNotOwned);
  format::CSR<int, int, void> d3(3, 3, d3_rp, d3_col, nullptr, format::kNotOwned);
  feature::TriangleCount<int, int, void> und(feature::TriangleCountParams(false)), dir(feature::TriangleCountParams(true));
  int64_t *t = und.GetTriangleCount(&c4, {&cpu_context}, true);
  EXPECT_EQ(*t, 1);
  delete t;
  t = und.GetTriangleCount(&k3, {&cpu_context}, true);
  EXPECT_EQ(*t, 0);
  delete t;
  t = dir.GetTriangleCount(&d3, {&cpu_context}, true);
  EXPECT_EQ(*t, 0);
  delete t;
}

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_triangle_count needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
