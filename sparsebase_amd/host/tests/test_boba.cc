// Host-layer tests of reorder::BOBAReorder: the reference's 3-vertex graph through ReorderBase::Reorder on COO, HIPCOO
// and CSR (through the converter), GetReorderDevice on square and rectangular input (max(n, m) entries on every
// path), the three index tuples, and a refused id.  Expected orders are the closed form of include/sbx.h, which
// tests/test_boba_host.py checks against the real reference (tests/golden/boba_heatmap.npz).
// Needs a GPU (the {COO} implementation stages the arrays through the default device).
#include <cstdint>
#include <memory>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

// functionality_common.inc: rows {0, 0, 1, 2}, cols {1, 2, 0, 0}; rows 1 and 2 start at column 0, row 0 at column 1
static const int rows3[4] = {0, 0, 1, 2}, cols3[4] = {1, 2, 0, 0}, rp3[4] = {0, 2, 3, 4};
static const int want3[3] = {2, 0, 1};

template <typename I, typename N, typename V>
static void reference_case() {
  std::vector<I> r(rows3, rows3 + 4), c(cols3, cols3 + 4);
  std::vector<N> rp(rp3, rp3 + 4);
  format::COO<I, N, V> coo(3, 3, 4, r.data(), c.data(), nullptr, format::kNotOwned);
  for (bool seq : {true, false}) {
    reorder::BOBAReorder<I, N, V> boba(seq);
    I *o = boba.GetReorder(&coo, {&cpu_context}, false);
    for (int i = 0; i < 3; i++) EXPECT_EQ((int)o[i], want3[i]);
    delete[] o;
    I *o2 = bases::ReorderBase::Reorder<reorder::BOBAReorder>({seq}, &coo, {&cpu_context}, true);
    for (int i = 0; i < 3; i++) EXPECT_EQ((int)o2[i], want3[i]);
    delete[] o2;
  }
  // device-resident input: the {HIPCOO} implementation, and the order left on the device
  std::unique_ptr<format::HIPCOO<I, N, V>> dcoo(coo.template Convert<format::HIPCOO>(hip_context.get()));
  reorder::BOBAReorder<I, N, V> boba(true);
  I *od = boba.GetReorder(dcoo.get(), {hip_context.get()}, false);
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)od[i], want3[i]);
  delete[] od;
  std::unique_ptr<format::HIPArray<I>> d(
      bases::ReorderBase::Reorder<reorder::BOBAReorder>({true}, dcoo.get(), *hip_context));
  EXPECT_EQ((int)d->get_dimensions()[0], 3);
  std::unique_ptr<format::Array<I>> back(d->template Convert<format::Array>(&cpu_context));
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)back->get_vals()[i], want3[i]);
  // a CSR reaches it through the converter (CSR -> COO), as in the reference
  format::CSR<I, N, V> csr(3, 3, rp.data(), c.data(), nullptr, format::kNotOwned);
  I *oc = bases::ReorderBase::Reorder<reorder::BOBAReorder>({false}, &csr, {&cpu_context}, true);
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)oc[i], want3[i]);
  delete[] oc;
  bool threw = false;  // no direct implementation for a CSR
  try {
    delete[] boba.GetReorder(&csr, {&cpu_context}, false);
  } catch (const std::exception &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

TEST(BOBA, ReferenceGraphInt) { reference_case<int, int, int>(); }
TEST(BOBA, ReferenceGraphInt64Double) { reference_case<int64_t, int64_t, double>(); }
TEST(BOBA, ReferenceGraphMixedWidth) { reference_case<int, long long, float>(); }

TEST(BOBA, RectangularGivesMaxNM) {
  // 3 x 6: rows {0, 2}, columns up to 5; nodes = 6.  Group 1: row 2 (mincol 1), row 0 (mincol 4);
  // group 2: columns 1, 4, 5 that are no row; group 3: 3 (no entry at all)
  std::vector<int> r{0, 2, 0, 2}, c{4, 1, 5, 2};
  format::COO<int, int, int> coo(3, 6, 4, r.data(), c.data(), nullptr, format::kNotOwned);
  const int want[6] = {1, 2, 0, 5, 3, 4};  // order: 2, 0, 1, 4, 5, 3 -> 2 gets 0, 0 gets 1, 1 gets 2, 4 gets 3, ...
  reorder::BOBAReorder<int, int, int> boba(true);
  int *o = boba.GetReorder(&coo, {&cpu_context}, true);
  for (int i = 0; i < 6; i++) EXPECT_EQ(o[i], want[i]);
  delete[] o;
  // host input through GetReorderDevice: max(n, m) entries uploaded, not dims[0]
  std::unique_ptr<format::HIPArray<int>> d(boba.GetReorderDevice(&coo, hip_context.get(), true));
  EXPECT_EQ((int)d->get_dimensions()[0], 6);
  std::unique_ptr<format::Array<int>> back(d->template Convert<format::Array>(&cpu_context));
  for (int i = 0; i < 6; i++) EXPECT_EQ(back->get_vals()[i], want[i]);
  std::unique_ptr<format::HIPCOO<int, int, int>> dcoo(coo.Convert<format::HIPCOO>(hip_context.get()));
  std::unique_ptr<format::HIPArray<int>> d2(boba.GetReorderDevice(dcoo.get(), hip_context.get(), true));
  EXPECT_EQ((int)d2->get_dimensions()[0], 6);
  std::unique_ptr<format::Array<int>> back2(d2->template Convert<format::Array>(&cpu_context));
  for (int i = 0; i < 6; i++) EXPECT_EQ(back2->get_vals()[i], want[i]);
}

TEST(BOBA, OutOfRangeIdThrows) {
  std::vector<int> r{0, 3}, c{1, 1};
  format::COO<int, int, int> coo(3, 3, 2, r.data(), c.data(), nullptr, format::kNotOwned, true);
  reorder::BOBAReorder<int, int, int> boba(false);
  bool threw = false;
  try {
    delete[] boba.GetReorder(&coo, {&cpu_context}, true);
  } catch (const std::exception &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_boba needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
