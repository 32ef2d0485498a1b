// Host-layer tests of reorder::SlashburnReorder: the reference's three SlashburnReorderTest cases
// (reorder/slashburn_reorder_tests.cc) on its 3-vertex graph, the device-resident key, ReorderBase::Reorder both ways,
// every index tuple, and a graph on which the flags change the result.  Expected orders are the real reference's
// (tests/golden/slashburn.npz) and the restatement's (tests/test_slashburn_host.py).
// Needs a GPU (the {CSR} implementation stages the arrays through the default device).
#include <cstdint>
#include <memory>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

// functionality_common.inc: n = 3, rows {0: 1 2, 1: 0, 2: 0}
static int rp3[4] = {0, 2, 3, 4}, col3[4] = {1, 2, 0, 0};

template <typename I>
static bool is_permutation(const I *inv, int n) {
  std::vector<int> seen(n, 0);
  for (int i = 0; i < n; i++) {
    if (inv[i] < 0 || inv[i] >= n || seen[inv[i]]) return false;
    seen[inv[i]] = 1;
  }
  return true;
}

template <typename I, typename N>
static void reference_case(int k, bool greedy, bool hub_order, std::vector<int> want) {
  std::vector<N> r(rp3, rp3 + 4);
  std::vector<I> c(col3, col3 + 4);
  std::vector<int> vals(4, 1);
  format::CSR<I, N, int> csr(3, 3, r.data(), c.data(), vals.data(), format::kNotOwned);
  reorder::SlashburnReorder<I, N, int> sb(k, greedy, hub_order);
  for (bool convert : {true, false}) {
    I *order = sb.GetReorder(&csr, {&cpu_context}, convert);
    EXPECT_TRUE(is_permutation(order, 3));
    for (int i = 0; i < 3; i++) EXPECT_EQ((int)order[i], want[i]);
    delete[] order;
  }
  // params struct and ReorderBase, host array
  I *o = bases::ReorderBase::Reorder<reorder::SlashburnReorder>({k, greedy, hub_order}, &csr, {&cpu_context}, true);
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)o[i], want[i]);
  delete[] o;
  // device-resident input: the {HIPCSR} implementation, and the order left on the device
  std::unique_ptr<format::HIPCSR<I, N, int>> dcsr(csr.template Convert<format::HIPCSR>(hip_context.get()));
  I *od = sb.GetReorder(dcsr.get(), {hip_context.get()}, false);
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)od[i], want[i]);
  delete[] od;
  std::unique_ptr<format::HIPArray<I>> d(
      bases::ReorderBase::Reorder<reorder::SlashburnReorder>({k, greedy, hub_order}, dcsr.get(), *hip_context));
  std::unique_ptr<format::Array<I>> back(d->template Convert<format::Array>(&cpu_context));
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)back->get_vals()[i], want[i]);
  // a host CSR through the device overload: staged, then the same order
  std::unique_ptr<format::HIPArray<I>> d2(
      bases::ReorderBase::Reorder<reorder::SlashburnReorder>({k, greedy, hub_order}, &csr, *hip_context));
  std::unique_ptr<format::Array<I>> back2(d2->template Convert<format::Array>(&cpu_context));
  for (int i = 0; i < 3; i++) EXPECT_EQ((int)back2->get_vals()[i], want[i]);
}

// slashburn_reorder_tests.cc: BasicTest (k = 1), BasicTestMultiK (k = 10), BasicTestGreedyHub (k = 1, greedy, hub order)
TEST(Slashburn, BasicTest) { reference_case<int, int>(1, false, false, {0, 1, 2}); }
TEST(Slashburn, BasicTestMultiK) { reference_case<int, int>(10, false, false, {2, 1, 0}); }
TEST(Slashburn, BasicTestGreedyHub) { reference_case<int, int>(1, true, true, {0, 1, 2}); }
TEST(Slashburn, Int64) { reference_case<int64_t, int64_t>(1, true, false, {0, 1, 2}); }
TEST(Slashburn, MixedWidth) { reference_case<int, int64_t>(10, false, true, {2, 1, 0}); }

TEST(Slashburn, FlagsAreHeldPerCall) {
  // hubs 0, 1 and 7 with spokes: a greedy call between two default calls leaves the second one alone
  // (rows 6 and 7: 6 -> 7, 7 -> 0, 1; 7 is a third hub of degree 3 in S)
  std::vector<int> rp{0, 3, 6, 7, 8, 9, 10, 11, 13}, col{2, 3, 7, 4, 5, 7, 0, 0, 1, 1, 7, 0, 1};
  format::CSR<int, int, int> csr(8, 8, rp.data(), col.data(), nullptr, format::kNotOwned);
  reorder::SlashburnReorder<int, int, int> plain(1, false, false), greedy(1, true, false);
  int *a = plain.GetReorder(&csr, {&cpu_context}, true);
  int *g = greedy.GetReorder(&csr, {&cpu_context}, true);
  int *b = plain.GetReorder(&csr, {&cpu_context}, true);
  EXPECT_TRUE(is_permutation(a, 8));
  EXPECT_TRUE(is_permutation(g, 8));
  for (int i = 0; i < 8; i++) EXPECT_EQ(a[i], b[i]);
  delete[] a;
  delete[] g;
  delete[] b;
}

TEST(Slashburn, BadArgumentsThrow) {
  format::CSR<int, int, int> csr(3, 3, rp3, col3, nullptr, format::kNotOwned);
  reorder::SlashburnReorder<int, int, int> zero(0, false, false);
  bool threw = false;
  try {
    delete[] zero.GetReorder(&csr, {&cpu_context}, true);
  } catch (const std::exception &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_slashburn needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
