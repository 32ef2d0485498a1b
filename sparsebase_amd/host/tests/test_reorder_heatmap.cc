// Host-layer tests of reorder::ReorderHeatmap and ReorderBase::Heatmap: the reference's two 3 x 3 known answers
// (reorder_heatmap_tests.cc, reorder_base_tests.cc; functionality_common.inc) with host arrays, device arrays and a
// COO through the converter, the three index tuples, double output, and the ReorderException cases.
// Needs a GPU (the {CSR, Array, Array} implementation stages the arrays through the default device).
#include <cstdint>
#include <memory>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

static const int rp3[4] = {0, 2, 3, 4}, cols3[4] = {1, 2, 0, 0}, rows3[4] = {0, 0, 1, 2};
static const float no_order_true[9] = {0, 0.25, 0.25, 0.25, 0, 0, 0.25, 0, 0};
static const int r_reorder[3] = {1, 2, 0}, c_reorder[3] = {2, 0, 1}, identity[3] = {0, 1, 2};
static const float rc_order_true[9] = {0, 0, 0.25, 0.25, 0.25, 0, 0, 0, 0.25};

template <typename I, typename N, typename V, typename F>
static void known_answers() {
  std::vector<N> rp(rp3, rp3 + 4);
  std::vector<I> c(cols3, cols3 + 4), r(rows3, rows3 + 4), id(identity, identity + 3), ro(r_reorder, r_reorder + 3),
      co(c_reorder, c_reorder + 3);
  format::CSR<I, N, V> csr(3, 3, rp.data(), c.data(), nullptr, format::kNotOwned);
  format::COO<I, N, V> coo(3, 3, 4, r.data(), c.data(), nullptr, format::kNotOwned);
  format::Array<I> a_id(3, id.data(), format::kNotOwned), a_r(3, ro.data(), format::kNotOwned),
      a_c(3, co.data(), format::kNotOwned);
  reorder::ReorderHeatmap<I, N, V, F> heatmapper(3);
  std::unique_ptr<format::FormatOrderOne<F>> h(heatmapper.Get(&csr, &a_id, &a_id, {&cpu_context}, false));
  for (int i = 0; i < 9; i++) EXPECT_EQ(h->template As<format::Array>()->get_vals()[i], (F)no_order_true[i]);
  std::unique_ptr<format::FormatOrderOne<F>> h2(heatmapper.Get(&csr, &a_r, &a_c, {&cpu_context}, true));
  for (int i = 0; i < 9; i++) EXPECT_EQ(h2->template As<format::Array>()->get_vals()[i], (F)rc_order_true[i]);
  // device arrays with a COO (reference tests' USE_CUDA branch): the converter makes an HIPCSR
  std::unique_ptr<format::HIPArray<I>> d_r(a_r.template Convert<format::HIPArray>(hip_context.get()));
  std::unique_ptr<format::HIPArray<I>> d_c(a_c.template Convert<format::HIPArray>(hip_context.get()));
  std::unique_ptr<format::FormatOrderOne<F>> h3(
      heatmapper.Get(&coo, d_r.get(), d_c.get(), {&cpu_context, hip_context.get()}, true));
  for (int i = 0; i < 9; i++) EXPECT_EQ(h3->template As<format::Array>()->get_vals()[i], (F)rc_order_true[i]);
  // fully device-resident: the {HIPCSR, HIPArray, HIPArray} implementation
  std::unique_ptr<format::HIPCSR<I, N, V>> dcsr(csr.template Convert<format::HIPCSR>(hip_context.get()));
  std::unique_ptr<format::FormatOrderOne<F>> h4(heatmapper.Get(dcsr.get(), d_r.get(), d_c.get(), {hip_context.get()}, false));
  for (int i = 0; i < 9; i++) EXPECT_EQ(h4->template As<format::Array>()->get_vals()[i], (F)rc_order_true[i]);
  // ReorderBase::Heatmap, host and device arrays
  std::unique_ptr<format::Array<F>> b1(bases::ReorderBase::Heatmap<F>(&csr, &a_id, &a_id, 3, {&cpu_context}, true));
  for (int i = 0; i < 9; i++) EXPECT_EQ(b1->get_vals()[i], (F)no_order_true[i]);
  std::unique_ptr<format::Array<F>> b2(
      bases::ReorderBase::Heatmap<F>(&coo, d_r.get(), d_c.get(), 3, {&cpu_context, hip_context.get()}, true));
  for (int i = 0; i < 9; i++) EXPECT_EQ(b2->get_vals()[i], (F)rc_order_true[i]);
  // the default constructor: num_parts = 3
  reorder::ReorderHeatmap<I, N, V, F> dflt;
  std::unique_ptr<format::FormatOrderOne<F>> h5(dflt.Get(&csr, &a_r, &a_c, {&cpu_context}, true));
  for (int i = 0; i < 9; i++) EXPECT_EQ(h5->template As<format::Array>()->get_vals()[i], (F)rc_order_true[i]);
}

TEST(ReorderHeatmap, KnownAnswersInt) { known_answers<int, int, int, float>(); }
TEST(ReorderHeatmap, KnownAnswersInt64Double) { known_answers<int64_t, int64_t, double, double>(); }
TEST(ReorderHeatmap, KnownAnswersMixedWidth) { known_answers<int, long long, float, float>(); }

TEST(ReorderHeatmap, NumPartsOutOfRangeThrows) {
  format::CSR<int, int, int> csr(3, 3, const_cast<int *>(rp3), const_cast<int *>(cols3), nullptr, format::kNotOwned);
  format::Array<int> a_id(3, const_cast<int *>(identity), format::kNotOwned);
  for (int b : {0, -1, 4}) {
    reorder::ReorderHeatmap<int, int, int, float> hm(b);
    bool threw = false;
    try {
      delete hm.Get(&csr, &a_id, &a_id, {&cpu_context}, true);
    } catch (const utils::ReorderException &e) {
      threw = std::string(e.what()) ==
              "Cannot generate heatmap for matrix when num_parts > number of rows or columns";
    }
    EXPECT_TRUE(threw);
  }
  bool threw = false;
  try {
    delete bases::ReorderBase::Heatmap<float>(&csr, &a_id, &a_id, 5, {&cpu_context}, true);
  } catch (const utils::ReorderException &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_reorder_heatmap needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
