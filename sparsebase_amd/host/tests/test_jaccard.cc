// Host-layer tests of feature::JaccardWeights: the reference's own test (feature/jaccard_weights_tests.cc on the
// matrix of functionality_common.inc:6-12) and a worked example whose weights are known exactly.
// Needs a GPU (the conversion search of the dispatch opens the device even when no HIP context is offered).
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;
typedef format::CSR<int, int, int> CSR3;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, sizeof(b));
  return b;
}

TEST(Jaccard, NoHipContext) {  // jaccard_weights_tests.cc: NoCuda, and the last case of Jaccard
  int row_ptr[4] = {0, 2, 3, 4}, cols[4] = {1, 2, 0, 0};
  CSR3 csr(3, 3, row_ptr, cols, nullptr, format::kNotOwned);
  feature::JaccardWeights<int, int, int, float> jac;
  EXPECT_THROW(jac.GetJaccardWeights(&csr, {&cpu_context}, true), utils::FunctionNotFoundException);
  EXPECT_THROW(jac.GetJaccardWeights(&csr, {&cpu_context}, false), utils::FunctionNotFoundException);
}

TEST(Jaccard, ReferenceCase) {  // jaccard_weights_tests.cc: Jaccard
  int row_ptr[4] = {0, 2, 3, 4}, cols[4] = {1, 2, 0, 0}, vals[4] = {1, 2, 3, 4};
  CSR3 csr(3, 3, row_ptr, cols, vals, format::kNotOwned);
  feature::JaccardWeights<int, int, int, float> jac;
  std::unique_ptr<format::Format> arr(jac.GetJaccardWeights(&csr, {hip_context.get()}, true));
  EXPECT_TRUE(arr->get_id() == format::HIPArray<float>::get_id_static());
  converter::ConverterOrderOne<float> converter;
  std::unique_ptr<format::Array<float>> host(converter.Convert<format::Array<float>>(arr.get(), {&cpu_context}));
  EXPECT_EQ(host->get_dimensions()[0], 4u);
  for (int i = 0; i < 4; i++) EXPECT_EQ(bits(host->get_vals()[i]), 0u);
  EXPECT_THROW(jac.GetJaccardWeights(&csr, {hip_context.get()}, false),
               utils::DirectExecutionNotAvailableException<std::vector<std::type_index>>);
  EXPECT_THROW(jac.GetJaccardWeights(&csr, {&cpu_context}, false), utils::FunctionNotFoundException);
}

// edges 0-1, 0-2, 1-2, 2-3 of an undirected graph
static int ex_row_ptr[5] = {0, 2, 4, 7, 8}, ex_cols[8] = {1, 2, 0, 2, 0, 1, 3, 2};

TEST(Jaccard, WorkedExampleFloat) {
  CSR3 csr(4, 4, ex_row_ptr, ex_cols, nullptr, format::kNotOwned);
  feature::JaccardWeights<int, int, int, float> jac;
  std::unique_ptr<format::Format> arr(jac.GetJaccardWeights(&csr, {hip_context.get()}, true));
  converter::ConverterOrderOne<float> converter;
  std::unique_ptr<format::Array<float>> host(converter.Convert<format::Array<float>>(arr.get(), {&cpu_context}));
  EXPECT_EQ(host->get_dimensions()[0], 8u);
  const float third = (float)1 / (float)3;
  const float want[8] = {third, 0.25f, third, 0.25f, 0.25f, 0.25f, 0.0f, 0.0f};
  EXPECT_EQ(bits(third), 0x3EAAAAABu);
  for (int i = 0; i < 8; i++) EXPECT_EQ(bits(host->get_vals()[i]), bits(want[i]));
}

TEST(Jaccard, WorkedExampleDoubleOnDevice) {  // a HIPCSR runs directly; double holds the float weights widened
  auto &dev = hip::Device::Get(hip_context->device_id);
  int ex_vals[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  format::HIPCSR<int, int, int> dcsr(4, 4, 8, dev.Upload(ex_row_ptr, 5), dev.Upload(ex_cols, 8), dev.Upload(ex_vals, 8),
                                     *hip_context);
  feature::JaccardWeights<int, int, int, double> jac;
  std::unique_ptr<format::Format> arr(
      feature::JaccardWeights<int, int, int, double>::GetJaccardWeightHIPCSR({&dcsr}, nullptr));
  std::unique_ptr<format::Format> arr2(jac.GetJaccardWeights(&dcsr, {hip_context.get()}, false));
  converter::ConverterOrderOne<double> converter;
  std::unique_ptr<format::Array<double>> host(converter.Convert<format::Array<double>>(arr.get(), {&cpu_context}));
  std::unique_ptr<format::Array<double>> host2(converter.Convert<format::Array<double>>(arr2.get(), {&cpu_context}));
  EXPECT_EQ(host->get_dimensions()[0], 8u);
  const double third = (double)((float)1 / (float)3);
  const double want[8] = {third, 0.25, third, 0.25, 0.25, 0.25, 0.0, 0.0};
  EXPECT_TRUE(third == 0.3333333432674408);
  for (int i = 0; i < 8; i++) {
    EXPECT_TRUE(std::memcmp(&host->get_vals()[i], &want[i], sizeof(double)) == 0);
    EXPECT_TRUE(std::memcmp(&host2->get_vals()[i], &want[i], sizeof(double)) == 0);
  }
}

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_jaccard needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
