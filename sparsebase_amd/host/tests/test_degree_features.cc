// Host-layer tests of the degree-statistic features (AvgDegree, MinDegree, MaxDegree, MinMaxAvgDegree and the seven
// *DegreeColumn classes) and of feature::OffDiagBlockNNZ: every class through Get..., Get...Cached, Extract, get_subs
// and the static ...CSR / ...CSC name, on a host format and on its HIP twin, for <int, int, float>,
// <int64_t, int64_t, double> and <int, long long, float> and both feature types.  The expected values are the real
// reference's outputs, taken from tests/golden/degree_stats.npz (cases reference_test, n4_even, n5_odd,
// uniform_1_100_7, uniform_0_100_7 and the 7 x 7 matrix of off_diag_block_nnz_tests.cc).  Avg, Min, Max, Median and
// OffDiagBlockNNZ must equal them bit for bit; StandardDeviation, CoefficientOfVariation and GeometricAvg come from
// exact integers here and must lie within the bounds tests/test_degree_stats_host.py derives.
// Needs a GPU (the host formats are staged through the default device).
#include <cmath>
#include <cstdint>
#include <memory>
#include <typeindex>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

struct Golden {
  int n;
  long long ptr[9];
  long long min, max;
  // avg, median, standard deviation, coefficient of variation, geometric average: the reference's float and double
  double f32[5], f64[5];
};
static const Golden kGolden[] = {
    {3, {0, 2, 3, 4}, 1, 2,
     {0x1.555556p+0, 0x1p+0, 0x1.a20bd6p-1, 0x1.3988ep-1, 0x1.428a3p+0},
     {0x1.5555555555555p+0, 0x1p+0, 0x1.a20bd700c2c3ep-1, 0x1.3988e1409212fp-1, 0x1.428a2f98d728bp+0}},
    {4, {0, 4, 5, 14, 16}, 1, 9,
     {0x1p+2, 0x1.8p+1, 0x1.8a85c2p+2, 0x1.8a85c2p+0, 0x1.74db92p+1},
     {0x1p+2, 0x1.8p+1, 0x1.8a85c24f70659p+2, 0x1.8a85c24f70659p+0, 0x1.74db90f5e151fp+1}},
    {5, {0, 4, 5, 14, 16, 18}, 1, 9,
     {0x1.ccccccp+1, 0x1p+1, 0x1.9acc5cp+2, 0x1.c8714ap+0, 0x1.59d884p+1},
     {0x1.ccccccccccccdp+1, 0x1p+1, 0x1.9acc59efaf54cp+2, 0x1.c871477c18254p+0, 0x1.59d8845fa620ap+1}},
    {7, {0, 55, 138, 234, 303, 306, 307, 321}, 1, 96,
     {0x1.6edb6ep+5, 0x1.b8p+5, 0x1.835632p+6, 0x1.0e4a8p+1, 0x1.3fa46ep+4},
     {0x1.6edb6db6db6dbp+5, 0x1.b8p+5, 0x1.8356318eea341p+6, 0x1.0e4a80b04a1c6p+1, 0x1.3fa4718876e72p+4}},
    {7, {0, 66, 124, 175, 267, 351, 380, 456}, 29, 92,
     {0x1.04924ap+6, 0x1.08p+6, 0x1.a3bdcep+5, 0x1.9c60a4p-1, 0x1.ebf362p+5},
     {0x1.0492492492492p+6, 0x1.08p+6, 0x1.a3bdcd811be05p+5, 0x1.9c60a5f81b632p-1, 0x1.ebf35d3b868ddp+5}},
};

template <typename F>
static const double *golden_of(const Golden &g) {
  return sizeof(F) == 4 ? g.f32 : g.f64;
}
template <typename F>
static double unit() {
  return sizeof(F) == 4 ? std::ldexp(1.0, -24) : std::ldexp(1.0, -53);
}
// relative distance the derived bounds allow between this project's value and the reference's: half of
// (n + 8) u + 4 u for the root of the sum of squared deviations (the bounds hold in the square), 3 u more for the
// coefficient of variation, (ln(G) (n + 2) + 4) u + u for the geometric average (the n u^2 avg^2 term is below one
// hundredth of an u for these inputs)
template <typename F>
static bool near_rel(F got, double want, double units) {
  return std::fabs((double)got - want) <= units * unit<F>() * std::fabs(want);
}

// one single-valued feature through its whole interface; `check` judges a value
template <typename Feature, typename Result, typename Check, typename GetFn, typename CachedFn, typename StaticFn>
static void walk(format::Format *host, format::Format *device, Check check, GetFn get, CachedFn cached, StaticFn stat) {
  Feature feature;
  EXPECT_EQ(feature.get_sub_ids().size(), (size_t)1);
  EXPECT_TRUE(feature.get_sub_ids()[0] == std::type_index(typeid(feature)));
  EXPECT_TRUE(Feature::get_id_static() == std::type_index(typeid(feature)));
  auto subs = feature.get_subs();
  EXPECT_EQ(subs.size(), (size_t)1);
  EXPECT_TRUE(std::type_index(typeid(*subs[0])) == std::type_index(typeid(feature)));
  EXPECT_NE(subs[0], (utils::Extractable *)&feature);
  delete subs[0];
  typename Feature::ParamsType params;
  Feature with_params(params), copy(feature);
  Feature shared(std::make_shared<typename Feature::ParamsType>());
  Result *r = stat({host}, &params);
  EXPECT_TRUE(check(*r));
  delete r;
  for (Feature *f : {&feature, &with_params, &copy, &shared}) {
    for (bool convert : {true, false}) {
      r = get(*f, host, std::vector<context::Context *>{&cpu_context}, convert);
      EXPECT_TRUE(check(*r));
      delete r;
    }
  }
  auto c = cached(feature, host, std::vector<context::Context *>{&cpu_context}, true);
  EXPECT_TRUE(check(*std::get<1>(c)));
  delete std::get<1>(c);
  auto fmap = feature.Extract(host, {&cpu_context}, true);
  EXPECT_EQ(fmap.size(), (size_t)1);
  for (auto &kv : fmap) EXPECT_TRUE(kv.first == std::type_index(typeid(feature)));
  Result *e = std::any_cast<Result *>(fmap[feature.get_id()]);
  EXPECT_TRUE(check(*e));
  delete e;
  // device-resident input: the HIP twin's implementation, nothing staged
  r = get(feature, device, std::vector<context::Context *>{hip_context.get()}, false);
  EXPECT_TRUE(check(*r));
  delete r;
}

#define WALK(Feature, Result, Name, Kind, host, device, check)                                                    \
  walk<Feature, Result>(                                                                                          \
      host, device, check,                                                                                        \
      [](Feature &f, format::Format *x, std::vector<context::Context *> c, bool v) { return f.Get##Name(x, c, v); }, \
      [](Feature &f, format::Format *x, std::vector<context::Context *> c, bool v) {                              \
        return f.Get##Name##Cached(x, c, v);                                                                      \
      },                                                                                                          \
      [](std::vector<format::Format *> fs, utils::Parameters *p) { return Feature::Get##Name##Kind(fs, p); })

template <typename I, typename N, typename V, typename F>
static void all_features(const Golden &g) {
  const int n = g.n;
  const double *want = golden_of<F>(g);
  std::vector<N> ptr(g.ptr, g.ptr + n + 1);
  const size_t nnz = (size_t)ptr[n];
  std::vector<I> ids(nnz, 0);  // (ignore_sort: the statistics read the offsets only)
  std::vector<V> vals(nnz, 1);
  format::CSR<I, N, V> csr(n, n, ptr.data(), ids.data(), vals.data(), format::kNotOwned, true);
  format::CSC<I, N, V> csc(n, n, ptr.data(), ids.data(), vals.data(), format::kNotOwned, true);
  std::unique_ptr<format::Format> dcsr(csr.template Convert<format::HIPCSR>(hip_context.get()));
  std::unique_ptr<format::Format> dcsc(csc.template Convert<format::HIPCSC>(hip_context.get()));
  EXPECT_TRUE(dcsr->get_id() == (format::HIPCSR<I, N, V>::get_id_static()));
  EXPECT_TRUE(dcsc->get_id() == (format::HIPCSC<I, N, V>::get_id_static()));

  auto is_avg = [&](F v) { return v == (F)want[0]; };
  auto is_min = [&](N v) { return v == (N)g.min; };
  auto is_max = [&](N v) { return v == (N)g.max; };
  auto is_median = [&](F v) { return v == (F)want[1]; };
  auto is_sd = [&](F v) { return near_rel<F>(v, want[2], 0.5 * (n + 12) + 0.01); };
  auto is_cv = [&](F v) { return near_rel<F>(v, want[3], 0.5 * (n + 12) + 3.01); };
  auto is_geo = [&](F v) { return near_rel<F>(v, want[4], std::log(want[4]) * (n + 2) + 5); };

  typedef feature::AvgDegree<I, N, V, F> Avg;
  typedef feature::MinDegree<I, N, V> Min;
  typedef feature::MaxDegree<I, N, V> Max;
  WALK(Avg, F, AvgDegree, CSR, &csr, dcsr.get(), is_avg);
  WALK(Min, N, MinDegree, CSR, &csr, dcsr.get(), is_min);
  WALK(Max, N, MaxDegree, CSR, &csr, dcsr.get(), is_max);
  typedef feature::AvgDegreeColumn<I, N, V, F> AvgC;
  typedef feature::MinDegreeColumn<I, N, V> MinC;
  typedef feature::MaxDegreeColumn<I, N, V> MaxC;
  typedef feature::MedianDegreeColumn<I, N, V, F> MedC;
  typedef feature::StandardDeviationDegreeColumn<I, N, V, F> SdC;
  typedef feature::CoefficientOfVariationDegreeColumn<I, N, V, F> CvC;
  typedef feature::GeometricAvgDegreeColumn<I, N, V, F> GeoC;
  WALK(AvgC, F, AvgDegreeColumn, CSC, &csc, dcsc.get(), is_avg);
  WALK(MinC, N, MinDegreeColumn, CSC, &csc, dcsc.get(), is_min);
  WALK(MaxC, N, MaxDegreeColumn, CSC, &csc, dcsc.get(), is_max);
  WALK(MedC, F, MedianDegreeColumn, CSC, &csc, dcsc.get(), is_median);
  WALK(SdC, F, StandardDeviationDegreeColumn, CSC, &csc, dcsc.get(), is_sd);
  WALK(CvC, F, CoefficientOfVariationDegreeColumn, CSC, &csc, dcsc.get(), is_cv);
  WALK(GeoC, F, GeometricAvgDegreeColumn, CSC, &csc, dcsc.get(), is_geo);

  // MinMaxAvgDegree: the three-entry map, keyed by the sub-features, from every entry of the interface
  typedef feature::MinMaxAvgDegree<I, N, V, F> MMA;
  MMA mma;
  auto ids3 = mma.get_sub_ids();
  EXPECT_EQ(ids3.size(), (size_t)3);
  auto subs = mma.get_subs();
  EXPECT_EQ(subs.size(), (size_t)3);
  for (size_t i = 0; i < subs.size(); i++) {
    EXPECT_TRUE(subs[i]->get_id() == ids3[i]);
    delete subs[i];
  }
  EXPECT_TRUE(std::find(ids3.begin(), ids3.end(), Min::get_id_static()) != ids3.end());
  EXPECT_TRUE(std::find(ids3.begin(), ids3.end(), Max::get_id_static()) != ids3.end());
  EXPECT_TRUE(std::find(ids3.begin(), ids3.end(), Avg::get_id_static()) != ids3.end());
  auto check_map = [&](std::unordered_map<std::type_index, std::any> m) {
    EXPECT_EQ(m.size(), (size_t)3);
    N *mn = std::any_cast<N *>(m[Min::get_id_static()]), *mx = std::any_cast<N *>(m[Max::get_id_static()]);
    F *av = std::any_cast<F *>(m[Avg::get_id_static()]);
    EXPECT_TRUE(is_min(*mn) && is_max(*mx) && is_avg(*av));
    delete mn;
    delete mx;
    delete av;
  };
  feature::Params params;
  check_map(MMA::GetCSR({&csr}, &params));
  check_map(mma.Get(&csr, {&cpu_context}, true));
  check_map(mma.Extract(&csr, {&cpu_context}, false));
  check_map(mma.Get(dcsr.get(), {hip_context.get()}, false));
  check_map(MMA(params).Get(&csr, {&cpu_context}, true));
  check_map(MMA(mma).Get(&csr, {&cpu_context}, true));
}

template <typename I, typename N, typename V>
static void every_golden_case() {
  for (const Golden &g : kGolden) {
    all_features<I, N, V, float>(g);
    all_features<I, N, V, double>(g);
  }
}

TEST(DegreeFeatures, IntIntFloat) { every_golden_case<int, int, float>(); }
TEST(DegreeFeatures, Int64Int64Double) { every_golden_case<int64_t, int64_t, double>(); }
TEST(DegreeFeatures, IntLongLongFloat) { every_golden_case<int, long long, float>(); }

TEST(DegreeFeatures, EmptyColumnMakesTheGeometricAverageZeroAndNoEntriesTheCoefficientNaN) {
  int ptr[5] = {0, 3, 3, 4, 9}, zero[5] = {0, 0, 0, 0, 0}, ids[9] = {0};
  format::CSC<int, int, void> csc(4, 4, ptr, ids, nullptr, format::kNotOwned, true);
  format::CSC<int, int, void> empty(4, 4, zero, ids, nullptr, format::kNotOwned, true);
  feature::GeometricAvgDegreeColumn<int, int, void, float> geo;
  float *g = geo.GetGeometricAvgDegreeColumn(&csc, {&cpu_context}, false);
  EXPECT_EQ(*g, 0.0f);
  delete g;
  feature::CoefficientOfVariationDegreeColumn<int, int, void, double> cv;
  double *c = cv.GetCoefficientOfVariationDegreeColumn(&empty, {&cpu_context}, false);
  EXPECT_TRUE(std::isnan(*c));
  delete c;
  feature::MedianDegreeColumn<int, int, void, float> med;
  float *m = med.GetMedianDegreeColumn(&csc, {&cpu_context}, false);
  EXPECT_EQ(*m, 2.0f);  // degrees 3 0 1 5: (1 + 3) / 2
  delete m;
}

TEST(DegreeFeatures, ColumnFeaturesCountRowsAndRefuseMoreRowsThanColumns) {
  // get_dimensions()[0] degrees are read, as in the reference: 2 of the 4 columns of a 2 x 4 matrix
  int ptr[5] = {0, 1, 4, 4, 6}, ids[6] = {0, 0, 0, 1, 0, 1};
  format::CSC<int, int, void> wide(2, 4, ptr, ids, nullptr, format::kNotOwned, true);
  feature::MaxDegreeColumn<int, int, void> mx;
  int *v = mx.GetMaxDegreeColumn(&wide, {&cpu_context}, false);
  EXPECT_EQ(*v, 3);
  delete v;
  feature::AvgDegreeColumn<int, int, void, float> avg;
  float *a = avg.GetAvgDegreeColumn(&wide, {&cpu_context}, false);
  EXPECT_EQ(*a, 2.0f);
  delete a;
  // 4 x 2: the reference reads past col_ptr
  int tall_ptr[5] = {0, 2, 3, 3, 3}, tall_ids[3] = {0, 1, 3};
  format::CSC<int, int, void> tall(4, 2, tall_ptr, tall_ids, nullptr, format::kNotOwned, true);
  EXPECT_THROW(mx.GetMaxDegreeColumn(&tall, {&cpu_context}, false), utils::FeatureException);
  EXPECT_THROW(avg.GetAvgDegreeColumn(&tall, {&cpu_context}, false), utils::FeatureException);
  feature::MedianDegreeColumn<int, int, void, double> med;
  EXPECT_THROW(med.GetMedianDegreeColumn(&tall, {&cpu_context}, false), utils::FeatureException);
  std::unique_ptr<format::Format> dtall(tall.Convert<format::HIPCSC>(hip_context.get()));
  EXPECT_THROW(mx.GetMaxDegreeColumn(dtall.get(), {hip_context.get()}, false), utils::FeatureException);
  // no implementation for a COO without conversion
  int row[2] = {0, 1}, col[2] = {1, 0};
  format::COO<int, int, void> coo(2, 2, 2, row, col, nullptr, format::kNotOwned);
  EXPECT_THROW(avg.GetAvgDegreeColumn(&coo, {&cpu_context}, false),
               utils::DirectExecutionNotAvailableException<std::vector<std::type_index>>);
}

// off_diag_block_nnz_tests.cc: the 7 x 7 matrix, h = w = 3 gives 8; the other shapes are the fixture's
static int od_rp[8] = {0, 2, 2, 5, 7, 9, 11, 12}, od_col[12] = {2, 3, 0, 3, 4, 0, 2, 2, 5, 4, 6, 5};
static const int od_shapes[8][3] = {{3, 3, 8}, {1, 1, 0}, {7, 7, 12}, {2, 5, 9}, {5, 2, 9}, {10, 3, 11}, {3, 10, 11}, {0, 3, 0}};

template <typename I, typename N>
static void off_diag_flow() {
  std::vector<N> rp(od_rp, od_rp + 8);
  std::vector<I> col(od_col, od_col + 12);
  format::CSR<I, N, void> csr(7, 7, rp.data(), col.data(), nullptr, format::kNotOwned);
  std::unique_ptr<format::Format> dcsr(csr.template Convert<format::HIPCSR>(hip_context.get()));
  typedef feature::OffDiagBlockNNZ<I, N, void> OD;
  for (auto &s : od_shapes) {
    feature::OffDiagBlockNNZParams p(s[0], s[1]);
    const I ans = (I)s[2];
    OD feature(p);
    EXPECT_EQ(feature.get_sub_ids().size(), (size_t)1);
    EXPECT_TRUE(feature.get_sub_ids()[0] == std::type_index(typeid(feature)));
    auto subs = feature.get_subs();
    EXPECT_EQ(subs.size(), (size_t)1);
    EXPECT_TRUE(std::type_index(typeid(*subs[0])) == std::type_index(typeid(feature)));
    EXPECT_NE(subs[0], (utils::Extractable *)&feature);
    delete subs[0];
    I *r = OD::GetOffDiagBlockNNZCSR({&csr}, &p);
    EXPECT_EQ(*r, ans);
    delete r;
    for (bool convert : {true, false}) {
      r = feature.GetOffDiagBlockNNZ(&csr, {&cpu_context}, convert);
      EXPECT_EQ(*r, ans);
      delete r;
    }
    auto cached = feature.GetOffDiagBlockNNZCached(&csr, {&cpu_context}, true);
    EXPECT_EQ(*std::get<1>(cached), ans);
    delete std::get<1>(cached);
    auto fmap = feature.Extract(&csr, {&cpu_context}, true);
    EXPECT_EQ(fmap.size(), (size_t)1);
    I *e = std::any_cast<I *>(fmap[feature.get_id()]);
    EXPECT_EQ(*e, ans);
    delete e;
    r = feature.GetOffDiagBlockNNZ(dcsr.get(), {hip_context.get()}, false);
    EXPECT_EQ(*r, ans);
    delete r;
    r = OD(feature).GetOffDiagBlockNNZ(&csr, {&cpu_context}, true);
    EXPECT_EQ(*r, ans);
    delete r;
    r = OD(std::make_shared<feature::OffDiagBlockNNZParams>(s[0], s[1])).GetOffDiagBlockNNZ(&csr, {&cpu_context}, true);
    EXPECT_EQ(*r, ans);
    delete r;
  }
  // the one-argument constructor is h = w; the default is one block: nothing lies outside it
  feature::OffDiagBlockNNZParams three(3);
  EXPECT_TRUE(three.blockrowsize == 3 && three.blockcolsize == 3);
  I *r = OD().GetOffDiagBlockNNZ(&csr, {&cpu_context}, true);
  EXPECT_EQ(*r, (I)0);
  delete r;
  // no column blocks: the reference divides by zero, here the call is refused
  EXPECT_THROW(OD(feature::OffDiagBlockNNZParams(2, 0)).GetOffDiagBlockNNZ(&csr, {&cpu_context}, true),
               utils::HIPDeviceException);
}

TEST(OffDiagBlockNNZ, IntInt) { off_diag_flow<int, int>(); }
TEST(OffDiagBlockNNZ, Int64Int64) { off_diag_flow<int64_t, int64_t>(); }
TEST(OffDiagBlockNNZ, IntLongLong) { off_diag_flow<int, long long>(); }

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_degree_features needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
