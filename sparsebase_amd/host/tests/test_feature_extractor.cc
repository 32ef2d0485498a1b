// Host-layer tests of feature::Extractor / FeatureExtractor, feature::Feature, the fused classes
// feature::Degrees_DegreeDistribution and feature::Bandwidth_Profile, and bases::GraphFeatureBase: the cases of the
// reference's extractor_tests.cc, degrees_degree_distribution_tests.cc and graph_feature_base_tests.cc restated on this
// layer's fixtures (the 3 x 3 matrix of test_reference_suite.cc, the 7 x 7 matrix of the bandwidth and profile tests),
// plus what this layer adds: the {HIPCSR} implementations, the Bandwidth + Profile fusion, the registered superset.
// Every fused value is compared with the value of the single class.
// Needs a GPU (the host formats are staged through the default device).
#include <algorithm>
#include <cstdint>
#include <memory>
#include <sstream>
#include <typeindex>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;
using feature::Feature;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;

static const int n = 3, nnz = 4;
static int row_ptr[n + 1] = {0, 2, 3, 4}, cols[nnz] = {1, 2, 0, 0}, rows[nnz] = {0, 0, 1, 2}, vals[nnz] = {1, 2, 3, 4};
static const int degrees[n] = {2, 1, 1};
static const int fn = 7, fnnz = 12;
static int frp[fn + 1] = {0, 2, 2, 5, 7, 9, 11, 12}, fcol[fnnz] = {2, 3, 0, 3, 4, 0, 2, 2, 5, 4, 6, 5};

typedef utils::DirectExecutionNotAvailableException<std::vector<std::type_index>> NoDirect;
template <typename T>
static T *take(std::unordered_map<std::type_index, std::any> &m, std::type_index id) {
  return std::any_cast<T *>(m.at(id));
}
static std::vector<std::type_index> chosen(feature::Extractor &e) {
  std::vector<std::type_index> ids;
  for (auto *c : e.GetClasses()) ids.push_back(c->get_id());
  return ids;
}

// ------------------------------------------------------------------ feature/extractor_tests.cc
template <typename I, typename N, typename V, typename F>
static void extractor_add_sub() {
  typedef feature::Degrees<I, N, V> Deg;
  typedef feature::DegreeDistribution<I, N, V, F> Dist;
  typedef feature::Degrees_DegreeDistribution<I, N, V, F> Both;
  feature::Extractor extractor = feature::FeatureExtractor<I, N, V, F>();
  extractor.Add(Feature(Deg{}));
  auto list = extractor.GetList();
  EXPECT_EQ(list.size(), (size_t)1);
  EXPECT_TRUE(list[0] == Deg::get_id_static());
  extractor.Add(Feature(Both{}));
  EXPECT_EQ(extractor.GetList().size(), (size_t)2);
  extractor.Subtract(Feature(Dist{}));
  extractor.Subtract(Feature(Deg{}));
  EXPECT_EQ(extractor.GetList().size(), (size_t)0);
  EXPECT_TRUE(extractor.Extract(nullptr, {&cpu_context}, true).empty());
}
TEST(Extractor, AddAndSubtract) {
  extractor_add_sub<int, int, int, float>();
  extractor_add_sub<int64_t, int64_t, double, double>();
  extractor_add_sub<int, long long, float, float>();
}

TEST(Extractor, ExtractOnACooConvertsOrThrows) {
  format::COO<int, int, int> coo(n, n, nnz, rows, cols, vals, format::kNotOwned);
  typedef feature::Degrees<int, int, int> Deg;
  typedef feature::DegreeDistribution<int, int, int, float> Dist;
  feature::Extractor engine = feature::FeatureExtractor<int, int, int, float>();
  engine.Add(Feature(Deg{}));
  auto raw = engine.Extract(&coo, {&cpu_context}, true);
  EXPECT_EQ(raw.size(), (size_t)1);
  int *deg = take<int>(raw, Deg::get_id_static());
  for (int i = 0; i < n; i++) EXPECT_EQ(deg[i], degrees[i]);
  delete[] deg;
  EXPECT_THROW(engine.Extract(&coo, {&cpu_context}, false), NoDirect);
  engine.Add(Feature(Dist{}));
  auto raw2 = engine.Extract(&coo, {&cpu_context}, true);
  EXPECT_EQ(raw2.size(), (size_t)2);
  deg = take<int>(raw2, Deg::get_id_static());
  float *dist = take<float>(raw2, Dist::get_id_static());
  for (int i = 0; i < n; i++) {
    EXPECT_EQ(deg[i], degrees[i]);
    EXPECT_EQ(dist[i], degrees[i] / (float)nnz);
  }
  delete[] deg;
  delete[] dist;
  EXPECT_THROW(engine.Extract(&coo, {&cpu_context}, false), NoDirect);
}

TEST(Extractor, TheStaticExtractOfGivenFeatures) {
  format::COO<int, int, int> coo(n, n, nnz, rows, cols, vals, format::kNotOwned);
  typedef feature::Degrees<int, int, int> Deg;
  typedef feature::DegreeDistribution<int, int, int, float> Dist;
  std::vector<Feature> features;
  features.push_back(Feature(Deg{}));
  features.push_back(Feature(Dist{}));
  auto results = feature::Extractor::Extract(features, &coo, {&cpu_context}, true);
  EXPECT_EQ(results.size(), (size_t)2);
  delete[] take<int>(results, Deg::get_id_static());
  delete[] take<float>(results, Dist::get_id_static());
  EXPECT_THROW(feature::Extractor::Extract(features, &coo, {&cpu_context}, false), NoDirect);
  // the fused class alone gives the same two keys
  std::vector<Feature> fused;
  fused.push_back(Feature(feature::Degrees_DegreeDistribution<int, int, int, float>{}));
  results = feature::Extractor::Extract(fused, &coo, {&cpu_context}, true);
  EXPECT_EQ(results.size(), (size_t)2);
  delete[] take<int>(results, Deg::get_id_static());
  delete[] take<float>(results, Dist::get_id_static());
}

TEST(Extractor, FeatureHoldsACopy) {
  feature::Degrees<int, int, float> deg;
  Feature f(deg);
  EXPECT_TRUE(f->get_id() == deg.get_id());
  feature::DegreeDistribution<int, int, int, float> dist;
  f = Feature(dist);
  EXPECT_TRUE(f->get_id() == dist.get_id());
  Feature ff(std::move(f));
  EXPECT_TRUE(ff->get_id() == dist.get_id());
  const Feature fff(deg);
  Feature ffff(fff);
  EXPECT_TRUE(ffff->get_id() == deg.get_id());
}

TEST(Extractor, AFeatureOfAnotherFeatureTypeThrows) {
  feature::Extractor engine = feature::FeatureExtractor<int, int, int, double>();
  EXPECT_THROW(engine.Add(Feature(feature::DegreeDistribution<int, int, int, float>{})), utils::FeatureException);
  EXPECT_THROW(engine.Add(Feature(feature::Degrees_DegreeDistribution<int, int, int, float>{})), utils::FeatureException);
  EXPECT_THROW(engine.Add(Feature(feature::Degrees<int64_t, int64_t, int>{})), utils::FeatureException);
  EXPECT_NO_THROW(engine.Add(Feature(feature::DegreeDistribution<int, int, int, double>{})));
  EXPECT_EQ(engine.GetList().size(), (size_t)1);
}

// ------------------------------------------------------------------ the fusion, through GetClasses and through the values
template <typename I, typename N, typename V, typename F>
static void fusion() {
  typedef feature::Degrees<I, N, V> Deg;
  typedef feature::DegreeDistribution<I, N, V, F> Dist;
  typedef feature::Degrees_DegreeDistribution<I, N, V, F> DegDist;
  typedef feature::Bandwidth<I, N, V> Bw;
  typedef feature::Profile<I, N, V> Pr;
  typedef feature::Bandwidth_Profile<I, N, V> BwPr;
  std::vector<N> rp(frp, frp + fn + 1);
  std::vector<I> col(fcol, fcol + fnnz);
  format::CSR<I, N, V> csr(fn, fn, rp.data(), col.data(), nullptr, format::kNotOwned);
  std::unique_ptr<format::Format> dcsr(csr.template Convert<format::HIPCSR>(hip_context.get()));

  // the single classes' own values
  std::unique_ptr<I[]> want_deg(Deg().GetDegrees(&csr, {&cpu_context}, true));
  std::unique_ptr<F[]> want_dist(Dist().GetDistribution(&csr, {&cpu_context}, true));
  std::unique_ptr<int> want_bw(Bw().GetBandwidth(&csr, {&cpu_context}, true));
  std::unique_ptr<I> want_pr(Pr().GetProfile(&csr, {&cpu_context}, true));
  EXPECT_EQ(*want_bw, 4);
  EXPECT_EQ(*want_pr, (I)9);

  feature::Extractor engine = feature::FeatureExtractor<I, N, V, F>();
  engine.Add(Feature(Deg{}));
  engine.Add(Feature(Dist{}));
  EXPECT_TRUE(chosen(engine) == std::vector<std::type_index>{DegDist::get_id_static()});
  engine.Add(Feature(Bw{}));
  EXPECT_EQ(chosen(engine).size(), (size_t)2);  // the fused pair and Bandwidth alone
  engine.Add(Feature(Pr{}));
  auto classes = chosen(engine);
  std::sort(classes.begin(), classes.end());
  std::vector<std::type_index> both = {DegDist::get_id_static(), BwPr::get_id_static()};
  std::sort(both.begin(), both.end());
  EXPECT_TRUE(classes == both);

  struct Input {
    format::Format *f;
    context::Context *c;
    bool convert;
  } inputs[] = {{&csr, &cpu_context, true}, {&csr, &cpu_context, false}, {dcsr.get(), hip_context.get(), false}};
  for (auto &in : inputs) {  // the last one runs in place: no conversion is allowed and none is needed
    auto m = engine.Extract(in.f, {in.c}, in.convert);
    EXPECT_EQ(m.size(), (size_t)4);
    I *deg = take<I>(m, Deg::get_id_static());
    F *dist = take<F>(m, Dist::get_id_static());
    int *bw = take<int>(m, Bw::get_id_static());
    I *pr = take<I>(m, Pr::get_id_static());
    for (int i = 0; i < fn; i++) {
      EXPECT_EQ(deg[i], want_deg[i]);
      EXPECT_EQ(dist[i], want_dist[i]);
      EXPECT_EQ(deg[i], (I)(frp[i + 1] - frp[i]));
    }
    EXPECT_EQ(*bw, *want_bw);
    EXPECT_EQ(*pr, *want_pr);
    delete[] deg;
    delete[] dist;
    delete bw;
    delete pr;
  }
  // the printed list names the fused classes
  std::stringstream captured;
  auto *old = std::cout.rdbuf(captured.rdbuf());
  engine.PrintFuncList();
  std::cout.rdbuf(old);
  EXPECT_TRUE(captured.str().find("Bandwidth_Profile") != std::string::npos);
  EXPECT_TRUE(captured.str().find("Degrees_DegreeDistribution") != std::string::npos);
  EXPECT_TRUE(captured.str().find("MinMaxAvgDegree") != std::string::npos);
  EXPECT_EQ(engine.GetFuncList().size(), (size_t)19);

  // Bandwidth_Profile through its own interface
  BwPr fused;
  auto ids = fused.get_sub_ids();
  EXPECT_EQ(ids.size(), (size_t)2);
  EXPECT_TRUE(ids[0] < ids[1]);
  auto subs = fused.get_subs();
  EXPECT_EQ(subs.size(), (size_t)2);
  for (size_t i = 0; i < subs.size(); i++) {
    EXPECT_TRUE(subs[i]->get_id() == ids[i]);
    delete subs[i];
  }
  feature::Params params;
  for (auto m : {BwPr::GetCSR({&csr}, &params), fused.Get(&csr, {&cpu_context}, true),
                 fused.Extract(dcsr.get(), {hip_context.get()}, false), BwPr(params).Get(&csr, {&cpu_context}, false),
                 BwPr(fused).Get(&csr, {&cpu_context}, true)}) {
    EXPECT_EQ(m.size(), (size_t)2);
    int *bw = take<int>(m, Bw::get_id_static());
    I *pr = take<I>(m, Pr::get_id_static());
    EXPECT_EQ(*bw, 4);
    EXPECT_EQ(*pr, (I)9);
    delete bw;
    delete pr;
  }
  format::COO<I, N, V> empty_coo(fn, fn, 0, (I *)nullptr, (I *)nullptr, (V *)nullptr, format::kNotOwned);
  EXPECT_THROW(fused.Get(&empty_coo, {&cpu_context}, false), NoDirect);
}
TEST(Fusion, IntIntVoid) { fusion<int, int, void, float>(); }
TEST(Fusion, Int64Int64Void) { fusion<int64_t, int64_t, void, double>(); }
TEST(Fusion, IntLongLongVoid) { fusion<int, long long, void, float>(); }

TEST(Fusion, MinMaxAvgIsPickedForItsThree) {
  format::CSR<int, int, void> csr(fn, fn, frp, fcol, nullptr, format::kNotOwned);
  feature::Extractor engine = feature::FeatureExtractor<int, int, void, float>();
  engine.Add(Feature(feature::MinDegree<int, int, void>{}));
  engine.Add(Feature(feature::AvgDegree<int, int, void, float>{}));
  EXPECT_EQ(chosen(engine).size(), (size_t)2);
  engine.Add(Feature(feature::MaxDegree<int, int, void>{}));
  typedef feature::MinMaxAvgDegree<int, int, void, float> MMA;
  EXPECT_TRUE(chosen(engine) == std::vector<std::type_index>{MMA::get_id_static()});
  auto m = engine.Extract(&csr, {&cpu_context}, true);
  EXPECT_EQ(m.size(), (size_t)3);
  int *mn = take<int>(m, feature::MinDegree<int, int, void>::get_id_static());
  int *mx = take<int>(m, feature::MaxDegree<int, int, void>::get_id_static());
  float *av = take<float>(m, feature::AvgDegree<int, int, void, float>::get_id_static());
  EXPECT_EQ(*mn, 0);
  EXPECT_EQ(*mx, 3);
  EXPECT_EQ(*av, 12.0f / 7.0f);
  delete mn;
  delete mx;
  delete av;
}

TEST(Fusion, ParamsOfAnAddedFeatureReachTheRegisteredClass) {
  format::CSR<int, int, void> csr(fn, fn, frp, fcol, nullptr, format::kNotOwned);
  feature::Extractor engine = feature::FeatureExtractor<int, int, void, float>();
  typedef feature::OffDiagBlockNNZ<int, int, void> OD;
  engine.Add(Feature(OD(feature::OffDiagBlockNNZParams(3, 3))));
  auto m = engine.Extract(&csr, {&cpu_context}, true);
  int *v = take<int>(m, OD::get_id_static());
  EXPECT_EQ(*v, 8);  // (one block, the default, gives 0)
  delete v;
}

// ------------------------------------------------------------------ feature/degrees_degree_distribution_tests.cc
struct Params1 : utils::Parameters {};
struct Params2 : utils::Parameters {};

TEST(DegreesDegreeDistribution, FeaturePreprocessType) {
  typedef feature::Degrees_DegreeDistribution<int, int, int, float> Both;
  Both feature;
  std::shared_ptr<Params1> p1(new Params1);
  std::shared_ptr<Params2> p2(new Params2);
  EXPECT_TRUE(std::type_index(typeid(Both)) == feature.get_id());
  EXPECT_THROW(feature.get_params(std::type_index(typeid(int))).get(), utils::FeatureParamsException);
  feature.set_params(feature::Degrees<int, int, int>::get_id_static(), p1);
  EXPECT_TRUE(feature.get_params(feature::Degrees<int, int, int>::get_id_static()).get() == p1.get());
  EXPECT_TRUE(feature.get_params(feature::Degrees<int, int, int>::get_id_static()).get() != p2.get());
  EXPECT_THROW(feature.set_params(typeid(int), p1), utils::FeatureParamsException);
  // the subs carry the params the fused object holds for them
  auto subs = feature.get_subs();
  for (auto *s : subs) {
    if (s->get_id() == feature::Degrees<int, int, int>::get_id_static()) EXPECT_TRUE(s->get_params().get() == p1.get());
    delete s;
  }
  // the constructor from a Params object registers its functions and params (the reference's does not)
  Both from_params{feature::Params()};
  EXPECT_NO_THROW(from_params.get_params(Both::get_id_static()));
  format::CSR<int, int, int> csr(n, n, row_ptr, cols, vals, format::kNotOwned);
  auto m = from_params.Get(&csr, {&cpu_context}, false);
  EXPECT_EQ(m.size(), (size_t)2);
  delete[] take<int>(m, feature::Degrees<int, int, int>::get_id_static());
  delete[] take<float>(m, feature::DegreeDistribution<int, int, int, float>::get_id_static());
}

template <typename I, typename N, typename V, typename F>
static void degrees_degree_distribution() {
  typedef feature::Degrees<I, N, V> Deg;
  typedef feature::DegreeDistribution<I, N, V, F> Dist;
  typedef feature::Degrees_DegreeDistribution<I, N, V, F> Both;
  std::vector<N> rp(row_ptr, row_ptr + n + 1);
  std::vector<I> c(cols, cols + nnz), r(rows, rows + nnz);
  std::vector<V> v(vals, vals + nnz);
  format::CSR<I, N, V> global_csr(n, n, rp.data(), c.data(), v.data(), format::kNotOwned);
  format::COO<I, N, V> global_coo(n, n, nnz, r.data(), c.data(), v.data(), format::kNotOwned);
  std::unique_ptr<format::Format> dcsr(global_csr.template Convert<format::HIPCSR>(hip_context.get()));
  Both feature;
  EXPECT_EQ(feature.get_sub_ids().size(), (size_t)2);
  std::vector<std::type_index> ids = {Deg::get_id_static(), Dist::get_id_static()};
  std::sort(ids.begin(), ids.end());
  EXPECT_TRUE(feature.get_sub_ids() == ids);
  auto subs = feature.get_subs();
  EXPECT_EQ(subs.size(), (size_t)2);
  for (size_t i = 0; i < subs.size(); i++) {
    EXPECT_TRUE(std::type_index(typeid(*subs[i])) == ids[i]);
    EXPECT_NE(subs[i], (utils::Extractable *)&feature);
    delete subs[i];
  }
  Params1 p1;
  for (auto m : {Both::GetCSR({&global_csr}, &p1), feature.Get(&global_csr, {&cpu_context}, true),
                 feature.Get(&global_coo, {&cpu_context}, true), feature.Extract(&global_csr, {&cpu_context}, true),
                 feature.Get(dcsr.get(), {hip_context.get()}, false), Both(feature).Get(&global_csr, {&cpu_context}, false)}) {
    EXPECT_EQ(m.size(), (size_t)2);
    EXPECT_TRUE(m.find(ids[0]) != m.end() && m.find(ids[1]) != m.end());
    I *deg = take<I>(m, Deg::get_id_static());
    F *dist = take<F>(m, Dist::get_id_static());
    for (int i = 0; i < n; i++) {
      EXPECT_EQ(dist[i], (F)degrees[i] / (F)nnz);
      EXPECT_EQ(deg[i], (I)degrees[i]);
    }
    delete[] deg;
    delete[] dist;
  }
  EXPECT_THROW(feature.Get(&global_coo, {&cpu_context}, false), NoDirect);
}
TEST(DegreesDegreeDistribution, IntIntIntFloat) { degrees_degree_distribution<int, int, int, float>(); }
TEST(DegreesDegreeDistribution, Int64Int64DoubleDouble) { degrees_degree_distribution<int64_t, int64_t, double, double>(); }
TEST(DegreesDegreeDistribution, IntLongLongFloatDouble) { degrees_degree_distribution<int, long long, float, double>(); }

// ------------------------------------------------------------------ bases/graph_feature_base_tests.cc
template <typename I, typename N, typename V, typename F>
static void graph_feature_base() {
  std::vector<N> rp(row_ptr, row_ptr + n + 1);
  std::vector<I> c(cols, cols + nnz), r(rows, rows + nnz);
  std::vector<V> v(vals, vals + nnz);
  format::CSR<I, N, V> global_csr(n, n, rp.data(), c.data(), v.data(), format::kNotOwned);
  format::COO<I, N, V> global_coo(n, n, nnz, r.data(), c.data(), v.data(), format::kNotOwned);
  std::unique_ptr<I[]> want_deg(feature::Degrees<I, N, V>().GetDegrees(&global_csr, {&cpu_context}, true));
  std::unique_ptr<F[]> want_dist(feature::DegreeDistribution<I, N, V, F>().GetDistribution(&global_csr, {&cpu_context}, true));
  auto same = [&](I *deg, F *dist) {
    for (int i = 0; i < n; i++) {
      if (deg) EXPECT_TRUE(deg[i] == want_deg[i] && deg[i] == (I)degrees[i]);
      if (dist) EXPECT_TRUE(dist[i] == want_dist[i] && dist[i] == (F)degrees[i] / (F)nnz);
    }
    delete[] deg;
    delete[] dist;
  };
  same(bases::GraphFeatureBase::GetDegrees(&global_csr, {&cpu_context}, true), nullptr);
  same(bases::GraphFeatureBase::GetDegrees(&global_coo, {&cpu_context}, true), nullptr);
  EXPECT_THROW(bases::GraphFeatureBase::GetDegrees(&global_coo, {&cpu_context}, false), NoDirect);
  same(nullptr, bases::GraphFeatureBase::GetDegreeDistribution<F>(&global_csr, {&cpu_context}, true));
  same(nullptr, bases::GraphFeatureBase::GetDegreeDistribution<F>(&global_coo, {&cpu_context}, true));
  EXPECT_THROW(bases::GraphFeatureBase::GetDegreeDistribution<F>(&global_coo, {&cpu_context}, false), NoDirect);
  // cached: a CSR needs no conversion, a COO gives back the CSR that was made of it
  auto d1 = bases::GraphFeatureBase::GetDegreesCached(&global_csr, {&cpu_context});
  EXPECT_EQ(d1.first.size(), (size_t)0);
  same(d1.second, nullptr);
  auto d2 = bases::GraphFeatureBase::GetDegreesCached(&global_coo, {&cpu_context});
  EXPECT_EQ(d2.first.size(), (size_t)1);
  same(d2.second, nullptr);
  auto f1 = bases::GraphFeatureBase::GetDegreeDistributionCached<F>(&global_csr, {&cpu_context});
  EXPECT_EQ(f1.first.size(), (size_t)0);
  same(nullptr, f1.second);
  auto f2 = bases::GraphFeatureBase::GetDegreeDistributionCached<F>(&global_coo, {&cpu_context});
  EXPECT_EQ(f2.first.size(), (size_t)1);
  same(nullptr, f2.second);
  for (auto *made : d2.first) {
    EXPECT_TRUE(made->get_id() == (format::CSR<I, N, V>::get_id_static()));
    delete made;
  }
  for (auto *made : f2.first) delete made;
}
TEST(GraphFeatureBase, IntIntIntFloat) { graph_feature_base<int, int, int, float>(); }
TEST(GraphFeatureBase, Int64Int64DoubleDouble) { graph_feature_base<int64_t, int64_t, double, double>(); }

int main() {
  utils::Logger::set_level(utils::LOG_LVL_NONE);
  if (hip::DeviceCount() < 1) {
    std::printf("test_feature_extractor needs a GPU (the path has no CPU fallback)\n");
    return 2;
  }
  hip_context.reset(new context::HIPContext(0));
  return minitest::run_all();
}
