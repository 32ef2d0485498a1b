// CPU-only tests of utils::ClassMatcherMixin, utils::Implementation (feature::Feature) and feature::Extractor on dummy
// Extractables: six single features A ... F, a fused AB and a fused CDE.  The program includes no device header and
// links nothing of the device library (host/Makefile builds it without -lsbx), so it also runs under
// -fsanitize=address,undefined: the ownership cases below (the slice-copy idiom, a copy that holds added features,
// instances Add does not keep) are what that run is for.
//
// The value a dummy extracts is 1000 * its number + the `v` of the params it was run with, so a result tells which
// params reached the class that computed it.
#include <algorithm>
#include <chrono>
#include <memory>
#include <typeindex>
#include <utility>
#include <vector>

#include "minitest.h"
#include "sparsebase/feature/extractor.h"

using namespace sparsebase;

struct DummyParams : utils::Parameters {
  int v = 0;
};
static int v_of(const std::shared_ptr<utils::Parameters> &p) { return std::static_pointer_cast<DummyParams>(p)->v; }

template <int K>
struct Single : utils::Extractable {
  static constexpr int kNumber = K;
  Single() {
    params_ = std::make_shared<DummyParams>();
    pmap_[typeid(Single)] = params_;
  }
  explicit Single(int v) : Single() { std::static_pointer_cast<DummyParams>(params_)->v = v; }
  std::type_index get_id() override { return typeid(Single); }
  std::vector<std::type_index> get_sub_ids() override { return {typeid(Single)}; }
  std::vector<utils::Extractable *> get_subs() override { return {new Single(*this)}; }
  ParamsPtr get_params() override { return params_; }
  ParamsPtr get_params(std::type_index t) override { return pmap_.at(t); }
  void set_params(std::type_index t, ParamsPtr p) override {
    if (t != std::type_index(typeid(Single))) throw utils::FeatureParamsException("Single", t.name());
    pmap_[t] = p;
    params_ = p;
  }
  FeatureMap Extract(format::Format *, std::vector<context::Context *>, bool) override {
    return {{get_id(), std::any(1000 * K + v_of(params_))}};
  }
};

template <typename... Subs>
struct Fused : utils::Extractable {
  Fused() {
    params_ = std::make_shared<DummyParams>();
    pmap_[typeid(Fused)] = params_;
    ((pmap_[typeid(Subs)] = std::make_shared<DummyParams>()), ...);
  }
  std::type_index get_id() override { return typeid(Fused); }
  std::vector<std::type_index> get_sub_ids() override {
    std::vector<std::type_index> ids = {typeid(Subs)...};
    std::sort(ids.begin(), ids.end());
    return ids;
  }
  std::vector<utils::Extractable *> get_subs() override {
    std::vector<utils::Extractable *> subs = {new Subs()...};
    for (auto *s : subs) s->set_params(s->get_id(), pmap_.at(s->get_id()));
    std::sort(subs.begin(), subs.end(), [](utils::Extractable *a, utils::Extractable *b) { return a->get_id() < b->get_id(); });
    return subs;
  }
  ParamsPtr get_params() override { return params_; }
  ParamsPtr get_params(std::type_index t) override { return pmap_.at(t); }
  void set_params(std::type_index t, ParamsPtr p) override {
    auto ids = get_sub_ids();
    if (std::find(ids.begin(), ids.end(), t) == ids.end()) throw utils::FeatureParamsException("Fused", t.name());
    pmap_[t] = p;
  }
  FeatureMap Extract(format::Format *, std::vector<context::Context *>, bool) override {
    runs()++;
    return {{std::type_index(typeid(Subs)), std::any(1000 * Subs::kNumber + v_of(pmap_.at(typeid(Subs))))}...};
  }
  static int &runs() {
    static int r = 0;
    return r;
  }
};

typedef Single<1> A;
typedef Single<2> B;
typedef Single<3> C;
typedef Single<4> D;
typedef Single<5> E;
typedef Single<6> F;
typedef Single<7> G;  // never registered
typedef Fused<A, B> AB;
typedef Fused<C, D, E> CDE;

struct TestExtractor : feature::Extractor {
  TestExtractor() {
    Reg(new A);
    Reg(new B);
    Reg(new C);
    Reg(new D);
    Reg(new E);
    Reg(new F);
    Reg(new AB);
    Reg(new CDE);
  }
  void Reg(utils::Extractable *c) { RegisterClass(c->get_sub_ids(), c); }
};

template <typename... Ts>
static std::vector<std::type_index> ids_of() {
  return {std::type_index(typeid(Ts))...};
}
static std::vector<std::type_index> chosen(feature::Extractor &e) {
  std::vector<std::type_index> ids;
  for (auto *c : e.GetClasses()) ids.push_back(c->get_id());
  return ids;
}
static std::vector<std::type_index> sorted(std::vector<std::type_index> v) {
  std::sort(v.begin(), v.end());
  return v;
}
template <typename T>
static int value(feature::Extractor::FeatureMap &m) {
  return std::any_cast<int>(m.at(typeid(T)));
}

TEST(ClassMatcher, OneFeatureItsOwnClass) {
  TestExtractor e;
  e.Add(feature::Feature(A{}));
  EXPECT_TRUE(chosen(e) == (ids_of<A>()));
  EXPECT_TRUE(e.GetList() == (ids_of<A>()));
}

TEST(ClassMatcher, TwoFeaturesOfOneFusedClass) {
  TestExtractor e;
  e.Add(feature::Feature(A{}));
  e.Add(feature::Feature(B{}));
  EXPECT_TRUE(chosen(e) == (ids_of<AB>()));
}

TEST(ClassMatcher, AMatchThatLeavesARemainder) {  // the reference reads past `ordered` here
  TestExtractor e;
  e.Add(feature::Feature(C{}));
  e.Add(feature::Feature(B{}));
  e.Add(feature::Feature(A{}));
  EXPECT_TRUE(chosen(e) == (ids_of<AB, C>()));
  auto m = e.Extract(nullptr, {}, true);
  EXPECT_EQ(m.size(), (size_t)3);
  EXPECT_EQ(value<A>(m), 1000);
  EXPECT_EQ(value<B>(m), 2000);
  EXPECT_EQ(value<C>(m), 3000);
}

TEST(ClassMatcher, TheLargestKeyFirst) {
  TestExtractor e;
  e.Add(feature::Feature(A{}));
  e.Add(feature::Feature(B{}));
  e.Add(feature::Feature(C{}));
  e.Add(feature::Feature(D{}));
  e.Add(feature::Feature(E{}));
  EXPECT_TRUE(chosen(e) == (ids_of<CDE, AB>()));
  EXPECT_EQ(e.Extract(nullptr, {}, true).size(), (size_t)5);
}

TEST(ClassMatcher, PartOfAFusedKeyIsNoMatch) {
  TestExtractor e;
  e.Add(feature::Feature(C{}));
  e.Add(feature::Feature(D{}));
  EXPECT_TRUE(sorted(chosen(e)) == sorted(ids_of<C, D>()));
  EXPECT_EQ(chosen(e).size(), (size_t)2);
}

TEST(ClassMatcher, ParamsReachTheMergedClass) {
  TestExtractor e;
  e.Add(feature::Feature(A(7)));
  e.Add(feature::Feature(B(9)));
  const int before = AB::runs();
  auto m = e.Extract(nullptr, {}, true);
  EXPECT_EQ(AB::runs(), before + 1);
  EXPECT_EQ(value<A>(m), 1007);
  EXPECT_EQ(value<B>(m), 2009);
  // a fused feature's subs carry the fused feature's params
  AB ab;
  ab.set_params(typeid(B), std::make_shared<DummyParams>());
  std::static_pointer_cast<DummyParams>(ab.get_params(typeid(B)))->v = 4;
  TestExtractor e2;
  e2.Add(feature::Feature(ab));
  e2.Add(feature::Feature(C(5)));
  m = e2.Extract(nullptr, {}, false);
  EXPECT_EQ(value<A>(m), 1000);
  EXPECT_EQ(value<B>(m), 2004);
  EXPECT_EQ(value<C>(m), 3005);
}

TEST(Extractor, AnUnregisteredFeatureThrows) {
  TestExtractor e;
  EXPECT_THROW(e.Add(feature::Feature(G{})), utils::FeatureException);
  EXPECT_THROW(e.Add(feature::Feature(Fused<A, C>{})), utils::FeatureException);  // registered subs, unregistered key
  EXPECT_TRUE(e.GetList().empty());
  EXPECT_TRUE(e.Extract(nullptr, {}, true).empty());
}

TEST(Extractor, SubtractOfAFusedFeatureRemovesBothSubs) {
  TestExtractor e;
  e.Add(feature::Feature(AB{}));
  e.Add(feature::Feature(A{}));  // there already: the new instance is freed
  e.Add(feature::Feature(F{}));
  EXPECT_TRUE(sorted(e.GetList()) == sorted(ids_of<A, B, F>()));
  e.Subtract(feature::Feature(AB{}));
  EXPECT_TRUE(e.GetList() == (ids_of<F>()));
  e.Subtract(feature::Feature(AB{}));  // nothing to remove
  EXPECT_TRUE(chosen(e) == (ids_of<F>()));
}

TEST(Extractor, TheStaticExtractMergesAndTheFirstWriterStays) {
  std::vector<feature::Feature> fs;
  fs.push_back(feature::Feature(A(1)));
  fs.push_back(feature::Feature(B(2)));
  fs.push_back(feature::Feature(AB{}));
  auto m = feature::Extractor::Extract(fs, nullptr, {}, true);
  EXPECT_EQ(m.size(), (size_t)2);
  EXPECT_EQ(value<A>(m), 1001);
  EXPECT_EQ(value<B>(m), 2002);
}

TEST(Extractor, FuncListNamesEveryRegisteredClass) {
  TestExtractor e;
  auto fl = e.GetFuncList();
  EXPECT_EQ(fl.size(), (size_t)8);
  std::vector<std::type_index> ids;
  for (auto *c : fl) ids.push_back(c->get_id());
  EXPECT_TRUE(sorted(ids) == sorted(ids_of<A, B, C, D, E, F, AB, CDE>()));
}

TEST(Extractor, TheSliceCopyIdiomKeepsTheRegisteredClasses) {
  feature::Extractor engine = TestExtractor();  // the temporary is gone behind this line
  EXPECT_EQ(engine.GetFuncList().size(), (size_t)8);
  engine.Add(feature::Feature(A(3)));
  engine.Add(feature::Feature(B{}));
  EXPECT_TRUE(chosen(engine) == (ids_of<AB>()));
  auto m = engine.Extract(nullptr, {}, true);
  EXPECT_EQ(value<A>(m), 1003);
}

TEST(Extractor, ACopyThatHoldsAddedFeatures) {
  TestExtractor e;
  e.Add(feature::Feature(A(1)));
  e.Add(feature::Feature(B(2)));
  feature::Extractor copy = e;
  e.Subtract(feature::Feature(B{}));
  e.Add(feature::Feature(F(6)));
  EXPECT_TRUE(sorted(copy.GetList()) == sorted(ids_of<A, B>()));
  EXPECT_TRUE(sorted(e.GetList()) == sorted(ids_of<A, F>()));
  auto mc = copy.Extract(nullptr, {}, true);
  auto me = e.Extract(nullptr, {}, true);
  EXPECT_EQ(mc.size(), (size_t)2);
  EXPECT_EQ(value<B>(mc), 2002);
  EXPECT_EQ(me.size(), (size_t)2);
  EXPECT_EQ(value<F>(me), 6006);
  feature::Extractor assigned = TestExtractor();
  assigned = copy;
  EXPECT_TRUE(chosen(assigned) == (ids_of<AB>()));
}

TEST(Implementation, OwnsACopyAndCopiesAndMoves) {
  A a(5);
  feature::Feature f(a);
  EXPECT_TRUE(f->get_id() == std::type_index(typeid(A)));
  feature::Feature g = f;
  feature::Feature h = std::move(f);
  auto mg = g->Extract(nullptr, {}, true), mh = h->Extract(nullptr, {}, true);
  EXPECT_EQ(value<A>(mg), 1005);
  EXPECT_EQ(value<A>(mh), 1005);
  feature::Feature k;
  k = g;
  EXPECT_TRUE(k->get_sub_ids() == (ids_of<A>()));
}

struct ManySingles : feature::Extractor {
  template <size_t... Is>
  void Fill(std::index_sequence<Is...>) {
    (RegisterClass(ids_of<Single<100 + (int)Is>>(), new Single<100 + (int)Is>), ...);
    (Add(feature::Feature(Single<100 + (int)Is>{})), ...);
  }
  ManySingles() {
    RegisterClass(AB().get_sub_ids(), new AB);  // a key of two: the search looks at pairs first
    Fill(std::make_index_sequence<24>());
  }
};

TEST(ClassMatcher, TwentyFourSinglesReturnPromptly) {  // 2^24 lookups per class without the key-size bound
  ManySingles e;
  const auto t0 = std::chrono::steady_clock::now();
  EXPECT_EQ(e.GetClasses().size(), (size_t)24);
  EXPECT_EQ(e.Extract(nullptr, {}, true).size(), (size_t)24);
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("  24 singles matched and extracted in %.3f s\n", s);
  EXPECT_TRUE(s < 5.0);
}

int main() { return minitest::run_all(); }
