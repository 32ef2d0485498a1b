// utils/symmetrize.h and RCMReorderParams::symmetrize on the device: MissingMirrors, IsStructurallySymmetric and
// Symmetrize on a host CSR and on an HIPCSR for <int, int, float>, <int64, int64, double> and <int, long long, float>
// against a restatement written here; the rectangular refusal; RCMReorder with and without symmetrize through
// ReorderBase::Reorder, host-array and HIPContext overloads.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <set>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

namespace {

template <typename I, typename N, typename V>
struct Host {
  I n = 0;
  std::vector<N> rp;
  std::vector<I> col;
  std::vector<V> val;
};

// a random n x n CSR with sorted rows, duplicates, diagonals and empty rows; every value tells its position
template <typename I, typename N, typename V>
Host<I, N, V> Random(I n, unsigned seed) {
  Host<I, N, V> h;
  h.n = n;
  h.rp.push_back(0);
  auto next = [&seed]() { return seed = seed * 1664525u + 1013904223u, seed >> 8; };
  for (I i = 0; i < n; i++) {
    std::vector<I> row;
    if (next() % 5) {
      const unsigned len = next() % 7;
      for (unsigned k = 0; k < len; k++) row.push_back((I)(next() % (unsigned)n));
      if (next() % 3 == 0) row.push_back(i);
      if (!row.empty() && next() % 2) row.push_back(row[0]);  // a duplicate
    }
    std::sort(row.begin(), row.end());
    for (I c : row) {
      h.val.push_back((V)(h.col.size() * 3 + 1));
      h.col.push_back(c);
    }
    h.rp.push_back((N)h.col.size());
  }
  return h;
}

// the rule of include/sbsym.h, entry by entry
template <typename I, typename N, typename V>
Host<I, N, V> Restate(const Host<I, N, V> &a, bool no_diagonal, int64_t *added) {
  std::map<std::pair<I, I>, size_t> first;
  for (I j = 0; j < a.n; j++)
    for (N p = a.rp[j]; p < a.rp[j + 1]; p++) first.emplace(std::make_pair(j, a.col[p]), (size_t)p);
  std::vector<std::vector<std::pair<I, size_t>>> rows(a.n);
  for (I i = 0; i < a.n; i++)
    for (N p = a.rp[i]; p < a.rp[i + 1]; p++)
      if (!(no_diagonal && a.col[p] == i)) rows[i].push_back({a.col[p], (size_t)p});
  *added = 0;
  for (auto &e : first) {
    const I j = e.first.first, i = e.first.second;
    if (j != i && !first.count({i, j})) {
      rows[i].push_back({j, e.second});
      ++*added;
    }
  }
  Host<I, N, V> b;
  b.n = a.n;
  b.rp.push_back(0);
  for (auto &r : rows) {
    std::stable_sort(r.begin(), r.end(), [](auto &x, auto &y) { return x.first < y.first; });
    for (auto &e : r) {
      b.col.push_back(e.first);
      b.val.push_back(a.val[e.second]);
    }
    b.rp.push_back((N)b.col.size());
  }
  return b;
}

template <typename T>
bool Same(const T *got, const std::vector<T> &want) {
  return want.empty() || std::memcmp(got, want.data(), want.size() * sizeof(T)) == 0;
}

template <typename I, typename N, typename V>
format::HIPCSR<I, N, V> *ToDevice(Host<I, N, V> &h, I m) {
  auto &dev = hip::Device::Get(hip::DefaultDevice());
  return new format::HIPCSR<I, N, V>(h.n, m, (N)h.col.size(), dev.Upload(h.rp.data(), h.rp.size()),
                                     dev.Upload(h.col.data(), std::max<size_t>(1, h.col.size())),
                                     dev.Upload(h.val.data(), std::max<size_t>(1, h.val.size())),
                                     context::HIPContext(hip::DefaultDevice()), format::kOwned, true);
}

template <typename I, typename N, typename V>
void CheckTuple() {
  for (unsigned seed : {1u, 2u, 3u}) {
    auto a = Random<I, N, V>(seed == 3 ? 1 : 60, seed);
    for (bool nd : {false, true}) {
      int64_t added = 0;
      auto want = Restate(a, nd, &added);
      format::CSR<I, N, V> csr(a.n, a.n, a.rp.data(), a.col.data(), a.val.data(), format::kNotOwned, true);
      EXPECT_EQ(utils::MissingMirrors(&csr), added);
      EXPECT_EQ(utils::IsStructurallySymmetric(&csr), added == 0);
      std::unique_ptr<format::CSR<I, N, V>> b(utils::Symmetrize<I, N, V>(&csr, nd));
      EXPECT_EQ((size_t)b->get_num_nnz(), want.col.size());
      EXPECT_EQ((I)b->get_dimensions()[0], a.n);
      EXPECT_TRUE(Same(b->get_row_ptr(), want.rp) && Same(b->get_col(), want.col) && Same(b->get_vals(), want.val));
      // in HBM
      std::unique_ptr<format::HIPCSR<I, N, V>> d(ToDevice(a, a.n));
      EXPECT_EQ(utils::MissingMirrors(d.get()), added);
      EXPECT_EQ(utils::IsStructurallySymmetric(d.get()), added == 0);
      std::unique_ptr<format::HIPCSR<I, N, V>> db(utils::Symmetrize<I, N, V>(d.get(), nd));
      EXPECT_EQ((size_t)db->get_num_nnz(), want.col.size());
      EXPECT_EQ(db->get_hip_context()->device_id, d->get_hip_context()->device_id);
      auto &dev = db->device();
      std::unique_ptr<N[]> rp(dev.Download(db->get_row_ptr(), want.rp.size()));
      EXPECT_TRUE(Same(rp.get(), want.rp));
      if (!want.col.empty()) {
        std::unique_ptr<I[]> col(dev.Download(db->get_col(), want.col.size()));
        std::unique_ptr<V[]> val(dev.Download(db->get_vals(), want.val.size()));
        EXPECT_TRUE(Same(col.get(), want.col) && Same(val.get(), want.val));
      }
      // the symmetrized matrix lacks nothing
      EXPECT_TRUE(utils::IsStructurallySymmetric(db.get()));
    }
  }
}

}  // namespace

TEST(Symmetrize, IntIntFloat) { CheckTuple<int, int, float>(); }
TEST(Symmetrize, Int64Int64Double) { CheckTuple<int64_t, int64_t, double>(); }
TEST(Symmetrize, IntLongLongFloat) { CheckTuple<int, long long, float>(); }

TEST(Symmetrize, PatternOnly) {
  auto a = Random<int, int, float>(40, 9);
  int64_t added = 0;
  auto want = Restate(a, false, &added);
  format::CSR<int, int, void> csr(a.n, a.n, a.rp.data(), a.col.data(), nullptr, format::kNotOwned, true);
  std::unique_ptr<format::CSR<int, int, void>> b(utils::Symmetrize<int, int, void>(&csr));
  EXPECT_EQ((size_t)b->get_num_nnz(), want.col.size());
  EXPECT_TRUE(Same(b->get_col(), want.col) && b->get_vals() == nullptr);
}

TEST(Symmetrize, RectangularIsRefusedWithBothDimensions) {
  auto a = Random<int, int, float>(6, 4);
  format::CSR<int, int, float> csr(a.n, 9, a.rp.data(), a.col.data(), a.val.data(), format::kNotOwned, true);
  EXPECT_THROW(utils::MissingMirrors(&csr), utils::TypeException);
  EXPECT_THROW(utils::IsStructurallySymmetric(&csr), utils::TypeException);
  std::string what;
  try {
    delete utils::Symmetrize<int, int, float>(&csr);
  } catch (utils::Exception &e) {
    what = e.what();
  }
  EXPECT_TRUE(what.find("6 x 9") != std::string::npos);
  std::unique_ptr<format::HIPCSR<int, int, float>> d(ToDevice(a, 9));
  EXPECT_THROW(delete (utils::Symmetrize<int, int, float>(d.get())), utils::TypeException);
  EXPECT_THROW(utils::MissingMirrors(d.get()), utils::TypeException);
}

// a directed chain k -> k - 1: the sweep from the smallest vertex reaches nothing else
template <typename I, typename N, typename V>
void CheckRcm() {
  const I n = 300;
  Host<I, N, V> a;
  a.n = n;
  a.rp.push_back(0);
  for (I i = 0; i < n; i++) {
    if (i > 0) {
      a.col.push_back(i - 1);
      a.val.push_back((V)1);
    }
    a.rp.push_back((N)a.col.size());
  }
  int64_t added = 0;
  auto s = Restate(a, false, &added);
  EXPECT_EQ(added, (int64_t)n - 1);
  format::CSR<I, N, V> csr(n, n, a.rp.data(), a.col.data(), a.val.data(), format::kNotOwned, true);
  format::CSR<I, N, V> sym(n, n, s.rp.data(), s.col.data(), s.val.data(), format::kNotOwned, true);
  context::HIPContext gpu(hip::DefaultDevice());
  context::CPUContext cpu;
  // without the parameter: the refusal as before, `{}` call sites compile as before
  EXPECT_THROW(delete[] (bases::ReorderBase::Reorder<reorder::RCMReorder>({}, &csr, {&cpu}, true)), utils::HIPDeviceException);
  EXPECT_THROW(delete[] (bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(false), &csr, {&cpu}, true)),
               utils::HIPDeviceException);
  std::unique_ptr<I[]> want(bases::ReorderBase::Reorder<reorder::RCMReorder>({}, &sym, {&cpu}, true));
  std::vector<I> sorted(want.get(), want.get() + n), iota((size_t)n);
  std::sort(sorted.begin(), sorted.end());
  std::iota(iota.begin(), iota.end(), (I)0);
  EXPECT_TRUE(sorted == iota);
  // host arrays
  std::unique_ptr<I[]> got(bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(true), &csr, {&cpu}, true));
  EXPECT_TRUE(std::equal(got.get(), got.get() + n, want.get()));
  // HIPCSR through the function table, and the HIPContext overload (the order stays in HBM)
  std::unique_ptr<format::HIPCSR<I, N, V>> d(ToDevice(a, n));
  std::unique_ptr<I[]> got_d(bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(true), d.get(), {&gpu}, false));
  EXPECT_TRUE(std::equal(got_d.get(), got_d.get() + n, want.get()));
  EXPECT_THROW(delete (bases::ReorderBase::Reorder<reorder::RCMReorder>({}, d.get(), gpu)), utils::HIPDeviceException);
  std::unique_ptr<format::HIPArray<I>> order(
      bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(true), d.get(), gpu));
  std::unique_ptr<I[]> got_a(hip::Device::Get(gpu.device_id).Download(order->get_vals(), (size_t)n));
  EXPECT_TRUE(std::equal(got_a.get(), got_a.get() + n, want.get()));
  // a host CSR through the HIPContext overload
  std::unique_ptr<format::HIPArray<I>> order_h(
      bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(true), &csr, gpu));
  std::unique_ptr<I[]> got_h(hip::Device::Get(gpu.device_id).Download(order_h->get_vals(), (size_t)n));
  EXPECT_TRUE(std::equal(got_h.get(), got_h.get() + n, want.get()));
  // a symmetric pattern: the parameter changes nothing
  std::unique_ptr<I[]> same(bases::ReorderBase::Reorder<reorder::RCMReorder>(reorder::RCMReorderParams(true), &sym, {&cpu}, true));
  EXPECT_TRUE(std::equal(same.get(), same.get() + n, want.get()));
}

TEST(RCMReorderSymmetrize, IntIntFloat) { CheckRcm<int, int, float>(); }
TEST(RCMReorderSymmetrize, Int64Int64Double) { CheckRcm<int64_t, int64_t, double>(); }
TEST(RCMReorderSymmetrize, IntLongLongFloat) { CheckRcm<int, long long, float>(); }

int main(int argc, char **argv) { return minitest::run_all(argc > 1 ? argv[1] : nullptr); }
