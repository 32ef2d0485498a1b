// Host-layer tests of io::MTXWriter and io::EdgeListWriter: the scenarios of the reference's mtx_writer_tests.cc and
// edge_list_writer_tests.cc (write, read back with this library's readers, compare), the reference's exceptions with
// their messages — and no file left behind a refusal —, files byte-equal to a plain `ostream <<` loop written here,
// the same files whatever the chunk size, and the device variants equal to the host ones.
// Needs a GPU (host formats are staged through the default device).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

// the chunk size is a compile-time macro of io/writer.h; defined to an expression here, the tests can run every
// scenario with the default and with chunks of 7 entries
static long g_chunk_entries = 1 << 24;
#define SBX_TEXT_CHUNK_ENTRIES g_chunk_entries

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static context::CPUContext cpu_context;
static std::unique_ptr<context::HIPContext> hip_context;
static std::string g_dir;

static std::string path_of(const char *name) { return g_dir + "/" + name; }
static bool exists(const std::string &p) { return std::ifstream(p).is_open(); }
static std::string slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  std::stringstream s;
  s << f.rdbuf();
  return s.str();
}

template <typename V>
struct Matrix {
  int n = 0, m = 0;
  std::vector<int> row, col;
  std::vector<V> val;
};

template <typename V>
static V some_value(std::mt19937 &g) {
  if constexpr (std::is_integral_v<V>) return (V)((int)(g() % 20001) - 10000);
  else {
    static const double mags[] = {1e-7, 1e-3, 0.125, 1.0, 3.0, 1e3, 1e6, 1e9};
    return (V)(((int)(g() % 2000001) - 1000000) / 1000.0 * mags[g() % 8]);
  }
}

template <typename V>
static Matrix<V> general_matrix(int n, int m, int nnz, unsigned seed) {
  std::mt19937 g(seed);
  Matrix<V> a;
  a.n = n; a.m = m;
  for (int i = 0; i < nnz; i++) {
    a.row.push_back((int)(g() % n));
    a.col.push_back((int)(g() % m));
    a.val.push_back(some_value<V>(g));
  }
  return a;
}

// mirrored pairs in a shuffled order, `diag` diagonal entries (zero when skew)
template <typename V>
static Matrix<V> symmetric_matrix(int n, int pairs, int diag, bool skew, unsigned seed) {
  std::mt19937 g(seed);
  Matrix<V> a;
  a.n = a.m = n;
  struct E { int r, c; V v; };
  std::vector<E> e;
  for (int i = 0; i < pairs; i++) {
    const int r = (int)(g() % n), c = (int)(g() % n);
    if (r == c) continue;
    const V v = some_value<V>(g);
    e.push_back({r, c, v});
    e.push_back({c, r, skew ? (V)-v : v});
  }
  for (int i = 0; i < diag; i++) {
    const int d = (int)(g() % n);
    e.push_back({d, d, skew ? (V)0 : some_value<V>(g)});
  }
  std::shuffle(e.begin(), e.end(), g);
  for (auto &x : e) { a.row.push_back(x.r); a.col.push_back(x.c); a.val.push_back(x.v); }
  return a;
}

// what the reference's loops write (io/mtx_writer.cc:201-211, :261-352), as a plain ostream << loop
template <typename V>
static std::string expect_coordinate(const Matrix<V> &a, const std::string &field, const std::string &sym, bool with_vals,
                                     int precision = 6) {
  std::ostringstream o;
  o.precision(precision);
  const bool said = sym != "general", skew = sym == "skew-symmetric";
  long long nnz = (long long)a.row.size(), diag = 0;
  for (size_t i = 0; i < a.row.size(); i++) diag += a.row[i] == a.col[i];
  if (said) nnz = nnz - (nnz - diag) / 2 - (skew ? diag : 0);
  o << "%%MatrixMarket matrix coordinate " << field << " " << sym << "\n" << a.n << " " << a.m << " " << nnz << "\n";
  for (size_t i = 0; i < a.row.size(); i++) {
    const bool keep = !said || a.col[i] < a.row[i] || (!skew && a.col[i] == a.row[i]);
    if (!keep) continue;
    o << a.row[i] + 1 << " " << a.col[i] + 1;
    if (with_vals && field != "pattern") o << " " << a.val[i];
    o << "\n";
  }
  return o.str();
}

template <typename V>
static std::string expect_edges(std::vector<int> row, std::vector<int> col, std::vector<V> val, bool weighted, bool directed,
                                int precision = 6) {
  std::ostringstream o;
  o.precision(precision);
  std::vector<size_t> idx(row.size());
  for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
  if (!directed) {
    for (size_t i = 0; i < row.size(); i++)
      if (row[i] > col[i]) std::swap(row[i], col[i]);
    std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) {
      return row[x] != row[y] ? row[x] < row[y] : col[x] < col[y];
    });
  }
  for (size_t k = 0; k < idx.size(); k++) {
    const size_t i = idx[k];
    if (!directed && k > 0 && row[idx[k - 1]] == row[i] && col[idx[k - 1]] == col[i]) continue;
    o << row[i] << " " << col[i];
    if (weighted) o << " " << val[i];
    o << "\n";
  }
  return o.str();
}

template <typename F>
static void both_chunk_sizes(F body) {
  for (long chunk : {1L << 24, 7L}) {
    g_chunk_entries = chunk;
    body();
  }
  g_chunk_entries = 1 << 24;
}

template <typename V>
static void mtx_all_paths(const Matrix<V> &a, const std::string &field, const std::string &sym, int precision,
                          const std::string &want) {
  const std::string p = path_of("paths.mtx");
  std::vector<int> r = a.row, c = a.col;
  std::vector<V> v = a.val;
  format::COO<int, int, V> coo(a.n, a.m, (int)r.size(), r.data(), c.data(), v.data(), format::kNotOwned, true);
  io::MTXWriter<int, int, V> writer(p, "matrix", "coordinate", field, sym, precision);
  both_chunk_sizes([&] {
    std::remove(p.c_str());
    writer.WriteCOO(&coo);
    EXPECT_TRUE(slurp(p) == want);
    std::unique_ptr<format::HIPCOO<int, int, V>> d(
        new format::HIPCOO<int, int, V>(a.n, a.m, (int)r.size(), hip::Device::Get(hip_context->device_id).Upload(r.data(), r.size()),
                                        hip::Device::Get(hip_context->device_id).Upload(c.data(), c.size()),
                                        hip::Device::Get(hip_context->device_id).Upload(v.data(), v.size()), *hip_context,
                                        format::kOwned, true));
    std::remove(p.c_str());
    writer.WriteHIPCOO(d.get());
    EXPECT_TRUE(slurp(p) == want);
  });
}

TEST(MTXWriter, GeneralFilesEqualTheStreamLoop) {
  const auto f = general_matrix<float>(40, 30, 300, 1);
  mtx_all_paths(f, "real", "general", 6, expect_coordinate(f, "real", "general", true));
  mtx_all_paths(f, "real", "general", 9, expect_coordinate(f, "real", "general", true, 9));
  mtx_all_paths(f, "pattern", "general", 6, expect_coordinate(f, "pattern", "general", true));
  const auto d = general_matrix<double>(25, 25, 200, 2);
  mtx_all_paths(d, "double", "general", 6, expect_coordinate(d, "double", "general", true));
  mtx_all_paths(d, "double", "general", 17, expect_coordinate(d, "double", "general", true, 17));
  const auto i = general_matrix<int>(10, 12, 50, 3);
  mtx_all_paths(i, "integer", "general", 6, expect_coordinate(i, "integer", "general", true));
  const auto e = general_matrix<float>(5, 5, 0, 4);  // no entries
  mtx_all_paths(e, "real", "general", 6, expect_coordinate(e, "real", "general", true));
}

TEST(MTXWriter, SymmetricAndSkewSymmetricFiles) {
  const auto s = symmetric_matrix<float>(30, 100, 8, false, 5);
  mtx_all_paths(s, "real", "symmetric", 6, expect_coordinate(s, "real", "symmetric", true));
  mtx_all_paths(s, "pattern", "symmetric", 6, expect_coordinate(s, "pattern", "symmetric", true));
  const auto k = symmetric_matrix<double>(30, 100, 5, true, 6);
  mtx_all_paths(k, "real", "skew-symmetric", 6, expect_coordinate(k, "real", "skew-symmetric", true));
  const auto si = symmetric_matrix<int>(12, 30, 3, false, 7);
  mtx_all_paths(si, "integer", "symmetric", 6, expect_coordinate(si, "integer", "symmetric", true));
}

TEST(MTXWriter, VoidValuesWriteAPattern) {
  auto a = general_matrix<float>(20, 20, 90, 8);
  const std::string p = path_of("void.mtx");
  format::COO<int, int, void> coo(a.n, a.m, (int)a.row.size(), a.row.data(), a.col.data(), nullptr, format::kNotOwned, true);
  io::MTXWriter<int, int, void>(p, "matrix", "coordinate", "pattern").WriteCOO(&coo);
  EXPECT_TRUE(slurp(p) == expect_coordinate(a, "pattern", "general", false));
  // a value type without values: lines without values, a symmetry check on the coordinates alone
  auto s = symmetric_matrix<float>(15, 40, 4, false, 9);
  format::COO<int, int, float> nov(s.n, s.m, (int)s.row.size(), s.row.data(), s.col.data(), nullptr, format::kNotOwned, true);
  io::MTXWriter<int, int, float>(p, "matrix", "coordinate", "real", "symmetric").WriteCOO(&nov);
  EXPECT_TRUE(slurp(p) == expect_coordinate(s, "real", "symmetric", false));
}

TEST(MTXWriter, WriteReadBackIsTheSameMatrix) {
  // the reference's mtx_writer_tests.cc: write, read, compare — here bit for bit at precision 9 / 17
  auto a = general_matrix<float>(50, 60, 500, 10);
  const std::string p = path_of("roundtrip.mtx");
  format::COO<int, int, float> coo(a.n, a.m, (int)a.row.size(), a.row.data(), a.col.data(), a.val.data(), format::kNotOwned);
  io::MTXWriter<int, int, float>(p, "matrix", "coordinate", "real", "general", 9).WriteCOO(&coo);
  std::unique_ptr<format::COO<int, int, float>> back(io::MTXReader<int, int, float>(p).ReadCOO());
  EXPECT_EQ(back->get_num_nnz(), coo.get_num_nnz());
  EXPECT_EQ(back->get_dimensions()[0], coo.get_dimensions()[0]);
  EXPECT_EQ(back->get_dimensions()[1], coo.get_dimensions()[1]);
  // duplicates of a coordinate may come back in another order: compare as sorted (row, col, bits) triples
  auto triples = [](format::COO<int, int, float> *x) {
    std::vector<std::tuple<int, int, uint32_t>> t;
    for (size_t i = 0; i < x->get_num_nnz(); i++) {
      uint32_t b;
      memcpy(&b, &x->get_vals()[i], 4);
      t.emplace_back(x->get_row()[i], x->get_col()[i], b);
    }
    std::sort(t.begin(), t.end());
    return t;
  };
  EXPECT_TRUE(triples(back.get()) == triples(&coo));
  // CSR and HIPCSR write what the COO of the same matrix writes
  std::unique_ptr<format::CSR<int, int, float>> csr(coo.Convert<format::CSR>(&cpu_context));
  std::unique_ptr<format::COO<int, int, float>> sorted(csr->Convert<format::COO>(&cpu_context));
  io::MTXWriter<int, int, float> w(p, "matrix", "coordinate", "real", "general", 9);
  w.WriteCOO(sorted.get());
  const std::string want = slurp(p);
  both_chunk_sizes([&] {
    std::remove(p.c_str());
    w.WriteCSR(csr.get());
    EXPECT_TRUE(slurp(p) == want);
    std::unique_ptr<format::HIPCSR<int, int, float>> dcsr(csr->Convert<format::HIPCSR>(hip_context.get()));
    std::remove(p.c_str());
    w.WriteHIPCSR(dcsr.get());
    EXPECT_TRUE(slurp(p) == want);
  });
}

TEST(MTXWriter, ArrayFormatAndWriteArray) {
  Matrix<float> a;
  a.n = 4; a.m = 3;
  a.row = {3, 0, 2, 1}; a.col = {2, 0, 1, 1}; a.val = {1.5f, -2.25f, 1e-5f, 123456.7f};
  const std::string p = path_of("array.mtx");
  format::COO<int, int, float> coo(a.n, a.m, 4, a.row.data(), a.col.data(), a.val.data(), format::kNotOwned, true);
  io::MTXWriter<int, int, float>(p, "matrix", "array").WriteCOO(&coo);
  EXPECT_TRUE(slurp(p) == "%%MatrixMarket matrix array real general\n4 3\n-2.25\n0\n0\n0\n0\n123457\n1e-05\n0\n0\n0\n0\n1.5\n");
  // a coordinate stored twice is refused, and no file appears
  std::vector<int> r2 = {0, 0}, c2 = {1, 1};
  std::vector<float> v2 = {1, 2};
  format::COO<int, int, float> dup(2, 2, 2, r2.data(), c2.data(), v2.data(), format::kNotOwned, true);
  std::remove(p.c_str());
  EXPECT_THROW((io::MTXWriter<int, int, float>(p, "matrix", "array").WriteCOO(&dup)), utils::WriterException);
  EXPECT_FALSE(exists(p));
  std::vector<double> vals = {0.5, 2.5, 1000005.0, 999999.5, -0.0, 1e22, 3.0};
  format::Array<double> arr((format::DimensionType)vals.size(), vals.data(), format::kNotOwned);
  both_chunk_sizes([&] {
    io::MTXWriter<int, int, double>(p, "matrix", "array").WriteArray(&arr);
    EXPECT_TRUE(slurp(p) == "%%MatrixMarket matrix array real general\n1 7\n0.5\n2.5\n1e+06\n1e+06\n-0\n1e+22\n3\n");
  });
}

template <typename W>
static std::string message_of(W write) {
  try {
    write();
  } catch (utils::WriterException &e) {
    return e.what();
  }
  return "(no exception)";
}

TEST(MTXWriter, RefusalsCarryTheReferenceMessagesAndLeaveNoFile) {
  auto a = general_matrix<float>(6, 6, 20, 11);
  format::COO<int, int, float> coo(a.n, a.m, (int)a.row.size(), a.row.data(), a.col.data(), a.val.data(), format::kNotOwned, true);
  format::COO<int, int, void> vcoo(a.n, a.m, (int)a.row.size(), a.row.data(), a.col.data(), nullptr, format::kNotOwned, true);
  auto rect = general_matrix<float>(6, 5, 20, 12);
  format::COO<int, int, float> rcoo(rect.n, rect.m, (int)rect.row.size(), rect.row.data(), rect.col.data(), rect.val.data(),
                                    format::kNotOwned, true);
  std::vector<float> av = {1, 2, 3};
  format::Array<float> arr(3, av.data(), format::kNotOwned);
  const std::string p = path_of("refused.mtx");
  std::remove(p.c_str());
  typedef io::MTXWriter<int, int, float> W;
  auto check = [&](const std::string &got, const char *want) {
    EXPECT_TRUE(got == want);
    if (got != want) std::printf("    got \"%s\"\n", got.c_str());
    EXPECT_FALSE(exists(p));
  };
  check(message_of([&] { W(p, "tensor").WriteCOO(&coo); }), "Illegal value for the 'object' option in matrix market header");
  check(message_of([&] { W(p, "vector").WriteCOO(&coo); }), "Matrix market writer does not currently support writing vectors.");
  check(message_of([&] { W(p, "matrix", "dense").WriteCOO(&coo); }), "Illegal value for the 'format' option in matrix market header");
  check(message_of([&] { W(p, "matrix", "coordinate", "rational").WriteCOO(&coo); }),
        "Illegal value for the 'field' option in matrix market header");
  check(message_of([&] { W(p, "matrix", "coordinate", "real", "triangular").WriteCOO(&coo); }),
        "Illegal value for the 'symmetry' option in matrix market header");
  check(message_of([&] { W(p, "matrix", "array", "pattern").WriteCOO(&coo); }),
        "Matrix market files with array format cannot have the field 'pattern' ");
  check(message_of([&] { W(p, "matrix", "array", "real", "symmetric").WriteCOO(&coo); }),
        "Matrix market files with array format cannot have the property 'symmetry' ");
  check(message_of([&] { W(p, "matrix", "coordinate", "real", "hermitian").WriteCOO(&coo); }),
        "Matrix market writer does not currently support hermitian symmetry.");
  check(message_of([&] { io::MTXWriter<int, int, void>(p).WriteCOO(&vcoo); }),
        "Cannot write an MTX with void ValueType, unless field is pattern.");
  check(message_of([&] { W(p, "matrix", "coordinate", "real", "symmetric").WriteCOO(&rcoo); }), "Matrix is not symmetric!");
  check(message_of([&] { W(p, "matrix", "coordinate", "real", "symmetric").WriteCOO(&coo); }), "Matrix is not symmetric!");
  check(message_of([&] { W(p, "matrix", "coordinate").WriteArray(&arr); }),
        "Matrix market writer does not currently support writing array as coordinate.");
  check(message_of([&] { io::MTXWriter<int, int, void>(p, "matrix", "array").WriteArray(nullptr); }),
        "Cannot write an MTX with void ValueType");
  // skew-symmetric with a diagonal entry that is not zero; a pattern is never skew-symmetric (mtx_writer.cc:127-130)
  std::vector<int> r = {0, 1, 2}, c = {1, 0, 2};
  std::vector<float> v = {1.5f, -1.5f, 3.0f};
  format::COO<int, int, float> skew(3, 3, 3, r.data(), c.data(), v.data(), format::kNotOwned, true);
  check(message_of([&] { W(p, "matrix", "coordinate", "real", "skew-symmetric").WriteCOO(&skew); }),
        "Skew-symmetric matrix with non-zero diagonal values!");
  format::COO<int, int, void> vskew(3, 3, 2, r.data(), c.data(), nullptr, format::kNotOwned, true);
  check(message_of([&] { io::MTXWriter<int, int, void>(p, "matrix", "coordinate", "pattern", "skew-symmetric").WriteCOO(&vskew); }),
        "Matrix is not symmetric!");
  // a refused write does not truncate a file that is there
  { std::ofstream keep(p); keep << "keep me\n"; }
  EXPECT_THROW(W(p, "matrix", "coordinate", "real", "symmetric").WriteCOO(&coo), utils::WriterException);
  EXPECT_TRUE(slurp(p) == "keep me\n");
  std::remove(p.c_str());
}

template <typename V>
static void edges_all_paths(const Matrix<V> &a, bool weighted, bool directed, int precision) {
  const std::string p = path_of("edges.txt");
  std::vector<int> r = a.row, c = a.col;
  std::vector<V> v = a.val;
  const std::string want = expect_edges(a.row, a.col, a.val, weighted, directed, precision);
  format::COO<int, int, V> coo(a.n, a.m, (int)r.size(), r.data(), c.data(), weighted ? v.data() : nullptr, format::kNotOwned, true);
  io::EdgeListWriter<int, int, V> writer(p, directed, precision);
  auto &dev = hip::Device::Get(hip_context->device_id);
  both_chunk_sizes([&] {
    std::remove(p.c_str());
    writer.WriteCOO(&coo);
    EXPECT_TRUE(slurp(p) == want);
    std::unique_ptr<format::HIPCOO<int, int, V>> d(new format::HIPCOO<int, int, V>(
        a.n, a.m, (int)r.size(), dev.Upload(r.data(), r.size()), dev.Upload(c.data(), c.size()),
        weighted ? dev.Upload(v.data(), v.size()) : nullptr, *hip_context, format::kOwned, true));
    std::remove(p.c_str());
    writer.WriteHIPCOO(d.get());
    EXPECT_TRUE(slurp(p) == want);
    // the device COO is as it was (an undirected list is made on a copy)
    std::vector<int> r_after(r.size());
    if (!r.empty()) dev.ToHost(r_after.data(), d->get_row(), r.size() * sizeof(int));
    EXPECT_TRUE(r_after == r);
  });
}

TEST(EdgeListWriter, DirectedAndUndirectedWeightedAndNot) {
  const auto a = general_matrix<float>(30, 30, 400, 13);  // duplicates and both directions of many pairs
  for (bool weighted : {false, true})
    for (bool directed : {true, false}) edges_all_paths(a, weighted, directed, 6);
  edges_all_paths(general_matrix<double>(50, 50, 300, 14), true, false, 17);
  edges_all_paths(general_matrix<int>(9, 9, 60, 15), true, false, 6);
  edges_all_paths(general_matrix<float>(9, 9, 0, 16), true, false, 6);
}

TEST(EdgeListWriter, WriteReadBackAndCsrPaths) {
  // the reference's edge_list_writer_tests.cc: write, read back, compare
  auto a = general_matrix<float>(40, 40, 300, 17);
  const std::string p = path_of("edges_rt.txt");
  format::COO<int, int, float> coo(a.n, a.m, (int)a.row.size(), a.row.data(), a.col.data(), a.val.data(), format::kNotOwned);
  io::EdgeListWriter<int, int, float>(p, true, 9).WriteCOO(&coo);
  std::unique_ptr<format::COO<int, int, float>> back(
      io::EdgeListReader<int, int, float>(p, true, false, false, false, false).ReadCOO());
  EXPECT_EQ(back->get_num_nnz(), coo.get_num_nnz());
  bool same = back->get_num_nnz() == coo.get_num_nnz();
  for (size_t i = 0; same && i < coo.get_num_nnz(); i++)
    same = back->get_row()[i] == coo.get_row()[i] && back->get_col()[i] == coo.get_col()[i] &&
           memcmp(&back->get_vals()[i], &coo.get_vals()[i], 4) == 0;
  EXPECT_TRUE(same);
  const std::string want = slurp(p);
  std::unique_ptr<format::CSR<int, int, float>> csr(coo.Convert<format::CSR>(&cpu_context));
  std::unique_ptr<format::HIPCSR<int, int, float>> dcsr(csr->Convert<format::HIPCSR>(hip_context.get()));
  both_chunk_sizes([&] {
    std::remove(p.c_str());
    io::EdgeListWriter<int, int, float>(p, true, 9).WriteCSR(csr.get());
    EXPECT_TRUE(slurp(p) == want);
    std::remove(p.c_str());
    io::EdgeListWriter<int, int, float>(p, true, 9).WriteHIPCSR(dcsr.get());
    EXPECT_TRUE(slurp(p) == want);
  });
}

int main(int argc, char **argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  hip_context.reset(new context::HIPContext(hip::DefaultDevice()));
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
