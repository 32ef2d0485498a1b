// Host-layer tests of the array-format side of io::MTXReader: ReadCOO / ReadCSR / ReadHIPCOO on array files (dimensions
// as the file states them, entries in (row, col) order, the reference's refusals with their messages), ReadArray /
// ReadHIPArray on array files and on coordinate files of a vector, the IOBase facade over them, and the round trips
// through MTXWriter at the precisions that read back bit-identical (9 for float, 17 for double).
// Needs a GPU (host formats are staged through the default device).
#include <cstdint>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static std::unique_ptr<context::HIPContext> hip_context;
static std::string g_dir;

static std::string path_of(const char *name) { return g_dir + "/" + name; }
static std::string write_file(const char *name, const std::string &text) {
  const std::string p = path_of(name);
  std::ofstream(p, std::ios::binary) << text;
  return p;
}
template <typename F>
static std::string message_of(F f) {
  try {
    f();
  } catch (utils::ReaderException &e) {
    return e.what();
  } catch (std::exception &e) {
    return std::string("another exception: ") + e.what();
  }
  return "no exception";
}
template <typename T>
static bool same_bits(const T *a, const T *b, size_t count) {
  return count == 0 || std::memcmp(a, b, count * sizeof(T)) == 0;
}
template <typename V>
static std::vector<V> some_values(size_t count, unsigned seed, int zero_every) {
  std::mt19937 g(seed);
  static const double mags[] = {1e-30, 1e-7, 1e-3, 0.125, 1.0, 3.0, 1e3, 1e6, 1e20};
  std::vector<V> v(count);
  for (size_t i = 0; i < count; i++) {
    if (std::is_integral_v<V>) v[i] = (V)((int)(g() % 20001) - 10000);
    else v[i] = (V)(((int)(g() % 2000001) - 1000000) / 1000.0 * mags[g() % 9]);
    if (zero_every && g() % zero_every == 0) v[i] = (V)0;
  }
  return v;
}

// a 3 x 2 file: column-major 1 0 3 / 0 5 6 -> entries (0,0)=1 (1,1)=5 (2,0)=3 (2,1)=6
static const char *k3x2 = "%%MatrixMarket matrix array real general\n% a comment\n3 2\n1\n0\n3\n0\n5\n6\n";

TEST(ArrayFile, ReadCOOKeepsTheFilesDimensionsAndRowMajorOrder) {
  const std::string p = write_file("a3x2.mtx", k3x2);
  std::unique_ptr<format::COO<int, int, float>> coo(io::MTXReader<int, int, float>(p).ReadCOO());
  EXPECT_EQ(coo->get_dimensions()[0], (format::DimensionType)3);
  EXPECT_EQ(coo->get_dimensions()[1], (format::DimensionType)2);
  EXPECT_EQ(coo->get_num_nnz(), (format::DimensionType)4);
  const int row[] = {0, 1, 2, 2}, col[] = {0, 1, 0, 1};
  const float val[] = {1, 5, 3, 6};
  EXPECT_TRUE(same_bits(coo->get_row(), row, 4) && same_bits(coo->get_col(), col, 4) && same_bits(coo->get_vals(), val, 4));
}

TEST(ArrayFile, ReadCSRAndReadHIPCOO) {
  const std::string p = write_file("a3x2.mtx", k3x2);
  std::unique_ptr<format::CSR<int, int, double>> csr(io::MTXReader<int, int, double>(p).ReadCSR());
  EXPECT_EQ(csr->get_dimensions()[0], (format::DimensionType)3);
  EXPECT_EQ(csr->get_dimensions()[1], (format::DimensionType)2);
  const int rp[] = {0, 1, 2, 4}, col[] = {0, 1, 0, 1};
  const double val[] = {1, 5, 3, 6};
  EXPECT_TRUE(same_bits(csr->get_row_ptr(), rp, 4) && same_bits(csr->get_col(), col, 4) && same_bits(csr->get_vals(), val, 4));
  std::unique_ptr<format::HIPCOO<long long, long long, double>> d(
      io::MTXReader<long long, long long, double>(p).ReadHIPCOO(*hip_context));
  EXPECT_EQ(d->get_dimensions()[0], (format::DimensionType)3);
  EXPECT_EQ(d->get_num_nnz(), (format::DimensionType)4);
  long long r64[4];
  d->device().ToHost(r64, d->get_row(), sizeof(r64));
  EXPECT_TRUE(r64[0] == 0 && r64[1] == 1 && r64[2] == 2 && r64[3] == 2);
  // all zeros: an empty COO of the file's dimensions
  const std::string z = write_file("zeros.mtx", "%%MatrixMarket matrix array integer general\n2 2\n0 0\n0 0\n");
  std::unique_ptr<format::COO<int, int, int>> zc(io::MTXReader<int, int, int>(z).ReadCOO());
  EXPECT_EQ(zc->get_num_nnz(), (format::DimensionType)0);
  EXPECT_EQ(zc->get_dimensions()[1], (format::DimensionType)2);
}

TEST(ArrayFile, LargerThanATileAgainstAHostLoop) {
  const int M = 131, N = 70;
  const std::vector<double> v = some_values<double>((size_t)M * N, 5, 3);
  std::string text = "%%MatrixMarket matrix array real general\n131 70\n";
  char buf[64];
  for (double x : v) {
    std::snprintf(buf, sizeof(buf), "%.17g\n", x);
    text += buf;
  }
  const std::string p = write_file("a131x70.mtx", text);
  std::unique_ptr<format::COO<int, long long, double>> coo(io::MTXReader<int, long long, double>(p).ReadCOO());
  std::vector<int> row, col;
  std::vector<double> val;
  for (int r = 0; r < M; r++)
    for (int c = 0; c < N; c++)
      if (v[(size_t)c * M + r] != 0) {
        row.push_back(r);
        col.push_back(c);
        val.push_back(v[(size_t)c * M + r]);
      }
  EXPECT_EQ((size_t)coo->get_num_nnz(), row.size());
  EXPECT_TRUE(same_bits(coo->get_row(), row.data(), row.size()) && same_bits(coo->get_col(), col.data(), col.size()) &&
              same_bits(coo->get_vals(), val.data(), val.size()));
}

TEST(ArrayFile, Refusals) {
  using R = io::MTXReader<int, int, float>;
  const std::string sym = write_file("sym.mtx", "%%MatrixMarket matrix array real symmetric\n2 2\n1\n2\n3\n");
  EXPECT_EQ(message_of([&] { delete R(sym).ReadCOO(); }),
            std::string("Library does not support reading array files that are symmetric, skew-symmetric, or hermetian"));
  const std::string skew = write_file("skew.mtx", "%%MatrixMarket matrix array real skew-symmetric\n2 2\n1\n");
  EXPECT_EQ(message_of([&] { delete R(skew).ReadCSR(); }),
            std::string("Library does not support reading array files that are symmetric, skew-symmetric, or hermetian"));
  const std::string pat = write_file("pat.mtx", "%%MatrixMarket matrix array pattern general\n2 2\n");
  EXPECT_EQ(message_of([&] { delete R(pat).ReadHIPCOO(*hip_context); }),
            std::string("Matrix market files with array format cannot have the field 'pattern' "));
  const std::string cplx = write_file("cplx.mtx", "%%MatrixMarket matrix array complex general\n1 2\n1 2\n3 4\n");
  EXPECT_THROW(delete R(cplx).ReadCOO(), utils::ReaderException);
  EXPECT_THROW(delete R(cplx).ReadArray(), utils::ReaderException);
  const std::string few = write_file("short.mtx", "%%MatrixMarket matrix array real general\n2 2\n1 2 3\n");
  EXPECT_THROW(delete R(few).ReadCOO(), utils::ReaderException);
  const std::string frac = write_file("frac.mtx", "%%MatrixMarket matrix array real general\n2 2\n1 1.5 2 3\n");
  EXPECT_THROW((delete io::MTXReader<int, int, int>(frac).ReadCOO()), utils::ReaderException);
  EXPECT_NO_THROW(delete R(frac).ReadCOO());
}

template <typename V>
static void array_round_trip(const char *name, int precision) {
  std::vector<V> v = some_values<V>(5000, 11, 7);
  format::Array<V> arr(v.size(), v.data(), format::kNotOwned);
  const std::string p = path_of(name);
  io::MTXWriter<int, int, V>(p, "matrix", "array", "real", "general", precision).WriteArray(&arr);
  std::unique_ptr<format::Array<V>> back(io::MTXReader<int, int, V>(p).ReadArray());
  EXPECT_EQ((size_t)back->get_dimensions()[0], v.size());
  EXPECT_TRUE(same_bits(back->get_vals(), v.data(), v.size()));
  std::unique_ptr<format::HIPArray<V>> d(io::MTXReader<int, int, V>(p).ReadHIPArray(*hip_context));
  EXPECT_EQ((size_t)d->get_dimensions()[0], v.size());
  std::vector<V> host(v.size());
  hip::Device::Get(hip_context->device_id).ToHost(host.data(), d->get_vals(), v.size() * sizeof(V));
  EXPECT_TRUE(same_bits(host.data(), v.data(), v.size()));
}

TEST(ReadArray, WriteArrayReadsBackBitIdentical) {
  array_round_trip<float>("arr_f32.mtx", 9);
  array_round_trip<double>("arr_f64.mtx", 17);
}

TEST(ReadArray, CoordinateFilesOfAVector) {
  // 1 x N, unsorted, one position stored twice: the later one in (row, col) order — here in file order — wins
  const std::string row_vec = write_file("c1xn.mtx",
                                         "%%MatrixMarket matrix coordinate real general\n1 6 4\n1 5 2.5\n1 2 -1\n1 5 7\n1 6 0.125\n");
  std::unique_ptr<format::Array<double>> a(io::MTXReader<int, int, double>(row_vec).ReadArray());
  EXPECT_EQ(a->get_dimensions()[0], (format::DimensionType)6);
  const double want[] = {0, -1, 0, 0, 7, 0.125};
  EXPECT_TRUE(same_bits(a->get_vals(), want, 6));
  const std::string col_vec = write_file("cnx1.mtx", "%%MatrixMarket matrix coordinate integer general\n5 1 2\n5 1 9\n1 1 -4\n");
  std::unique_ptr<format::Array<int>> b(io::MTXReader<int, int, int>(col_vec).ReadArray());
  EXPECT_EQ(b->get_dimensions()[0], (format::DimensionType)5);
  const int want_b[] = {-4, 0, 0, 0, 9};
  EXPECT_TRUE(same_bits(b->get_vals(), want_b, 5));
  // 64-bit ids, an empty coordinate file
  const std::string empty = write_file("cempty.mtx", "%%MatrixMarket matrix coordinate real general\n4 1 0\n");
  std::unique_ptr<format::Array<float>> e(io::MTXReader<long long, long long, float>(empty).ReadArray());
  const float zeros[4] = {0, 0, 0, 0};
  EXPECT_EQ(e->get_dimensions()[0], (format::DimensionType)4);
  EXPECT_TRUE(same_bits(e->get_vals(), zeros, 4));
  // read as is (no conversion to zero-based ids), the last position is N: outside the vector, refused
  EXPECT_THROW((delete io::MTXReader<int, int, double>(row_vec, false).ReadArray()), utils::ReaderException);
}

TEST(ReadArray, Refusals) {
  const std::string mat = write_file("c2x3.mtx", "%%MatrixMarket matrix coordinate real general\n2 3 1\n1 1 1\n");
  EXPECT_EQ(message_of([&] { delete io::MTXReader<int, int, float>(mat).ReadArray(); }),
            std::string("Trying to read a 2D matrix with multiple rows and multiple columns into dense array"));
  const std::string amat = write_file("a3x2.mtx", k3x2);
  EXPECT_EQ(message_of([&] { delete io::MTXReader<int, int, float>(amat).ReadArray(); }),
            std::string("Trying to read a 2D matrix with multiple rows and multiple columns into dense array"));
  const std::string pat = write_file("cpat.mtx", "%%MatrixMarket matrix coordinate pattern general\n1 3 1\n1 2\n");
  EXPECT_EQ(message_of([&] { delete io::MTXReader<int, int, float>(pat).ReadArray(); }),
            std::string("Cannot read a matrix market file into an Array if it is in pattern format"));
  EXPECT_EQ(message_of([&] { (void)io::MTXReader<int, int, void>(pat).ReadArray(); }),
            std::string("Cannot read a matrix market file into an Array whose ValueType is void"));
}

TEST(IOBase, ReadMTXToArrayAndTheMTXWriters) {
  using bases::IOBase;
  std::vector<float> v = some_values<float>(300, 21, 0);
  format::Array<float> arr(v.size(), v.data(), format::kNotOwned);
  const std::string pa = path_of("io_arr.mtx");
  // the reference's default format for an Array is "coordinate", which WriteArray refuses
  EXPECT_THROW((IOBase::WriteArrayToMTX<int, int, float>(&arr, pa)), utils::WriterException);
  IOBase::WriteArrayToMTX<int, int, float>(&arr, pa, "matrix", "array", "real", "general", 9);
  std::unique_ptr<format::Array<float>> back(IOBase::ReadMTXToArray<int, int, float>(pa));
  EXPECT_EQ((size_t)back->get_dimensions()[0], v.size());
  EXPECT_TRUE(same_bits(back->get_vals(), v.data(), v.size()));

  // a sorted COO without stored zeros, through both formats of both writers
  const int n = 90, m = 70;
  std::mt19937 g(3);
  std::vector<int> row, col;
  std::vector<double> val;
  for (int r = 0; r < n; r++)
    for (int c = 0; c < m; c++)
      if (g() % 9 == 0) {
        row.push_back(r);
        col.push_back(c);
        val.push_back(((int)(g() % 20001) - 10000) / 7.0 + 0.001);
      }
  const size_t nnz = row.size();
  format::COO<int, int, double> coo(n, m, (int)nnz, row.data(), col.data(), val.data(), format::kNotOwned);
  std::vector<int> rp(n + 1, 0);
  for (int r : row) rp[r + 1]++;
  for (int r = 0; r < n; r++) rp[r + 1] += rp[r];
  format::CSR<int, int, double> csr_host(n, m, rp.data(), col.data(), val.data(), format::kNotOwned);
  format::CSR<int, int, double> *csr = &csr_host;
  for (const char *fmt : {"coordinate", "array"}) {
    const std::string pc = path_of("io_coo.mtx"), pr = path_of("io_csr.mtx");
    IOBase::WriteCOOToMTX<int, int, double>(&coo, pc, "matrix", fmt, "real", "general", 17);
    IOBase::WriteCSRToMTX<int, int, double>(csr, pr, "matrix", fmt, "real", "general", 17);
    for (const std::string &p : {pc, pr}) {
      std::unique_ptr<format::COO<int, int, double>> b(IOBase::ReadMTXToCOO<int, int, double>(p));
      EXPECT_EQ(b->get_dimensions()[0], (format::DimensionType)n);
      EXPECT_EQ(b->get_dimensions()[1], (format::DimensionType)m);
      EXPECT_EQ((size_t)b->get_num_nnz(), nnz);
      EXPECT_TRUE(same_bits(b->get_row(), row.data(), nnz) && same_bits(b->get_col(), col.data(), nnz) &&
                  same_bits(b->get_vals(), val.data(), nnz));
      std::unique_ptr<format::CSR<int, int, double>> c(IOBase::ReadMTXToCSR<int, int, double>(p));
      EXPECT_TRUE(same_bits(c->get_row_ptr(), csr->get_row_ptr(), (size_t)n + 1) && same_bits(c->get_col(), col.data(), nnz));
    }
  }
}

int main(int argc, char **argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  hip_context.reset(new context::HIPContext(hip::DefaultDevice()));
  return minitest::run_all(argc > 2 ? argv[2] : nullptr);
}
