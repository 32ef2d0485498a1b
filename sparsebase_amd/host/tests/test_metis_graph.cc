// Host-layer tests of io::MetisGraphReader, io::MetisGraphWriter and object::Graph: the reference's two gtest files
// (tests/suites/sparsebase/io/metis_graph_reader_tests.cc, metis_graph_writer_tests.cc) transcribed for minitest.h over
// the two files they use (kept as fixtures: tests/golden/metis_tiny_03.graph, metis_tiny_04.graph), the bytes the writer
// leaves, the refusals, and a round trip read -> RCM -> permute -> write -> read on the device.
// Usage: test_metis_graph <scratch dir> <fixture dir> [filter].  Needs a GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

// the chunk size is a compile-time macro of io/writer.h; defined to an expression here, the writer can be run with the
// default and with chunks of a few items (as test_text_writers.cc does)
static long g_chunk_entries = 1 << 24;
#define SBX_TEXT_CHUNK_ENTRIES g_chunk_entries

#include "minitest.h"
#include "sparsebase/sparsebase.h"

using namespace sparsebase;

static std::unique_ptr<context::HIPContext> hip_context;
static std::string g_dir, g_fixtures;

static std::string path_of(const std::string &name) { return g_dir + "/" + name; }
static std::string write_file(const std::string &name, const std::string &text) {
  const std::string p = path_of(name);
  std::ofstream(p, std::ios::binary) << text;
  return p;
}
static std::string slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static bool exists(const std::string &p) { return std::ifstream(p).is_open(); }
template <typename F>
static std::string message_of(F f) {
  try {
    f();
  } catch (utils::Exception &e) {
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

// What a well-formed file says, read the plain way (line by line, no comments, every vertex has a line): the expected
// value of the tests below.  Rows and neighbours as the file numbers them (1-based).
struct Plain {
  int n = 0, m = 0, fmt = 0, ncon = 0;
  std::vector<int> row, col, val;
  std::vector<std::vector<int>> vw;  // [vertex 1-based][j]; vw[0] is the zero vector
};
static Plain plain_read(const std::string &path) {
  std::ifstream f(path);
  std::string line;
  std::getline(f, line);
  Plain p;
  std::istringstream head(line);
  head >> p.n >> p.m >> p.fmt >> p.ncon;
  const bool ew = p.fmt == 1 || p.fmt == 11;
  if (ew && p.ncon == 0) p.ncon = 1;
  const bool vw = p.fmt >= 10 && p.ncon > 0;
  p.vw.assign(p.n + 1, std::vector<int>(p.ncon, 0));
  for (int v = 1; v <= p.n && std::getline(f, line); v++) {
    std::istringstream iss(line);
    if (vw)
      for (int j = 0; j < p.ncon; j++) iss >> p.vw[v][j];
    std::vector<std::pair<int, int>> nb;
    int c, w = 0;
    while (iss >> c) {
      if (ew) iss >> w;
      nb.push_back({c, w});
    }
    std::sort(nb.begin(), nb.end());
    for (auto &e : nb) p.row.push_back(v), p.col.push_back(e.first), p.val.push_back(e.second);
  }
  return p;
}

// reader_tests.cc:19-58 / :60-98 / :100-139 / :141-179 for one file and one index mode
static void check_read(const std::string &file, bool zero, bool edge_weights) {
  const Plain p = plain_read(file);
  std::unique_ptr<object::Graph<int, int, int>> g(io::MetisGraphReader<int, int, int>(file, zero).ReadGraph());
  auto *coo = g->get_connectivity()->AsAbsolute<format::COO<int, int, int>>();
  const int off = zero ? 1 : 0;
  EXPECT_EQ((int)coo->get_dimensions()[0], p.n + 1 - off);
  EXPECT_EQ((int)coo->get_num_nnz(), 2 * p.m);
  EXPECT_EQ((int)g->n_, p.n + 1 - off);
  EXPECT_EQ((int)g->m_, 2 * p.m);
  EXPECT_EQ((int)g->ncon_, p.ncon);
  EXPECT_NE(coo->get_row(), nullptr);
  EXPECT_NE(coo->get_col(), nullptr);
  EXPECT_EQ(coo->get_vals() != nullptr, edge_weights);
  EXPECT_NE(g->vertexWeights_, nullptr);
  if ((size_t)coo->get_num_nnz() != p.row.size() || !g->vertexWeights_) return;
  for (size_t i = 0; i < p.row.size(); i++) {
    EXPECT_EQ(coo->get_row()[i], p.row[i] - off);
    EXPECT_EQ(coo->get_col()[i], p.col[i] - off);
    if (edge_weights) EXPECT_EQ(coo->get_vals()[i], p.val[i]);
  }
  for (int v = 0; v < p.n + 1 - off; v++)
    for (int j = 0; j < p.ncon; j++) EXPECT_EQ(g->vertexWeights_[v]->get_vals()[j], p.vw[v + off][j]);
}

TEST(MetisGraphReader, ReadGraph) {
  const std::string f1 = g_fixtures + "/metis_tiny_03.graph", f2 = g_fixtures + "/metis_tiny_04.graph";
  check_read(f1, false, true);
  check_read(f2, false, false);
  check_read(f1, true, true);
  check_read(f2, true, false);
  // reader_tests.cc:181-207: ValueType void
  const Plain p = plain_read(f1);
  std::unique_ptr<object::Graph<int, int, void>> g(io::MetisGraphReader<int, int, void>(f1, false).ReadGraph());
  auto *coo = g->get_connectivity()->AsAbsolute<format::COO<int, int, void>>();
  EXPECT_EQ((int)coo->get_dimensions()[0], p.n + 1);
  EXPECT_EQ((int)coo->get_num_nnz(), 2 * p.m);
  EXPECT_EQ((int)g->ncon_, 0);
  EXPECT_EQ(coo->get_vals(), nullptr);
  EXPECT_EQ(g->vertexWeights_, nullptr);
  EXPECT_TRUE(same_bits(coo->get_row(), p.row.data(), p.row.size()) && same_bits(coo->get_col(), p.col.data(), p.col.size()));
  // 64-bit ids, float weights, on the device
  std::unique_ptr<object::Graph<long long, long long, float>> d(
      io::MetisGraphReader<long long, long long, float>(f1, true).ReadHIPGraph(*hip_context));
  auto *dcoo = d->get_connectivity()->AsAbsolute<format::HIPCOO<long long, long long, float>>();
  std::vector<long long> col(p.col.size());
  std::vector<float> val(p.col.size());
  auto &dev = hip::Device::Get(hip_context->device_id);
  dev.ToHost(col.data(), dcoo->get_col(), col.size() * sizeof(long long));
  dev.ToHost(val.data(), dcoo->get_vals(), val.size() * sizeof(float));
  for (size_t i = 0; i < col.size(); i++) EXPECT_TRUE(col[i] == p.col[i] - 1 && val[i] == (float)p.val[i]);
  EXPECT_EQ(d->vertexWeights_[0]->get_vals()[0], (float)p.vw[1][0]);
}

// writer_tests.cc: read, write, read what was written, compare everything
template <typename V>
static void check_write(const std::string &file, bool ew, bool vw, bool zero, const std::string &out_name) {
  std::unique_ptr<object::Graph<int, int, V>> org(io::MetisGraphReader<int, int, V>(file, zero).ReadGraph());
  const std::string out = path_of(out_name);
  io::MetisGraphWriter<int, int, V>(out, ew, vw, zero).WriteGraph(org.get());
  std::unique_ptr<object::Graph<int, int, V>> got(io::MetisGraphReader<int, int, V>(out, zero).ReadGraph());
  auto *a = org->get_connectivity()->template AsAbsolute<format::COO<int, int, V>>();
  auto *b = got->get_connectivity()->template AsAbsolute<format::COO<int, int, V>>();
  EXPECT_EQ(a->get_dimensions()[0], b->get_dimensions()[0]);
  EXPECT_EQ(a->get_num_nnz(), b->get_num_nnz());
  if (a->get_num_nnz() != b->get_num_nnz()) return;
  const size_t nnz = a->get_num_nnz();
  EXPECT_TRUE(same_bits(a->get_row(), b->get_row(), nnz) && same_bits(a->get_col(), b->get_col(), nnz));
  if constexpr (!std::is_same_v<V, void>) {
    EXPECT_EQ(org->ncon_, got->ncon_);
    if (ew) EXPECT_TRUE(b->get_vals() && same_bits(a->get_vals(), b->get_vals(), nnz));
    if (vw)
      for (size_t v = 0; v < (size_t)a->get_dimensions()[0]; v++)
        EXPECT_TRUE(same_bits(org->vertexWeights_[v]->get_vals(), got->vertexWeights_[v]->get_vals(), (size_t)org->ncon_));
  } else {
    EXPECT_EQ((int)got->ncon_, 0);
    EXPECT_EQ(got->vertexWeights_, nullptr);
  }
}

TEST(MetisGraphWriter, WriteGraph) {
  const std::string f1 = g_fixtures + "/metis_tiny_03.graph", f2 = g_fixtures + "/metis_tiny_04.graph";
  check_write<int>(f1, true, true, false, "org1.graph");
  check_write<int>(f2, false, true, false, "org2.graph");
  check_write<int>(f1, true, true, true, "org3.graph");
  check_write<void>(f1, false, false, false, "org4.graph");
}

TEST(MetisGraphWriter, TheBytes) {
  const std::string f = write_file("tiny.graph", "% c\n4 2 11 2\n5 6 2 7\n1.5 2 1 7 3 0.25\n0 0 2 0.25\n\n");
  std::unique_ptr<object::Graph<int, int, float>> g(io::MetisGraphReader<int, int, float>(f, true).ReadGraph());
  EXPECT_EQ((int)g->ncon_, 2);
  const std::string out = path_of("tiny_out.graph");
  const std::string both = " 4 2 11 2\n5 6    2 7\n1.5 2    1 7   3 0.25\n0 0    2 0.25\n0 0   \n";
  io::MetisGraphWriter<int, int, float>(out, true, true, true).WriteGraph(g.get());
  EXPECT_EQ(slurp(out), both);
  io::MetisGraphWriter<int, int, float>(out, false, false, true).WriteGraph(g.get());
  EXPECT_EQ(slurp(out), std::string(" 4 2 10\n 2\n 1  3\n 2\n\n"));
  io::MetisGraphWriter<int, int, float>(out, true, false, true).WriteGraph(g.get());
  EXPECT_EQ(slurp(out), std::string(" 4 2 1\n 2 7\n 1 7   3 0.25\n 2 0.25\n\n"));
  // not zero-indexed: the arrays are 1-based already and row 0 is not written
  std::unique_ptr<object::Graph<int, int, float>> g1(io::MetisGraphReader<int, int, float>(f, false).ReadGraph());
  io::MetisGraphWriter<int, int, float>(out, false, true, false).WriteGraph(g1.get());
  EXPECT_EQ(slurp(out), std::string(" 4 2 10 2\n5 6    2\n1.5 2    1  3\n0 0    2\n0 0   \n"));
  // the connectivity on the device gives the same file
  std::unique_ptr<object::Graph<int, int, float>> gd(io::MetisGraphReader<int, int, float>(f, true).ReadHIPGraph(*hip_context));
  io::MetisGraphWriter<int, int, float>(out, true, true, true).WriteGraph(gd.get());
  EXPECT_EQ(slurp(out), both);
  // the same bytes whatever the chunk: a row weighs its entries + 1 + ncon items (4, 5, 4 and 3 here), so chunks of 7
  // items are rows {0}, {1} and {2, 3}, and a chunk smaller than any row still takes one row at a time
  for (long chunk : {7L, 1L}) {
    g_chunk_entries = chunk;
    io::MetisGraphWriter<int, int, float>(out, true, true, true).WriteGraph(gd.get());
    EXPECT_EQ(slurp(out), both);
    io::MetisGraphWriter<int, int, float>(out, false, true, false).WriteGraph(g1.get());
    EXPECT_EQ(slurp(out), std::string(" 4 2 10 2\n5 6    2\n1.5 2    1  3\n0 0    2\n0 0   \n"));
  }
  g_chunk_entries = 1 << 24;
}

TEST(MetisGraph, Refusals) {
  EXPECT_EQ(message_of([&] { delete io::MetisGraphReader<int, int, int>(path_of("no_such.graph")).ReadGraph(); }),
            std::string("file does not exist!"));
  const std::string short_file = write_file("short.graph", "3 3\n2 3\n1\n");
  const std::string msg = message_of([&] { delete io::MetisGraphReader<int, int, int>(short_file, true).ReadGraph(); });
  EXPECT_TRUE(msg.find("3 neighbours") != std::string::npos && msg.find("needs 6") != std::string::npos);
  for (const char *text : {"\n3 1\n2\n1\n", "% only\n", "3\n", "3 1 100\n2\n1\n", "3 1\n2\n4\n", "3 1\n2\n1x\n", "2 1\n2\n1\n\n\n",
                           "3 2 1\n2 5 3\n1 5\n3 1\n"}) {
    const std::string p = write_file("bad.graph", text);
    EXPECT_THROW((delete io::MetisGraphReader<int, int, int>(p, true).ReadGraph()), utils::ReaderException);
  }
  // the writer's: before the file is opened
  const std::string f = write_file("plain.graph", "2 1\n2\n1\n");
  std::unique_ptr<object::Graph<int, int, float>> g(io::MetisGraphReader<int, int, float>(f, true).ReadGraph());
  const std::string out = path_of("refused.graph");
  EXPECT_THROW((io::MetisGraphWriter<int, int, float>(out, true, false, true).WriteGraph(g.get())), utils::WriterException);
  EXPECT_THROW((io::MetisGraphWriter<int, int, float>(out, false, true, true).WriteGraph(g.get())), utils::WriterException);
  EXPECT_THROW((io::MetisGraphWriter<int, int, float>(out, false, false, true, 18).WriteGraph(g.get())), utils::WriterException);
  EXPECT_FALSE(exists(out));
}

TEST(Graph, ConnectivityAndCopies) {
  const std::string f = g_fixtures + "/metis_tiny_04.graph";
  std::unique_ptr<object::Graph<int, int, int>> g(io::MetisGraphReader<int, int, int>(f, true).ReadGraph());
  EXPECT_TRUE(g->ConnectivityIsOwned());
  object::Graph<int, int, int> copy(*g);  // object.cc:69-74: the connectivity alone
  EXPECT_TRUE(copy.get_connectivity() != g->get_connectivity() && copy.n_ == g->n_ && copy.m_ == g->m_);
  EXPECT_EQ((int)copy.ncon_, 0);
  EXPECT_EQ(copy.vertexWeights_, nullptr);
  format::Format *raw = copy.release_connectivity();
  EXPECT_FALSE(copy.ConnectivityIsOwned());
  object::Graph<int, int, int> adopted(raw);
  EXPECT_EQ(adopted.m_, g->m_);
  int one[1] = {1};
  format::Array<int> one_dim(1, one);
  EXPECT_THROW((object::Graph<int, int, int>(new format::Array<int>(one_dim))), int);
}

// a .graph file in, RCM and permute on the device, a .graph file out that reads back to the permuted arrays
TEST(MetisGraph, ReadReorderPermuteWriteRead) {
  std::mt19937 rng(5);
  const int n = 2000;
  std::vector<std::vector<std::pair<int, float>>> adj(n);
  for (int e = 0; e < 7000; e++) {
    const int a = (int)(rng() % n), b = (int)(rng() % n);
    bool dup = a == b;
    for (auto &x : adj[a]) dup |= x.first == b;
    if (dup) continue;
    const float w = (float)((int)(rng() % 2000001) - 1000000) / 1024.0f;
    adj[a].push_back({b, w});
    adj[b].push_back({a, w});
  }
  std::ostringstream text;
  size_t entries = 0;
  for (auto &a : adj) entries += a.size();
  text << "% generated\n" << n << " " << entries / 2 << " 1\n";
  char buf[64];
  for (auto &a : adj) {
    for (auto &x : a) {
      std::snprintf(buf, sizeof buf, "%d %.9g ", x.first + 1, (double)x.second);
      text << buf;
    }
    text << "\n";
  }
  const std::string in = write_file("rt_in.graph", text.str()), out = path_of("rt_out.graph");
  context::HIPContext &gpu = *hip_context;
  std::unique_ptr<object::Graph<int, int, float>> g(io::MetisGraphReader<int, int, float>(in, true).ReadHIPGraph(gpu));
  auto *coo = g->get_connectivity()->AsAbsolute<format::HIPCOO<int, int, float>>();
  EXPECT_EQ((size_t)coo->get_num_nnz(), entries);
  std::unique_ptr<format::HIPCSR<int, int, float>> csr(coo->Convert<format::HIPCSR>(&gpu));
  std::unique_ptr<format::HIPArray<int>> order(bases::ReorderBase::Reorder<reorder::RCMReorder>({}, csr.get(), gpu));
  std::unique_ptr<format::HIPCSR<int, int, float>> permuted(
      bases::ReorderBase::Permute2D<format::HIPCSR>(order.get(), csr.get(), {&gpu}, true));
  object::Graph<int, int, float> pg(permuted->Convert<format::HIPCOO>(&gpu));
  io::MetisGraphWriter<int, int, float>(out, true, false, true, 9).WriteGraph(&pg);
  // chunks of 100 items (about 12 rows each, rows of up to 20 entries among them) leave the same file
  const std::string whole = slurp(out);
  g_chunk_entries = 100;
  io::MetisGraphWriter<int, int, float>(out, true, false, true, 9).WriteGraph(&pg);
  g_chunk_entries = 1 << 24;
  EXPECT_TRUE(!whole.empty() && slurp(out) == whole);
  context::CPUContext cpu;
  std::unique_ptr<format::COO<int, int, float>> want(
      pg.get_connectivity()->AsAbsolute<format::HIPCOO<int, int, float>>()->Convert<format::COO>(&cpu));
  for (bool zero : {true, false}) {
    std::unique_ptr<object::Graph<int, int, float>> back(io::MetisGraphReader<int, int, float>(out, zero).ReadGraph());
    auto *b = back->get_connectivity()->AsAbsolute<format::COO<int, int, float>>();
    EXPECT_EQ((int)b->get_dimensions()[0], n + (zero ? 0 : 1));
    EXPECT_EQ((size_t)b->get_num_nnz(), entries);
    if ((size_t)b->get_num_nnz() != entries) continue;
    bool same = same_bits(b->get_vals(), want->get_vals(), entries);
    for (size_t i = 0; i < entries; i++)
      same &= b->get_row()[i] == want->get_row()[i] + (zero ? 0 : 1) && b->get_col()[i] == want->get_col()[i] + (zero ? 0 : 1);
    EXPECT_TRUE(same);
  }
}

int main(int argc, char **argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  g_fixtures = argc > 2 ? argv[2] : "tests/golden";
  hip_context.reset(new context::HIPContext(hip::DefaultDevice()));
  return minitest::run_all(argc > 3 ? argv[3] : nullptr);
}
