// Host-layer tests of io::PatohReader, io::PatohWriter and object::HyperGraph: the reference's reader tests
// (tests/suites/sparsebase/io/patoh_reader_tests.cc) over the four files they write (kept as fixtures:
// tests/golden/patoh_*.hypeg), compared with a plain getline reader; the bytes the writer leaves for every flag and base
// combination, for host and device hypergraphs and for every chunk size; the refusals; a round trip write -> read of a
// random hypergraph for three type tuples.
// Usage: test_patoh <scratch dir> <fixture dir> [filter].  Needs a GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

// the chunk size is a compile-time macro of io/writer.h; defined to an expression here, the writer can be run with the
// default and with chunks of a few items (as test_metis_graph.cc does)
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

// What a well-formed file says, read the plain way: getline, `>> int`, the last line the cell weights iff the cells are
// weighted and getline hit the end of the file; the cell -> net side by the definition (row c: the nets of the pins equal
// to c + base, in pin order).
struct Plain {
  int base = 0, cells = 0, nets = 0, pins = 0, scheme = 0, constraints = 1;
  std::vector<int> xpin, pin, xnet, net, nw, cw;
};
static Plain plain_read(const std::string &path) {
  std::ifstream f(path);
  std::string line;
  while (f.peek() == '%') std::getline(f, line);
  std::getline(f, line);
  Plain p;
  std::istringstream head(line);
  head >> p.base >> p.cells >> p.nets >> p.pins;
  if (!(head >> p.scheme)) p.scheme = 0;
  else if (!(head >> p.constraints)) p.constraints = 1;
  p.nw.assign(p.nets, 1);
  p.cw.assign(p.cells, 1);
  p.xpin.push_back(0);
  while (std::getline(f, line)) {
    if (!line.empty() && line[0] == '%') continue;
    std::istringstream iss(line);
    int v;
    if ((p.scheme & 1) && f.eof()) {
      for (size_t i = 0; iss >> v; i++) p.cw[i] = v;
      continue;
    }
    if (p.scheme & 2) {
      iss >> v;
      p.nw[p.xpin.size() - 1] = v;
    }
    while (iss >> v) p.pin.push_back(v);
    p.xpin.push_back((int)p.pin.size());
  }
  p.xnet.push_back(0);
  for (int c = 0; c < p.cells; c++) {
    for (size_t i = 0; i < p.pin.size(); i++)
      if (p.pin[i] == c + p.base) {
        const int j = (int)(std::upper_bound(p.xpin.begin(), p.xpin.end(), (int)i) - p.xpin.begin()) - 1;
        p.net.push_back(j + p.base);
      }
    p.xnet.push_back((int)p.net.size());
  }
  return p;
}

template <typename T, typename U>
static bool same_values(const T *a, const std::vector<U> &b) {
  for (size_t i = 0; i < b.size(); i++)
    if (!(a[i] == (T)b[i])) return false;
  return true;
}

// patoh_reader_tests.cc, one file
template <typename I, typename N, typename V>
static void check_read(const std::string &file) {
  const Plain p = plain_read(file);
  std::unique_ptr<object::HyperGraph<I, N, V>> g(io::PatohReader<I, N, V>(file).ReadHyperGraph());
  auto *con = g->get_connectivity()->template AsAbsolute<format::CSR<I, N, V>>();
  EXPECT_EQ((int)g->n_, p.nets);
  EXPECT_EQ((int)g->m_, p.pins);
  EXPECT_EQ((int)con->get_dimensions()[1], p.cells);
  EXPECT_EQ((int)g->constraint_num_, p.constraints);
  EXPECT_EQ((int)g->base_type_, p.base);
  EXPECT_NE(con->get_row_ptr(), nullptr);
  EXPECT_NE(con->get_col(), nullptr);
  EXPECT_TRUE(g->xNetCSR_ != nullptr && g->xNetHIPCSR_ == nullptr);
  EXPECT_TRUE(con->get_vals() == nullptr && g->xNetCSR_->get_vals() == nullptr);
  EXPECT_TRUE(g->PartsAreOwned());
  if ((int)g->n_ != p.nets || (int)g->m_ != p.pins || !g->xNetCSR_) return;
  EXPECT_TRUE(same_values(con->get_row_ptr(), p.xpin) && same_values(con->get_col(), p.pin));
  EXPECT_TRUE(same_values(g->xNetCSR_->get_row_ptr(), p.xnet) && same_values(g->xNetCSR_->get_col(), p.net));
  EXPECT_EQ((int)g->xNetCSR_->get_dimensions()[0], p.cells);
  EXPECT_EQ((int)g->xNetCSR_->get_dimensions()[1], p.nets);
  if constexpr (!std::is_same_v<V, void>) {
    EXPECT_TRUE(g->netWeights_ != nullptr && g->cellWeights_ != nullptr);
    if (!g->netWeights_ || !g->cellWeights_) return;
    EXPECT_EQ((int)g->netWeights_->get_dimensions()[0], p.nets);
    EXPECT_EQ((int)g->cellWeights_->get_dimensions()[0], p.cells);
    EXPECT_TRUE(same_values(g->netWeights_->get_vals(), p.nw) && same_values(g->cellWeights_->get_vals(), p.cw));
  } else {
    EXPECT_TRUE(g->netWeights_ == nullptr && g->cellWeights_ == nullptr);
  }
}

static const char *const kFixtures[4] = {"patoh_unweighted.hypeg", "patoh_net_weights.hypeg", "patoh_cell_weights.hypeg",
                                         "patoh_both_weights.hypeg"};

TEST(PatohReader, ReadHyperGraph) {
  for (const char *name : kFixtures) {
    const std::string f = g_fixtures + "/" + name;
    check_read<int, int, int>(f);
    check_read<int, int, float>(f);
    check_read<long long, long long, double>(f);
    check_read<int, long long, int>(f);
  }
  check_read<int, int, void>(g_fixtures + "/" + kFixtures[0]);
  // the example of include/sbhg.h's description
  const std::string f = write_file("example.hypeg", "1 5 3 7 3\n4 1 2 3\n% c\n6 3 4\n9 5 1\n1 2 3 4 5");
  check_read<int, int, int>(f);
  std::unique_ptr<object::HyperGraph<int, int, int>> g(io::PatohReader<int, int, int>(f).ReadHyperGraph());
  EXPECT_TRUE(same_values(g->xNetCSR_->get_row_ptr(), std::vector<int>{0, 2, 3, 5, 6, 7}));
  EXPECT_TRUE(same_values(g->xNetCSR_->get_col(), std::vector<int>{1, 3, 1, 1, 2, 2, 3}));
  EXPECT_TRUE(same_values(g->netWeights_->get_vals(), std::vector<int>{4, 6, 9}));
  // a void ValueType skips the weights instead of taking them for pins
  std::unique_ptr<object::HyperGraph<int, int, void>> gv(io::PatohReader<int, int, void>(f).ReadHyperGraph());
  EXPECT_TRUE(same_values(gv->get_connectivity()->AsAbsolute<format::CSR<int, int, void>>()->get_col(),
                          std::vector<int>{1, 2, 3, 3, 4, 5, 1}));
  // through the interface
  const io::PatohReader<int, int, int> reader(f);
  const io::ReadsHyperGraph<int, int, int> &iface = reader;
  std::unique_ptr<object::HyperGraph<int, int, int>> gi(iface.ReadHyperGraph());
  EXPECT_EQ((int)gi->m_, 7);
}

TEST(PatohReader, ReadHIPHyperGraph) {
  const std::string f = g_fixtures + "/" + kFixtures[3];
  const Plain p = plain_read(f);
  std::unique_ptr<object::HyperGraph<long long, long long, float>> d(
      io::PatohReader<long long, long long, float>(f).ReadHIPHyperGraph(*hip_context));
  auto *con = d->get_connectivity()->AsAbsolute<format::HIPCSR<long long, long long, float>>();
  EXPECT_TRUE(d->xNetCSR_ == nullptr && d->xNetHIPCSR_ != nullptr);
  EXPECT_EQ((int)d->n_, p.nets);
  EXPECT_EQ((int)d->m_, p.pins);
  auto &dev = hip::Device::Get(hip_context->device_id);
  std::vector<long long> pin(p.pins), net(p.pins), xnet(p.cells + 1);
  dev.ToHost(pin.data(), con->get_col(), pin.size() * sizeof(long long));
  dev.ToHost(net.data(), d->xNetHIPCSR_->get_col(), net.size() * sizeof(long long));
  dev.ToHost(xnet.data(), d->xNetHIPCSR_->get_row_ptr(), xnet.size() * sizeof(long long));
  EXPECT_TRUE(same_values(pin.data(), p.pin) && same_values(net.data(), p.net) && same_values(xnet.data(), p.xnet));
  EXPECT_TRUE(same_values(d->netWeights_->get_vals(), p.nw) && same_values(d->cellWeights_->get_vals(), p.cw));
}

TEST(PatohWriter, TheBytes) {
  const std::string in = "1 5 3 7 3\n4 1 2 3\n% c\n6 3 4\n9 5 1\n1 2 3 4 5";
  const std::string f = write_file("bytes_in.hypeg", in), out = path_of("bytes_out.hypeg");
  std::unique_ptr<object::HyperGraph<int, int, int>> g(io::PatohReader<int, int, int>(f).ReadHyperGraph());
  auto *con = g->get_connectivity()->AsAbsolute<format::CSR<int, int, int>>();
  const std::vector<int> pins_before(con->get_col(), con->get_col() + 7), nets_before(g->xNetCSR_->get_col(), g->xNetCSR_->get_col() + 7);
  const std::string both1 = "1 5 3 7 3\n4 1 2 3\n6 3 4\n9 5 1\n1 2 3 4 5", both0 = "0 5 3 7 3\n4 0 1 2\n6 2 3\n9 4 0\n1 2 3 4 5";
  for (long chunk : {1L << 24, 5L, 1L}) {
    g_chunk_entries = chunk;
    io::PatohWriter<int, int, int>(out, false, true, true).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), both1);
    io::PatohWriter<int, int, int>(out, true, true, true).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), both0);
    io::PatohWriter<int, int, int>(out, false, false, false).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), std::string("1 5 3 7\n1 2 3\n3 4\n5 1"));
    io::PatohWriter<int, int, int>(out, true, true, false).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), std::string("0 5 3 7 2\n4 0 1 2\n6 2 3\n9 4 0"));
    io::PatohWriter<int, int, int>(out, true, false, true).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), std::string("0 5 3 7 1\n0 1 2\n2 3\n4 0\n1 2 3 4 5"));
  }
  g_chunk_entries = 1 << 24;
  // the hypergraph is left as it was (the reference rewrites its arrays when the base changes)
  EXPECT_TRUE(same_values(con->get_col(), pins_before) && same_values(g->xNetCSR_->get_col(), nets_before));
  // constraints: behind schemes 1 and 2 when not 1, never behind 3
  g->constraint_num_ = 2;
  io::PatohWriter<int, int, int>(out, true, true, false, 2).WriteHyperGraph(g.get());
  EXPECT_EQ(slurp(out).substr(0, 14), std::string("0 5 3 7 2 2\n4 "));
  io::PatohWriter<int, int, int>(out, true, false, true, 2).WriteHyperGraph(g.get());
  EXPECT_EQ(slurp(out).substr(0, 12), std::string("0 5 3 7 1 2\n"));
  io::PatohWriter<int, int, int>(out, true, true, true, 2).WriteHyperGraph(g.get());
  EXPECT_EQ(slurp(out), both0);
  io::PatohWriter<int, int, int>(out, true, false, false, 2).WriteHyperGraph(g.get());
  EXPECT_EQ(slurp(out).substr(0, 8), std::string("0 5 3 7\n"));
  g->constraint_num_ = 1;
  // the connectivity on the device gives the same file; so does the interface; float weights print as the stream does
  std::unique_ptr<object::HyperGraph<int, int, float>> gd(io::PatohReader<int, int, float>(f).ReadHIPHyperGraph(*hip_context));
  const io::PatohWriter<int, int, float> wf(out, false, true, true);
  const io::WritesHyperGraph<int, int, float> &iface = wf;
  iface.WriteHyperGraph(gd.get());
  EXPECT_EQ(slurp(out), both1);
  gd->netWeights_->get_vals()[1] = 2.5f;
  io::PatohWriter<int, int, float>(out, true, true, false).WriteHyperGraph(gd.get());
  EXPECT_EQ(slurp(out), std::string("0 5 3 7 2\n4 0 1 2\n2.5 2 3\n9 4 0"));
  EXPECT_THROW((delete io::PatohReader<int, int, float>(out).ReadHyperGraph()), utils::ReaderException);  // 2.5 is no integer
  // a void ValueType ignores both flags
  std::unique_ptr<object::HyperGraph<int, int, void>> gv(io::PatohReader<int, int, void>(f).ReadHyperGraph());
  io::PatohWriter<int, int, void>(out, true, true, true).WriteHyperGraph(gv.get());
  EXPECT_EQ(slurp(out), std::string("0 5 3 7\n0 1 2\n2 3\n4 0"));
}

TEST(PatohWriter, EmptyNets) {
  // empty nets first, in the middle and last: the last line, being empty, keeps its '\n'
  const std::string in = "0 4 5 4\n\n0 1\n\n2 3\n\n";
  const std::string f = write_file("empty_in.hypeg", in), out = path_of("empty_out.hypeg");
  std::unique_ptr<object::HyperGraph<int, int, int>> g(io::PatohReader<int, int, int>(f).ReadHyperGraph());
  EXPECT_EQ((int)g->n_, 5);
  for (long chunk : {1L << 24, 2L}) {
    g_chunk_entries = chunk;
    io::PatohWriter<int, int, int>(out, true, false, false).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), in);
    io::PatohWriter<int, int, int>(out, true, true, false).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), std::string("0 4 5 4 2\n1\n1 0 1\n1\n1 2 3\n1"));
    io::PatohWriter<int, int, int>(out, false, false, true).WriteHyperGraph(g.get());
    EXPECT_EQ(slurp(out), std::string("1 4 5 4 1\n\n1 2\n\n3 4\n\n1 1 1 1"));
    std::unique_ptr<object::HyperGraph<int, int, int>> back(io::PatohReader<int, int, int>(out).ReadHyperGraph());
    EXPECT_EQ((int)back->n_, 5);
  }
  g_chunk_entries = 1 << 24;
}

TEST(Patoh, Refusals) {
  EXPECT_THROW((delete io::PatohReader<int, int, int>(path_of("no_such.hypeg")).ReadHyperGraph()), utils::ReaderException);
  const std::string nl = write_file("newline.hypeg", "1 4 2 4 1\n1 2\n3 4\n7 7 7 7\n");
  std::string msg;
  try {
    delete io::PatohReader<int, int, int>(nl).ReadHyperGraph();
  } catch (utils::Exception &e) {
    msg = e.what();
  }
  EXPECT_TRUE(msg.find("3 net lines") != std::string::npos && msg.find("nets is 2") != std::string::npos);
  for (const char *text : {"", "% only\n", "1 4 2\n1 2\n", "2 4 1 2\n1 2\n", "1 4 1 2 4\n1 2\n", "1 4 2 4\n1 2\n3 5\n", "1 4 2 4\n1 2\n3 4x\n",
                           "1 4 2 5\n1 2\n3 4\n", "1 4 2 4 1\n1 2\n3 4\n1 2 3 4 5", "1 4 2 3 2\n5 1 2\n\n"}) {
    const std::string p = write_file("bad.hypeg", text);
    EXPECT_THROW((delete io::PatohReader<int, int, int>(p).ReadHyperGraph()), utils::ReaderException);
  }
  // the writer's: before the file is opened
  const std::string f = write_file("plain.hypeg", "0 3 1 2\n0 2\n");
  std::unique_ptr<object::HyperGraph<int, int, float>> g(io::PatohReader<int, int, float>(f).ReadHyperGraph());
  const std::string out = path_of("refused.hypeg");
  EXPECT_THROW((io::PatohWriter<int, int, float>(out, true, false, false, 1, 18).WriteHyperGraph(g.get())), utils::WriterException);
  format::Array<float> *nw = g->netWeights_;
  g->netWeights_ = nullptr;
  EXPECT_THROW((io::PatohWriter<int, int, float>(out, true, true, false).WriteHyperGraph(g.get())), utils::WriterException);
  g->netWeights_ = nw;
  EXPECT_FALSE(exists(out));
}

TEST(HyperGraph, ConstructorsAndOwnership) {
  int xpin[3] = {0, 2, 3}, pin[3] = {0, 1, 1}, xnet[3] = {0, 1, 3}, net[3] = {0, 0, 1}, nwv[2] = {5, 6}, cwv[2] = {7, 8};
  format::CSR<int, int, int> xn(2, 2, xnet, net, nullptr, format::kNotOwned, true);
  format::Array<int> nw(2, nwv), cw(2, cwv);
  {
    object::HyperGraph<int, int, int> a(new format::CSR<int, int, int>(2, 2, xpin, pin, nullptr, format::kNotOwned, true), 0, 1, &xn);
    EXPECT_TRUE(a.n_ == 2 && a.m_ == 3 && a.base_type_ == 0 && a.constraint_num_ == 1 && a.xNetCSR_ == &xn);
    EXPECT_TRUE(a.netWeights_ == nullptr && a.cellWeights_ == nullptr && !a.PartsAreOwned());
    object::HyperGraph<int, int, int> b(new format::CSR<int, int, int>(2, 2, xpin, pin, nullptr, format::kNotOwned, true), &nw, &cw,
                                        1, 3, &xn);
    EXPECT_TRUE(b.netWeights_ == &nw && b.cellWeights_ == &cw && b.base_type_ == 1 && b.constraint_num_ == 3);
    const std::string out = path_of("built.hypeg");
    io::PatohWriter<int, int, int>(out, false, true, true).WriteHyperGraph(&b);  // stored in base 1, written in base 1
    EXPECT_EQ(slurp(out), std::string("1 2 2 3 3\n5 0 1\n6 1\n7 8"));
  }  // (the callers' parts are not freed: they live on this stack)
  EXPECT_EQ(nw.get_vals()[1], 6);
}

// a random hypergraph out and in again, for three type tuples, host and device, several chunk sizes
template <typename I, typename N, typename V>
static void round_trip(unsigned seed, bool zero, bool ew, bool vw) {
  std::mt19937 rng(seed);
  const int nets = 3000, cells = 1777, base = (int)(seed & 1);
  std::ostringstream text;
  std::vector<std::vector<int>> lines(nets);
  size_t pins = 0;
  for (auto &l : lines) {
    l.resize(rng() % 9);
    for (auto &c : l) c = (int)(rng() % cells) + base;
    pins += l.size();
  }
  lines[1500].resize(4000);  // one long net
  for (auto &c : lines[1500]) c = (int)(rng() % cells) + base;
  pins = 0;
  for (auto &l : lines) pins += l.size();
  text << "% generated\n" << base << " " << cells << " " << nets << " " << pins << " 3\n";
  for (auto &l : lines) {
    text << (rng() % 1000 + 1);
    for (int c : l) text << " " << c;
    text << "\n";
  }
  for (int c = 0; c < cells; c++) text << (c ? " " : "") << (rng() % 50 + 1);
  const std::string in = write_file("rt_in.hypeg", text.str()), out = path_of("rt_out.hypeg");
  std::unique_ptr<object::HyperGraph<I, N, V>> g(io::PatohReader<I, N, V>(in).ReadHIPHyperGraph(*hip_context));
  io::PatohWriter<I, N, V>(out, zero, ew, vw).WriteHyperGraph(g.get());
  const std::string whole = slurp(out);
  g_chunk_entries = 700;
  io::PatohWriter<I, N, V>(out, zero, ew, vw).WriteHyperGraph(g.get());
  g_chunk_entries = 1 << 24;
  EXPECT_TRUE(!whole.empty() && slurp(out) == whole);
  std::unique_ptr<object::HyperGraph<I, N, V>> a(io::PatohReader<I, N, V>(in).ReadHyperGraph());
  std::unique_ptr<object::HyperGraph<I, N, V>> b(io::PatohReader<I, N, V>(out).ReadHyperGraph());
  auto *ca = a->get_connectivity()->template AsAbsolute<format::CSR<I, N, V>>();
  auto *cb = b->get_connectivity()->template AsAbsolute<format::CSR<I, N, V>>();
  EXPECT_TRUE(a->n_ == b->n_ && a->m_ == b->m_ && (size_t)a->m_ == pins);
  EXPECT_EQ((int)b->base_type_, zero ? 0 : 1);
  if (a->m_ != b->m_ || a->n_ != b->n_) return;
  const I delta = (I)((zero ? 0 : 1) - base);
  bool same = std::memcmp(ca->get_row_ptr(), cb->get_row_ptr(), ((size_t)nets + 1) * sizeof(N)) == 0 &&
              std::memcmp(a->xNetCSR_->get_row_ptr(), b->xNetCSR_->get_row_ptr(), ((size_t)cells + 1) * sizeof(N)) == 0;
  for (size_t i = 0; i < pins; i++)
    same &= cb->get_col()[i] == ca->get_col()[i] + delta && b->xNetCSR_->get_col()[i] == a->xNetCSR_->get_col()[i] + delta;
  if constexpr (!std::is_same_v<V, void>) {
    for (int j = 0; j < nets; j++) same &= b->netWeights_->get_vals()[j] == (ew ? a->netWeights_->get_vals()[j] : V(1));
    for (int c = 0; c < cells; c++) same &= b->cellWeights_->get_vals()[c] == (vw ? a->cellWeights_->get_vals()[c] : V(1));
  }
  EXPECT_TRUE(same);
}

TEST(Patoh, WriteReadRoundTrip) {
  round_trip<int, int, int>(1, true, true, true);
  round_trip<int, int, int>(2, false, false, false);
  round_trip<long long, long long, double>(3, false, true, false);
  round_trip<int, long long, float>(4, true, false, true);
  round_trip<int, int, void>(5, false, true, true);
}

int main(int argc, char **argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  g_fixtures = argc > 2 ? argv[2] : "tests/golden";
  hip_context.reset(new context::HIPContext(hip::DefaultDevice()));
  return minitest::run_all(argc > 3 ? argv[3] : nullptr);
}
