// sparsebase/io/patoh_reader.h — PaToH hypergraph reader (reference: io/patoh_reader.h, io/patoh_reader.cc:11-242).  The
// header line is parsed here, as the reference parses it: leading lines that begin with '%' are skipped, then
// `base cells nets pins [scheme [constraints]]`, every token through stoi; scheme defaults to 0 (bit 0: the cells are
// weighted, bit 1: the nets are), constraints to 1.  Everything behind it goes to the GPU as it is: sbhg_patoh_parse
// (include/sbhg.h) finds lines and tokens, gives every token its role, and builds the cells x nets side by a stable sort
// of the pin positions where the reference runs two nested loops over cells x pins.  ReadHyperGraph's connectivity and
// xNetCSR_ are host CSRs, as in the reference; ReadHIPHyperGraph's connectivity is a HIPCSR that stays on the device,
// with the cells x nets side in xNetHIPCSR_.  The weights are host Arrays in both (absent for a void ValueType), and all
// of it is owned by the HyperGraph.
//
// The reference's quirk is kept: the cell weights are the file's last line, and only if the file does not end in '\n'.
//
// Deliberate divergences, each a place where the reference has undefined behaviour: another number of net lines than
// the header's nets (where a weighted file that ends in '\n' ends up), another number of pins, more cell weights than
// cells, a pin outside [base, cells + base), a token that is no complete decimal integer, a net line without a weight in
// a net-weighted file, a header without its four counts, base outside {0, 1}, scheme outside 0..3, a text of 2^32 bytes
// and more: ReaderException.  A void ValueType skips the weight tokens (the reference takes them for pins).
#ifndef SPARSEBASE_IO_PATOH_READER_H_
#define SPARSEBASE_IO_PATOH_READER_H_
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "sbhg.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/object/object.h"
#include "sparsebase/utils/exception.h"

namespace sparsebase::io {

template <typename IDType, typename NNZType, typename ValueType>
class ReadsHyperGraph {
 public:
  virtual ~ReadsHyperGraph() = default;
  virtual object::HyperGraph<IDType, NNZType, ValueType> *ReadHyperGraph() const = 0;
};

namespace detail {
struct PatohHeader {
  long long base = 0, cells = 0, nets = 0, pins = 0, scheme = 0, constraints = 1;
  size_t body = 0;  // offset of the byte behind the header line
};
// patoh_reader.cc:11-43
inline PatohHeader ParsePatohHeader(const std::string &text) {
  size_t pos = 0;
  while (pos < text.size() && text[pos] == '%') {
    const size_t end = text.find('\n', pos);
    pos = end == std::string::npos ? text.size() : end + 1;
  }
  if (pos >= text.size()) throw utils::ReaderException("patoh: no header line");
  const size_t end = text.find('\n', pos);
  const size_t stop = end == std::string::npos ? text.size() : end;
  std::istringstream iss(text.substr(pos, stop - pos));
  std::string tok[6];
  for (auto &t : tok) iss >> t;
  auto to_int = [](const std::string &t, const char *what) {  // std::stoi: the longest integer prefix, or it throws
    try {
      return (long long)std::stoll(t);
    } catch (std::exception &) {
      throw utils::ReaderException(std::string("patoh: the header line does not give ") + what);
    }
  };
  PatohHeader h;
  h.body = end == std::string::npos ? text.size() : end + 1;
  h.base = to_int(tok[0], "the base");
  h.cells = to_int(tok[1], "the number of cells");
  h.nets = to_int(tok[2], "the number of nets");
  h.pins = to_int(tok[3], "the number of pins");
  if (!tok[4].empty()) h.scheme = to_int(tok[4], "the scheme");
  if (!tok[5].empty()) h.constraints = to_int(tok[5], "the constraints");
  if (h.base != 0 && h.base != 1) throw utils::ReaderException("patoh: base " + std::to_string(h.base) + ": 0 or 1");
  if (h.cells < 0 || h.nets < 0 || h.pins < 0) throw utils::ReaderException("patoh: a negative count in the header line");
  if (h.scheme < 0 || h.scheme > 3) throw utils::ReaderException("patoh: scheme " + std::to_string(h.scheme) + ": 0..3");
  return h;
}
}  // namespace detail

template <typename IDType, typename NNZType, typename ValueType>
class PatohReader : public ReadsHyperGraph<IDType, NNZType, ValueType> {
 public:
  using HyperGraphT = object::HyperGraph<IDType, NNZType, ValueType>;
  explicit PatohReader(std::string filename) : filename_(std::move(filename)) {}

  HyperGraphT *ReadHyperGraph() const override {
    std::unique_ptr<HyperGraphT> g(ReadHIPHyperGraph(context::HIPContext(hip::DefaultDevice())));
    auto *con = g->get_connectivity()->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
    auto &dev = con->device();
    const auto dims = con->get_dimensions();
    const size_t nets = dims[0], cells = dims[1], pins = con->get_num_nnz();
    auto to_host = [&](format::HIPCSR<IDType, NNZType, ValueType> *d, size_t rows, size_t cols) {
      std::unique_ptr<NNZType[]> rp(new NNZType[rows + 1]);
      std::unique_ptr<IDType[]> col(new IDType[pins + 1]);
      dev.ToHost(rp.get(), d->get_row_ptr(), (rows + 1) * sizeof(NNZType));
      if (pins) dev.ToHost(col.get(), d->get_col(), pins * sizeof(IDType));
      // (the pins are in file order: no sort, as in the reference)
      auto *h = new format::CSR<IDType, NNZType, ValueType>((IDType)rows, (IDType)cols, rp.get(), col.get(), nullptr,
                                                            format::kOwned, true);
      rp.release();
      col.release();
      return h;
    };
    auto *xnet = to_host(g->xNetHIPCSR_, cells, nets);
    delete g->xNetHIPCSR_;
    g->xNetHIPCSR_ = nullptr;
    g->xNetCSR_ = xnet;
    g->set_connectivity(to_host(con, nets, cells), true);  // (the device CSR is released here)
    return g.release();
  }

  HyperGraphT *ReadHIPHyperGraph(context::HIPContext ctx) const {
    std::ifstream fin(filename_, std::ios::binary);
    if (!fin.is_open()) throw utils::ReaderException("Can not read HyperGraph\n");  // (patoh_reader.cc:22)
    const std::string text((std::istreambuf_iterator<char>(fin)), std::istreambuf_iterator<char>());
    const detail::PatohHeader hd = detail::ParsePatohHeader(text);
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    const size_t bytes = text.size() - hd.body, nets = (size_t)hd.nets, cells = (size_t)hd.cells, pins = (size_t)hd.pins;
    auto &dev = hip::Device::Get(ctx.device_id);
    hip::Staged<char> d_text(dev, text.data() + hd.body, bytes + 1);
    NNZType *xpin = (NNZType *)dev.Malloc((nets + 1) * sizeof(NNZType)), *xnet = (NNZType *)dev.Malloc((cells + 1) * sizeof(NNZType));
    IDType *pin = (IDType *)dev.Malloc((pins + 1) * sizeof(IDType)), *net = (IDType *)dev.Malloc((pins + 1) * sizeof(IDType));
    void *nw = vb ? dev.Malloc((nets + 1) * vb) : nullptr, *cw = vb ? dev.Malloc((cells + 1) * vb) : nullptr;
    auto release = [&] { dev.Free(xpin), dev.Free(xnet), dev.Free(pin), dev.Free(net), dev.Free(nw), dev.Free(cw); };
    int64_t counts[3] = {0, 0, 0};
    const int rc = sbhg_patoh_parse(dev.handle(), hip::IndexTag<IDType, NNZType>(), hip::ValueTag<ValueType>(), d_text.get(),
                                    (int64_t)bytes, hd.cells, hd.nets, hd.pins, (int)hd.base, (int)hd.scheme, (int64_t)pins + 1,
                                    xpin, pin, xnet, net, nw, cw, counts);
    if (rc != SBX_OK) {
      release();
      throw utils::ReaderException(std::string("patoh: ") + sbx_last_error(dev.handle()));
    }
    std::vector<char> h_nw(nets * vb), h_cw(cells * vb);
    try {
      if (vb && nets) dev.ToHost(h_nw.data(), nw, nets * vb);
      if (vb && cells) dev.ToHost(h_cw.data(), cw, cells * vb);
    } catch (...) {
      release();
      throw;
    }
    dev.Free(nw), dev.Free(cw);
    // (pins in file order: the constructors' sort is skipped, as the reference skips it)
    auto *con = new format::HIPCSR<IDType, NNZType, ValueType>((IDType)nets, (IDType)cells, (NNZType)pins, xpin, pin, nullptr, ctx,
                                                               format::kOwned, true);
    auto *xn = new format::HIPCSR<IDType, NNZType, ValueType>((IDType)cells, (IDType)nets, (NNZType)pins, xnet, net, nullptr, ctx,
                                                              format::kOwned, true);
    HyperGraphT *g = nullptr;
    if constexpr (std::is_same_v<ValueType, void>) {
      g = new HyperGraphT(con, (IDType)hd.base, (IDType)hd.constraints, nullptr);
    } else {
      auto host_array = [](const std::vector<char> &src, size_t count) {
        ValueType *v = new ValueType[count ? count : 1];
        if (count) std::memcpy(v, src.data(), count * sizeof(ValueType));
        return new format::Array<ValueType>((format::DimensionType)count, v, format::kOwned);
      };
      g = new HyperGraphT(con, host_array(h_nw, nets), host_array(h_cw, cells), (IDType)hd.base, (IDType)hd.constraints,
                          nullptr);
    }
    g->xNetHIPCSR_ = xn;
    g->OwnParts();
    return g;
  }

 private:
  std::string filename_;
};

}  // namespace sparsebase::io
#endif
