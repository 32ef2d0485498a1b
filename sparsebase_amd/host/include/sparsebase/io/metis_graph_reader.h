// sparsebase/io/metis_graph_reader.h — METIS graph reader (reference: io/metis_graph_reader.h:24-39,
// io/metis_graph_reader.cc:9-106).  The header line is parsed here, as the reference parses it (`n m [FMT [NCON]]` read
// with `>>`, FMT as an int: `011` is 11; FMT 1 / 11 without NCON has NCON 1; edge weights iff FMT is 1 or 11, vertex
// weights iff FMT >= 10 and NCON > 0, so `10` alone reads none).  Everything behind it goes to the GPU as it is:
// sbgr_metis_parse (include/sbgr.h) finds lines and tokens, gives every token its role and parses it exactly, and
// leaves the entries in (row, col) order.  ReadGraph's connectivity is a host COO, as in the reference;
// ReadHIPGraph's is a HIPCOO that stays on the device.  Vertex weights are on the host in both, one Array per row, and
// owned by the Graph.  Graph::ncon_ is the NCON so derived for non-void value types, even where no weights are read;
// for void it is 0 and vertexWeights_ is null.
//
// Deliberate divergences, each a place where the reference has undefined behaviour:
//   - the lines hold another number of neighbours than 2 * m (the reference leaves the tail of its arrays uninitialised
//     or writes past them): ReaderException naming both counts — this is what a `10`-without-NCON file with weights gets;
//   - more vertex lines than n, an id outside the graph, a malformed token (the reference drops the rest of the line), an
//     edge-weighted line with a neighbour without weight, FMT outside {0, 1, 10, 11}, an empty line or no line before
//     the header, a header without n and m, a text of 2^32 bytes and more: ReaderException;
//   - a vertex-weighted file with fewer lines than n: the missing rows have zero weights (the reference leaves the
//     pointers uninitialised);
//   - neighbours given twice with different weights come in file order (std::sort leaves it open).
#ifndef SPARSEBASE_IO_METIS_GRAPH_READER_H_
#define SPARSEBASE_IO_METIS_GRAPH_READER_H_
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "sbgr.h"
#include "sparsebase/converter/converter_order_two.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/object/object.h"
#include "sparsebase/utils/exception.h"

namespace sparsebase::io {

namespace detail {
struct MetisHeader {
  long long n = 0, m = 0;
  int fmt = 0, ncon = 0;
  size_t body = 0;  // offset of the byte behind the header line
};
// metis_graph_reader.cc:26-39
inline MetisHeader ParseMetisHeader(const std::string &text) {
  size_t pos = 0;
  while (pos < text.size()) {
    const size_t end = text.find('\n', pos);
    const size_t stop = end == std::string::npos ? text.size() : end;
    const size_t next = end == std::string::npos ? text.size() : end + 1;
    if (stop == pos) throw utils::ReaderException("metis graph: an empty line before the header line");
    if (text[pos] != '%') {
      std::istringstream iss(text.substr(pos, stop - pos));
      MetisHeader h;
      h.body = next;
      if (!(iss >> h.n >> h.m) || h.n < 0 || h.m < 0) throw utils::ReaderException("metis graph: the header line does not give n and m");
      if (iss >> h.fmt) {
      }
      if (iss >> h.ncon) {
      }
      if ((h.fmt == 1 || h.fmt == 11) && h.ncon == 0) h.ncon = 1;
      if (h.fmt != 0 && h.fmt != 1 && h.fmt != 10 && h.fmt != 11)
        throw utils::ReaderException("metis graph: FMT " + std::to_string(h.fmt) + " (vertex sizes) is not supported");
      if (h.ncon < 0) throw utils::ReaderException("metis graph: NCON is negative");
      return h;
    }
    pos = next;
  }
  throw utils::ReaderException("metis graph: no header line");
}
}  // namespace detail

template <typename IDType, typename NNZType, typename ValueType>
class MetisGraphReader {
 public:
  explicit MetisGraphReader(std::string filename, bool convert_to_zero_index = false)
      : filename_(std::move(filename)), convert_to_zero_index_(convert_to_zero_index) {}

  object::Graph<IDType, NNZType, ValueType> *ReadGraph() const {
    std::unique_ptr<object::Graph<IDType, NNZType, ValueType>> g(ReadHIPGraph(context::HIPContext(hip::DefaultDevice())));
    context::CPUContext cpu;
    format::Format *coo = converter::HIPCooCooConditionalFunction<IDType, NNZType, ValueType>(g->get_connectivity(), &cpu);
    g->set_connectivity(coo, true);  // (the device COO is released here)
    return g.release();
  }

  object::Graph<IDType, NNZType, ValueType> *ReadHIPGraph(context::HIPContext ctx) const {
    std::ifstream fin(filename_, std::ios::binary);
    if (!fin.is_open()) throw utils::ReaderException("file does not exist!");
    const std::string text((std::istreambuf_iterator<char>(fin)), std::istreambuf_iterator<char>());
    const detail::MetisHeader hd = detail::ParseMetisHeader(text);
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    const bool edge_weighted = hd.fmt == 1 || hd.fmt == 11, vertex_weighted = hd.fmt >= 10 && hd.ncon > 0;
    const int64_t n_dim = hd.n + (convert_to_zero_index_ ? 0 : 1), nnz = 2 * hd.m;
    const size_t bytes = text.size() - hd.body;
    auto &dev = hip::Device::Get(ctx.device_id);
    hip::Staged<char> d_text(dev, text.data() + hd.body, bytes + 1);
    const size_t cap = (size_t)nnz + 1;
    IDType *row = (IDType *)dev.Malloc(cap * sizeof(IDType)), *col = (IDType *)dev.Malloc(cap * sizeof(IDType));
    void *val = (edge_weighted && vb) ? dev.Malloc(cap * vb) : nullptr;
    const size_t weights = (vertex_weighted && vb) ? (size_t)n_dim * (size_t)hd.ncon : 0;
    void *vw = weights ? dev.Malloc(weights * vb) : nullptr;
    int64_t dims[2] = {0, 0};
    const int rc = sbgr_metis_parse(dev.handle(), hip::IndexTag<IDType>(), hip::ValueTag<ValueType>(), d_text.get(),
                                    (int64_t)bytes, hd.n, hd.m, hd.fmt, hd.ncon, convert_to_zero_index_ ? SBGR_ZERO_INDEX : 0u,
                                    (int64_t)cap, row, col, val, vw, nullptr, dims);
    std::vector<char> host_weights(weights * vb);
    if (rc == SBX_OK && weights) {
      try {
        dev.ToHost(host_weights.data(), vw, weights * vb);
      } catch (...) {
        dev.Free(row), dev.Free(col), dev.Free(val), dev.Free(vw);
        throw;
      }
    }
    dev.Free(vw);
    if (rc != SBX_OK) {
      dev.Free(row), dev.Free(col), dev.Free(val);
      throw utils::ReaderException(std::string("metis graph: ") + sbx_last_error(dev.handle()));
    }
    // already in (row, col) order: the constructor's check would find nothing to do
    auto *coo = new format::HIPCOO<IDType, NNZType, ValueType>((IDType)dims[0], (IDType)dims[0], (NNZType)dims[1], row, col,
                                                               (ValueType *)val, ctx, format::kOwned, true);
    if constexpr (std::is_same_v<ValueType, void>) {
      return new object::Graph<IDType, NNZType, ValueType>(coo);
    } else {
      format::Array<ValueType> **table = nullptr;
      if (vertex_weighted) {
        table = new format::Array<ValueType> *[(size_t)n_dim];
        const ValueType *w = (const ValueType *)host_weights.data();
        for (int64_t v = 0; v < n_dim; v++) {
          ValueType *mine = new ValueType[(size_t)hd.ncon];
          for (int j = 0; j < hd.ncon; j++) mine[j] = w[(size_t)v * hd.ncon + j];
          table[v] = new format::Array<ValueType>((format::DimensionType)hd.ncon, mine, format::kOwned);
        }
      }
      auto *g = new object::Graph<IDType, NNZType, ValueType>(coo, (NNZType)hd.ncon, table);
      if (table) g->OwnVertexWeights(table, (size_t)n_dim);
      return g;
    }
  }

 private:
  std::string filename_;
  bool convert_to_zero_index_;
};

}  // namespace sparsebase::io
#endif
