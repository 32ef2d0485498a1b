// sparsebase/io/metis_graph_writer.h — METIS graph writer (reference: io/metis_graph_writer.h:20-37,
// io/metis_graph_writer.cc:14-85).  The reference converts the Graph's COO to a CSR on the host and writes one
// `ofstream <<` per token.  Here the connectivity — a host COO or a HIPCOO — becomes a CSR on the device
// (sbx_coo_to_csr), the lines are formatted there (sbgr_metis_format, include/sbgr.h) and leave it in chunks of rows,
// cut by their number of entries, through one page-locked buffer (io/writer.h).  Reproduced from the reference: the
// header line `" " n " " nnz/2`, then for a non-void ValueType `" " FMT` — 1, 11, or 10: a writer with neither flag
// writes 10 — and `" " NCON` when vertex-weighted with NCON > 0; n = dim0 - !zero_indexed, and row 0 is skipped unless
// zero_indexed; the spacing of the lines, byte for byte; a void ValueType ignores both flags.
//
// One argument more than the reference: `precision` (default 6, what the reference's stream prints); 9 for float and 17
// for double give a file that reads back bit-identical.
//
// Deliberate divergences: edgeWeighted without values and vertexWeighted with a null vertexWeights_ (null dereferences in
// the reference) are WriterExceptions; every check runs before the file is opened.
#ifndef SPARSEBASE_IO_METIS_GRAPH_WRITER_H_
#define SPARSEBASE_IO_METIS_GRAPH_WRITER_H_
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

#include "sbgr.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/io/writer.h"
#include "sparsebase/object/object.h"

namespace sparsebase::io {

template <typename IDType, typename NNZType, typename ValueType>
class MetisGraphWriter {
 public:
  explicit MetisGraphWriter(std::string filename, bool edgeWeighted = false, bool vertexWeighted = false,
                            bool zero_indexed = false, int precision = 6)
      : filename_(std::move(filename)), edgeWeighted_(edgeWeighted), vertexWeighted_(vertexWeighted),
        zero_indexed_(zero_indexed), precision_(precision) {}

  void WriteGraph(object::Graph<IDType, NNZType, ValueType> *graph) const {
    if (precision_ < 1 || precision_ > 17) throw utils::WriterException("precision: 1..17");
    format::Format *con = graph->get_connectivity();
    if (!con) throw utils::WriterException("metis graph: the graph has no connectivity");
    if (con->template IsAbsolute<format::HIPCOO<IDType, NNZType, ValueType>>()) {
      auto *d = con->template AsAbsolute<format::HIPCOO<IDType, NNZType, ValueType>>();
      const auto dims = d->get_dimensions();
      WriteDevice(graph, d->device(), (int64_t)dims[0], (int64_t)d->get_num_nnz(), d->get_row(), d->get_col(),
                  (const void *)d->get_vals(), d->rows_known_sorted());
      return;
    }
    auto *coo = con->template AsAbsolute<format::COO<IDType, NNZType, ValueType>>();
    const auto dims = coo->get_dimensions();
    const size_t nnz = coo->get_num_nnz();
    auto &dev = hip::Device::Get(hip::DefaultDevice());
    hip::Staged<IDType> row(dev, coo->get_row(), nnz), col(dev, coo->get_col(), nnz);
    const char *hv = (const char *)coo->get_vals();
    hip::Staged<char> val(dev, hv, nnz * hip::ValueBytes<ValueType>());
    WriteDevice(graph, dev, (int64_t)dims[0], (int64_t)nnz, row.get(), col.get(), hv ? val.get() : nullptr, false);
  }

 private:
  // row / col / val: the device COO in (row, col) order (val may be null)
  void WriteDevice(object::Graph<IDType, NNZType, ValueType> *graph, const hip::Device &dev, int64_t dim0, int64_t nnz,
                   const IDType *row, const IDType *col, const void *val, bool rows_sorted) const {
    constexpr bool is_void = std::is_same_v<ValueType, void>;
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    const bool ew = !is_void && edgeWeighted_, vw = !is_void && vertexWeighted_;
    if (ew && !val) throw utils::WriterException("metis graph: edgeWeighted, but the connectivity has no values");
    if (vw && !graph->vertexWeights_) throw utils::WriterException("metis graph: vertexWeighted, but the graph has no vertex weights");
    const int ncon = vw ? (int)graph->ncon_ : 0;
    const int64_t row_begin = zero_indexed_ ? 0 : 1;
    if (dim0 < row_begin) throw utils::WriterException("metis graph: a graph that is not zero-indexed has row 0");
    // the vertex weights, row-major, on the device
    std::vector<char> host_weights;
    if constexpr (!is_void) {
      if (vw && ncon > 0) {
        host_weights.resize((size_t)dim0 * ncon * vb);
        ValueType *w = (ValueType *)host_weights.data();
        for (int64_t v = 0; v < dim0; v++) {
          const format::Array<ValueType> *a = v >= row_begin ? graph->vertexWeights_[v] : nullptr;  // (row 0 is not written)
          if (v >= row_begin && (!a || (int64_t)a->get_dimensions()[0] < ncon))
            throw utils::WriterException("metis graph: a vertex has fewer weights than ncon_");
          for (int j = 0; j < ncon; j++) w[(size_t)v * ncon + j] = a ? a->get_vals()[j] : ValueType(0);
        }
      }
    }
    hip::Staged<char> d_weights(dev, host_weights.empty() ? nullptr : host_weights.data(), host_weights.size());
    hip::Staged<NNZType> rp(dev, (size_t)dim0 + 1);
    const sbx_index_type it = hip::IndexTag<IDType, NNZType>();
    const sbx_value_type vt = hip::ValueTag<ValueType>();
    if (!rows_sorted && nnz > 1) {  // (a COO built with its sort skipped: col and val would not follow the row offsets)
      int sorted = 1;
      detail::WriterCheck(dev, sbx_coo_is_sorted(dev.handle(), it, nnz, row, col, &sorted));
      if (!sorted) throw utils::WriterException("metis graph: the connectivity is not in (row, col) order");
      rows_sorted = true;
    }
    detail::WriterCheck(dev, sbx_coo_to_csr(dev.handle(), it, SBX_V_NONE, dim0, dim0, nnz, row, nullptr, nullptr, rp.get(), nullptr,
                                            nullptr, SBX_FLAG_MOVE | (rows_sorted ? SBX_FLAG_ROWS_SORTED : 0u)));
    std::ofstream out = detail::OpenText(filename_);
    out << " " << (dim0 - row_begin) << " " << nnz / 2;  // metis_graph_writer.cc:41
    if (!is_void) {
      out << " " << (ew && !vw ? "1" : ew ? "11" : "10");  // :56-63
      if (ncon > 0) out << " " << ncon;
    }
    out << "\n";
    detail::TextStreamer text(dev);
    const unsigned flags = (ew ? SBGR_EDGE_WEIGHTS : 0u) | (vw ? SBGR_VERTEX_WEIGHTS : 0u);
    const int precision = precision_;
    const int64_t base = zero_indexed_ ? 1 : 0;  // :47, :75: col + zero_indexed
    // The chunks are row ranges (their outputs concatenate to the whole), cut by what the formatter counts: a row weighs
    // its entries + 1 + ncon items, and a chunk is the longest run of rows that weighs at most SBX_TEXT_CHUNK_ENTRIES,
    // one row at the least.  So device text and pinned staging are bounded by max(SBX_TEXT_CHUNK_ENTRIES, the longest
    // row's weight) items, whatever the graph's size, and a call stays below the formatter's 2^32 items unless one row
    // alone exceeds them.  The cuts are found by a binary search (detail::NextCut) that reads single offsets of the device
    // row_ptr; rows weigh row_items at the least, which bounds the rows of a chunk.
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(SBX_TEXT_CHUNK_ENTRIES)), row_items = 1 + ncon;
    auto weight_at = [&](int64_t r) {
      NNZType o;
      dev.ToHost(&o, rp.get() + r, sizeof(NNZType));
      return (int64_t)o + r * row_items;
    };
    auto format = [&](int64_t b, int64_t c, void *o, int64_t cap, int64_t *bytes) {
      return sbgr_metis_format(dev.handle(), it, vt, b, b + c, rp.get(), col, ew ? val : nullptr,
                               host_weights.empty() ? nullptr : d_weights.get(), ncon, base, precision, flags, o, cap, bytes);
    };
    for (int64_t b = row_begin; b < dim0;) {
      const int64_t e = detail::NextCut(b, dim0, std::max<int64_t>(1, chunk / row_items), chunk, weight_at);
      text.Chunk(out, b, e - b, format);
      b = e;
    }
    detail::CloseText(out, filename_);
  }

  std::string filename_;
  bool edgeWeighted_, vertexWeighted_, zero_indexed_;
  int precision_;
};

}  // namespace sparsebase::io
#endif
