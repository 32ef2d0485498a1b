// sparsebase/io/patoh_writer.h — PaToH hypergraph writer (reference: io/patoh_writer.h, io/patoh_writer.cc:12-255).  The
// reference builds every line as a std::string on the host, for <int, int, int> alone, and rewrites the hypergraph's
// pin and net arrays in place when the base changes.  Here the nets x cells CSR — a host CSR or a HIPCSR — is formatted
// on the device (sbhg_patoh_format, sbhg_patoh_format_weights: include/sbhg.h) and leaves it in chunks of nets, cut by
// their number of items (pins + nets), through one page-locked buffer (io/writer.h); the hypergraph is left untouched
// and every type tuple is written.  Reproduced from the reference, byte for byte: the header `idx cells nets pins`, then
// ` scheme` when weighted, then ` constraints` for schemes 1 and 2 only and only when it is not 1 (the hypergraph's
// constraint_num_, as in the reference; the constructor's argument is not looked at there either); ids written as
// stored + (is_zero_indexed ? 0 : 1) - base_type_; no '\n' behind the file's last line; a void ValueType ignores both
// flags.
//
// One argument more than the reference: `precision` (default 6) for float and double weights, which the reference
// cannot write at all.  They print as `ostream << v`; 3.0f prints "3" and reads back, a non-integral weight prints but
// PatohReader refuses it (the format's weights are integers).
//
// Deliberate divergences: an empty net is an empty line, or the bare weight (the reference throws std::out_of_range on
// an unweighted one and never writes those behind the last pin); when the file's last line would be such an empty line
// it keeps its '\n', or the file would hold one net fewer; weighted flags without the weight arrays (null dereferences
// in the reference) are WriterExceptions; every check runs before the file is opened.
#ifndef SPARSEBASE_IO_PATOH_WRITER_H_
#define SPARSEBASE_IO_PATOH_WRITER_H_
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <string>

#include "sbhg.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/io/writer.h"
#include "sparsebase/object/object.h"

namespace sparsebase::io {

template <typename IDType, typename NNZType, typename ValueType>
class WritesHyperGraph {
 public:
  virtual ~WritesHyperGraph() = default;
  virtual void WriteHyperGraph(object::HyperGraph<IDType, NNZType, ValueType> *hyperGraph) const = 0;
};

template <typename IDType, typename NNZType, typename ValueType>
class PatohWriter : public WritesHyperGraph<IDType, NNZType, ValueType> {
 public:
  explicit PatohWriter(std::string filename, bool is_zero_indexed = true, bool is_edge_weighted = false,
                       bool is_vertex_weighted = false, int constraint_num = 1, int precision = 6)
      : filename_(std::move(filename)), is_zero_indexed_(is_zero_indexed), is_edge_weighted_(is_edge_weighted),
        is_vertex_weighted_(is_vertex_weighted), precision_(precision) {
    (void)constraint_num;
  }

  void WriteHyperGraph(object::HyperGraph<IDType, NNZType, ValueType> *hg) const override {
    if (precision_ < 1 || precision_ > 17) throw utils::WriterException("precision: 1..17");
    format::Format *con = hg->get_connectivity();
    if (!con) throw utils::WriterException("patoh: the hypergraph has no connectivity");
    if (con->template IsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>()) {
      auto *d = con->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
      const auto dims = d->get_dimensions();
      WriteDevice(hg, d->device(), (int64_t)dims[0], (int64_t)dims[1], (int64_t)d->get_num_nnz(), d->get_row_ptr(), d->get_col());
      return;
    }
    auto *csr = con->template AsAbsolute<format::CSR<IDType, NNZType, ValueType>>();
    const auto dims = csr->get_dimensions();
    const size_t pins = csr->get_num_nnz();
    auto &dev = hip::Device::Get(hip::DefaultDevice());
    hip::Staged<NNZType> xpin(dev, csr->get_row_ptr(), (size_t)dims[0] + 1);
    hip::Staged<IDType> pin(dev, csr->get_col(), pins);
    WriteDevice(hg, dev, (int64_t)dims[0], (int64_t)dims[1], (int64_t)pins, xpin.get(), pin.get());
  }

 private:
  void WriteDevice(object::HyperGraph<IDType, NNZType, ValueType> *hg, const hip::Device &dev, int64_t nets, int64_t cells,
                   int64_t pins, const NNZType *xpin, const IDType *pin) const {
    constexpr bool is_void = std::is_same_v<ValueType, void>;
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    const bool ew = !is_void && is_edge_weighted_, vw = !is_void && is_vertex_weighted_;
    const char *h_nw = nullptr, *h_cw = nullptr;
    if constexpr (!is_void) {
      if (ew) {
        if (!hg->netWeights_ || (int64_t)hg->netWeights_->get_dimensions()[0] < nets)
          throw utils::WriterException("patoh: is_edge_weighted, but the hypergraph has no weight for every net");
        h_nw = (const char *)hg->netWeights_->get_vals();
      }
      if (vw) {
        if (!hg->cellWeights_ || (int64_t)hg->cellWeights_->get_dimensions()[0] < cells)
          throw utils::WriterException("patoh: is_vertex_weighted, but the hypergraph has no weight for every cell");
        h_cw = (const char *)hg->cellWeights_->get_vals();
      }
    }
    hip::Staged<char> d_nw(dev, h_nw, h_nw ? (size_t)nets * vb : 0), d_cw(dev, h_cw, h_cw ? (size_t)cells * vb : 0);
    const sbx_index_type it = hip::IndexTag<IDType, NNZType>();
    const sbx_value_type vt = hip::ValueTag<ValueType>();
    const int64_t idx = is_zero_indexed_ ? 0 : 1, delta = idx - (int64_t)hg->base_type_;
    auto offset_at = [&](int64_t r) {
      NNZType o;
      dev.ToHost(&o, xpin + r, sizeof(NNZType));
      return (int64_t)o;
    };
    // without a cell-weight line the last net line is the file's last and loses its '\n' — unless it is empty
    const bool last_empty = nets > 0 && !ew && offset_at(nets) == offset_at(nets - 1);
    std::ofstream out = detail::OpenText(filename_);
    const int scheme = (vw ? 1 : 0) | (ew ? 2 : 0);
    out << idx << ' ' << cells << ' ' << nets << ' ' << pins;  // patoh_writer.cc:122, :149, :188, :220
    if (scheme) out << ' ' << scheme;
    if ((scheme == 1 || scheme == 2) && hg->constraint_num_ != 1) out << ' ' << (long long)hg->constraint_num_;
    out << "\n";
    detail::TextStreamer text(dev);
    const int precision = precision_;
    // The chunks are net ranges (their outputs concatenate to the whole), cut by what the formatter counts: a net weighs
    // its pins + 1 items, and a chunk is the longest run of nets that weighs at most SBX_TEXT_CHUNK_ENTRIES, one net at
    // the least: device text and pinned staging are bounded by the chunk size or the longest net.
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(SBX_TEXT_CHUNK_ENTRIES));
    auto weight_at = [&](int64_t r) { return offset_at(r) + r; };
    for (int64_t b = 0; b < nets;) {
      const int64_t e = detail::NextCut(b, nets, chunk, chunk, weight_at);
      const unsigned flags = (ew ? SBHG_NET_WEIGHTS : 0u) | ((e == nets && !vw && !last_empty) ? SBHG_NO_LAST_NEWLINE : 0u);
      text.Chunk(out, b, e - b, [&](int64_t begin, int64_t count, void *o, int64_t cap, int64_t *bytes) {
        return sbhg_patoh_format(dev.handle(), it, vt, begin, begin + count, xpin, pin, ew ? d_nw.get() : nullptr, delta,
                                 precision, flags, o, cap, bytes);
      });
      b = e;
    }
    if (vw)
      text.Stream(out, cells, [&](int64_t begin, int64_t count, void *o, int64_t cap, int64_t *bytes) {
        return sbhg_patoh_format_weights(dev.handle(), vt, begin, begin + count, d_cw.get(), precision, o, cap, bytes);
      });
    detail::CloseText(out, filename_);
  }

  std::string filename_;
  bool is_zero_indexed_, is_edge_weighted_, is_vertex_weighted_;
  int precision_;
};

}  // namespace sparsebase::io
#endif
