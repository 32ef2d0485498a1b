// sparsebase/io/edge_list_writer.h — edge list writer (reference: io/edge_list_writer.h:13-34,
// io/edge_list_writer.cc:11-190).
//
// "u v[ w]" per edge, zero-based.  The reference collects the edges in a vector of tuples, sorts and deduplicates an
// undirected list on the host (:26-51) and writes one `ofstream <<` per token.  Here the edges go to the GPU (if they
// are not there already); an undirected list goes through sbx_coo_undirected_unique on a copy (swap to u <= v, sort,
// first of every run); the lines are formatted on the device and leave it chunk by chunk (io/writer.h).  The list is
// weighted only when the format holds values (vals != nullptr), as in the reference (:95).
//
// One argument more than the reference: `precision` (default 6, what the reference's stream prints).
//
// Deliberate divergences:
//   - duplicates of an undirected list: the weight that survives is the first one in input order; the reference's
//     std::sort leaves it unspecified (the divergence io/edge_list_reader.h documents for the reader);
//   - a CSR's entries are written in (row, col) order (the device conversion applies the COO constructor's sort,
//     format/coo.cc:96-157); the reference walks the CSR's arrays as they stand — the same for every CSR whose rows
//     are sorted;
//   - every check runs before the file is opened; counts are 64-bit (the reference loops over int).
#ifndef SPARSEBASE_IO_EDGE_LIST_WRITER_H_
#define SPARSEBASE_IO_EDGE_LIST_WRITER_H_
#include <fstream>
#include <string>

#include "sparsebase/format/coo.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/io/writer.h"

namespace sparsebase::io {

template <typename IDType, typename NNZType, typename ValueType>
class EdgeListWriter {
 public:
  explicit EdgeListWriter(std::string filename, bool directed = true, int precision = 6)
      : filename_(std::move(filename)), directed_(directed), precision_(precision) {}

  void WriteCOO(format::COO<IDType, NNZType, ValueType> *coo) const {
    CheckOptions();
    const size_t nnz = coo->get_num_nnz();
    auto &dev = hip::Device::Get(hip::DefaultDevice());
    const char *hv = (const char *)coo->get_vals();
    hip::Staged<IDType> row(dev, coo->get_row(), nnz), col(dev, coo->get_col(), nnz);
    hip::Staged<char> val(dev, hv, nnz * hip::ValueBytes<ValueType>());
    WriteDevice(dev, (int64_t)nnz, row.get(), col.get(), hv ? val.get() : nullptr, /*scratch=*/true);
  }
  void WriteCSR(format::CSR<IDType, NNZType, ValueType> *csr) const {
    CheckOptions();
    const auto dims = csr->get_dimensions();
    const size_t n = dims[0], nnz = csr->get_num_nnz();
    auto &dev = hip::Device::Get(hip::DefaultDevice());
    const char *hv = (const char *)csr->get_vals();
    hip::Staged<NNZType> rp(dev, csr->get_row_ptr(), n + 1);
    hip::Staged<IDType> col(dev, csr->get_col(), nnz);
    hip::Staged<char> val(dev, hv, nnz * hip::ValueBytes<ValueType>());
    detail::CsrAsCoo<IDType, NNZType, ValueType> coo(dev, (int64_t)n, (int64_t)dims[1], (int64_t)nnz, rp.get(), col.get(),
                                                     hv ? val.get() : nullptr);
    WriteDevice(dev, (int64_t)nnz, coo.row, coo.col, coo.val, false);
  }
  void WriteHIPCOO(format::HIPCOO<IDType, NNZType, ValueType> *coo) const {
    CheckOptions();
    WriteDevice(coo->device(), (int64_t)coo->get_num_nnz(), coo->get_row(), coo->get_col(), (const void *)coo->get_vals(), false);
  }
  void WriteHIPCSR(format::HIPCSR<IDType, NNZType, ValueType> *csr) const {
    CheckOptions();
    const auto dims = csr->get_dimensions();
    const int64_t nnz = (int64_t)csr->get_num_nnz();
    auto &dev = csr->device();
    detail::CsrAsCoo<IDType, NNZType, ValueType> coo(dev, (int64_t)dims[0], (int64_t)dims[1], nnz, csr->get_row_ptr(),
                                                     csr->get_col(), (const void *)csr->get_vals());
    WriteDevice(dev, nnz, coo.row, coo.col, coo.val, false);
  }

 private:
  void CheckOptions() const {
    if (precision_ < 1 || precision_ > 17) throw utils::WriterException("precision: 1..17");
  }
  // scratch: the arrays are staging copies the call may reorder in place; otherwise an undirected list is made on copies
  void WriteDevice(const hip::Device &dev, int64_t nnz, const IDType *row, const IDType *col, const void *val,
                   bool scratch) const {
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    if (vb == 0) val = nullptr;
    const sbx_index_type it = hip::IndexTag<IDType, NNZType>();
    const sbx_value_type vt = hip::ValueTag<ValueType>();
    IDType *r2 = nullptr, *c2 = nullptr;
    void *v2 = nullptr;
    try {
      if (!directed_ && nnz > 0) {  // edge_list_writer.cc:26-51
        if (scratch) {
          r2 = const_cast<IDType *>(row);
          c2 = const_cast<IDType *>(col);
          v2 = const_cast<void *>(val);
        } else {
          r2 = static_cast<IDType *>(dev.Malloc((size_t)nnz * sizeof(IDType)));
          c2 = static_cast<IDType *>(dev.Malloc((size_t)nnz * sizeof(IDType)));
          dev.Copy(r2, row, (size_t)nnz * sizeof(IDType));
          dev.Copy(c2, col, (size_t)nnz * sizeof(IDType));
          if (val) {
            v2 = dev.Malloc((size_t)nnz * vb);
            dev.Copy(v2, val, (size_t)nnz * vb);
          }
        }
        int64_t left = 0;
        detail::WriterCheck(dev, sbx_coo_undirected_unique(dev.handle(), it, val ? vt : SBX_V_NONE, nnz, r2, c2, v2, &left));
        row = r2;
        col = c2;
        val = v2;
        nnz = left;
      }
      std::ofstream out = detail::OpenText(filename_);
      detail::TextStreamer text(dev);
      const int precision = precision_;
      text.Stream(out, nnz, [&](int64_t b, int64_t c, void *o, int64_t cap, int64_t *bytes) {
        return sbx_text_format_coordinate(dev.handle(), it, val ? vt : SBX_V_NONE, c, row + b, col + b,
                                          val ? (const void *)((const char *)val + (size_t)b * vb) : nullptr, 0, precision, 0u, o,
                                          cap, bytes);
      });
      detail::CloseText(out, filename_);
    } catch (...) {
      if (!scratch) {
        dev.Free(r2);
        dev.Free(c2);
        dev.Free(v2);
      }
      throw;
    }
    if (!scratch) {
      dev.Free(r2);
      dev.Free(c2);
      dev.Free(v2);
    }
  }

  std::string filename_;
  bool directed_;
  int precision_;
};

}  // namespace sparsebase::io
#endif
