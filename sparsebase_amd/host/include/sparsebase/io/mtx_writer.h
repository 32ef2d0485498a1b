// sparsebase/io/mtx_writer.h — Matrix Market writer (reference: io/mtx_writer.h:14-42, io/mtx_writer.cc:14-423).
//
// The reference writes one `ofstream <<` per token and checks a symmetric matrix with a double loop over its entries,
// quadratic in nnz (:116-168).  Here the matrix goes to the GPU (if it is not there already), the check is
// sbx_coo_symmetry_check (a sort and a search) and the lines are formatted on the device (include/sbx_text.h), leaving
// it chunk by chunk (io/writer.h).  Reproduced from the reference: the option checks and their messages (:38-69,
// :362-397), the refusal of a void ValueType (:83-85, :409), "Matrix is not symmetric!" (:109-112, :166),
// "Skew-symmetric matrix with non-zero diagonal values!" (:192), the banner and the size line — a symmetric file's
// NNZ is nnz - (nnz - diagonal) / 2, minus the diagonal count again when skew-symmetric (:194-199) — the entries a
// symmetric file keeps (col < row in input order, plus the diagonal unless skew-symmetric, :287-340), field "pattern"
// dropping the values, the array format of a COO (:213-259) and WriteArray's "1 <n>" size line (:415).
//
// One argument more than the reference: `precision` (default 6, what the reference's stream prints).  9 for float and
// 17 for double give a file that reads back bit-identical, which the reference has no way to write.
//
// Deliberate divergences:
//   - every check runs BEFORE the file is opened: a refused write neither creates nor truncates a file (the reference
//     opens the file first and leaves one that holds only the banner);
//   - vals == nullptr with a non-void ValueType: the symmetry check compares coordinates only and the lines carry no
//     value (the reference dereferences the null pointer);
//   - counts are 64-bit (the reference loops over int);
//   - array format: the entries may come in any order and a coordinate stored twice is refused (the reference
//     misaligns every later line behind one), as are n * m >= 2^31 cells (sbx_text_format_dense);
//   - an id outside the matrix is refused where the device path checks it (symmetric files, array format).
#ifndef SPARSEBASE_IO_MTX_WRITER_H_
#define SPARSEBASE_IO_MTX_WRITER_H_
#include <fstream>
#include <string>

#include "sparsebase/format/array.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/io/writer.h"

namespace sparsebase::io {

template <typename IDType, typename NNZType, typename ValueType>
class MTXWriter {
 public:
  explicit MTXWriter(std::string filename, std::string object = "matrix", std::string format = "coordinate",
                     std::string field = "real", std::string symmetry = "general", int precision = 6)
      : filename_(std::move(filename)), object_(std::move(object)), format_(std::move(format)), field_(std::move(field)),
        symmetry_(std::move(symmetry)), precision_(precision) {}

  void WriteCOO(format::COO<IDType, NNZType, ValueType> *coo) const {
    CheckOptions(false);  // (before anything is staged)
    const auto dims = coo->get_dimensions();
    const size_t nnz = coo->get_num_nnz();
    auto &dev = hip::Device::Get(hip::DefaultDevice());
    hip::Staged<IDType> row(dev, coo->get_row(), nnz), col(dev, coo->get_col(), nnz);
    hip::Staged<char> val(dev, HostValues(coo->get_vals()), nnz * hip::ValueBytes<ValueType>());
    WriteDevice(dev, (int64_t)dims[0], (int64_t)dims[1], (int64_t)nnz, row.get(), col.get(),
                HostValues(coo->get_vals()) ? val.get() : nullptr);
  }
  // mtx_writer.cc:356-365: CSR -> COO, then WriteCOO — the conversion on the device
  void WriteCSR(format::CSR<IDType, NNZType, ValueType> *csr) const {
    CheckOptions(false);
    const auto dims = csr->get_dimensions();
    const size_t n = dims[0], nnz = csr->get_num_nnz();
    auto &dev = hip::Device::Get(hip::DefaultDevice());
    hip::Staged<NNZType> rp(dev, csr->get_row_ptr(), n + 1);
    hip::Staged<IDType> col(dev, csr->get_col(), nnz);
    hip::Staged<char> val(dev, HostValues(csr->get_vals()), nnz * hip::ValueBytes<ValueType>());
    detail::CsrAsCoo<IDType, NNZType, ValueType> coo(dev, (int64_t)n, (int64_t)dims[1], (int64_t)nnz, rp.get(), col.get(),
                                                     HostValues(csr->get_vals()) ? val.get() : nullptr);
    WriteDevice(dev, (int64_t)n, (int64_t)dims[1], (int64_t)nnz, coo.row, coo.col, coo.val);
  }
  void WriteHIPCOO(format::HIPCOO<IDType, NNZType, ValueType> *coo) const {
    CheckOptions(false);
    const auto dims = coo->get_dimensions();
    WriteDevice(coo->device(), (int64_t)dims[0], (int64_t)dims[1], (int64_t)coo->get_num_nnz(), coo->get_row(), coo->get_col(),
                (const void *)coo->get_vals());
  }
  void WriteHIPCSR(format::HIPCSR<IDType, NNZType, ValueType> *csr) const {
    CheckOptions(false);
    const auto dims = csr->get_dimensions();
    const int64_t nnz = (int64_t)csr->get_num_nnz();
    auto &dev = csr->device();
    detail::CsrAsCoo<IDType, NNZType, ValueType> coo(dev, (int64_t)dims[0], (int64_t)dims[1], nnz, csr->get_row_ptr(),
                                                     csr->get_col(), (const void *)csr->get_vals());
    WriteDevice(dev, (int64_t)dims[0], (int64_t)dims[1], nnz, coo.row, coo.col, coo.val);
  }
  // mtx_writer.cc:367-423: "1 <n>" and one value per line
  void WriteArray(format::Array<ValueType> *arr) const {
    CheckOptions(true);
    if constexpr (std::is_same_v<ValueType, void>) {
      throw utils::WriterException("Cannot write an MTX with void ValueType");
    } else {
      const int64_t count = (int64_t)arr->get_dimensions()[0];
      auto &dev = hip::Device::Get(hip::DefaultDevice());
      hip::Staged<ValueType> vals(dev, arr->get_vals(), (size_t)count);
      std::ofstream out = detail::OpenText(filename_);
      out << "%%MatrixMarket " << object_ << " " << format_ << " " << field_ << " " << symmetry_ << "\n";
      out << 1 << " " << count << "\n";
      detail::TextStreamer text(dev);
      const ValueType *v = vals.get();
      const int precision = precision_;
      text.Stream(out, count, [&](int64_t b, int64_t c, void *o, int64_t cap, int64_t *bytes) {
        return sbx_text_format_values(dev.handle(), hip::ValueTag<ValueType>(), c, v + b, precision, o, cap, bytes);
      });
      detail::CloseText(out, filename_);
    }
  }

 private:
  template <typename V>
  static const char *HostValues(const V *vals) {
    return (const char *)vals;
  }
  // mtx_writer.cc:38-69 (WriteCOO) and :362-397 (WriteArray), in the reference's order and words
  void CheckOptions(bool array_object) const {
    if (object_ != "matrix" && object_ != "vector")
      throw utils::WriterException("Illegal value for the 'object' option in matrix market header");
    else if (object_ == "vector")
      throw utils::WriterException("Matrix market writer does not currently support writing vectors.");
    if (format_ != "array" && format_ != "coordinate")
      throw utils::WriterException("Illegal value for the 'format' option in matrix market header");
    if (field_ != "real" && field_ != "double" && field_ != "complex" && field_ != "integer" && field_ != "pattern")
      throw utils::WriterException("Illegal value for the 'field' option in matrix market header");
    if (symmetry_ != "general" && symmetry_ != "symmetric" && symmetry_ != "skew-symmetric" && symmetry_ != "hermitian")
      throw utils::WriterException("Illegal value for the 'symmetry' option in matrix market header");
    if (format_ == "array" && field_ == "pattern")
      throw utils::WriterException("Matrix market files with array format cannot have the field 'pattern' ");
    if (format_ == "array" && symmetry_ != "general")
      throw utils::WriterException("Matrix market files with array format cannot have the property 'symmetry' ");
    if (symmetry_ == "hermitian")
      throw utils::WriterException("Matrix market writer does not currently support hermitian symmetry.");
    if (array_object && format_ == "coordinate")
      throw utils::WriterException("Matrix market writer does not currently support writing array as coordinate.");
    if (precision_ < 1 || precision_ > 17) throw utils::WriterException("precision: 1..17");
  }

  // row / col / val: device arrays of nnz entries (val may be null); every check, then the file
  void WriteDevice(const hip::Device &dev, int64_t n, int64_t m, int64_t nnz, const IDType *row, const IDType *col,
                   const void *val) const {
    constexpr bool is_void = std::is_same_v<ValueType, void>;
    if (is_void && field_ != "pattern")
      throw utils::WriterException("Cannot write an MTX with void ValueType, unless field is pattern.");
    if (is_void) val = nullptr;
    const sbx_index_type it = hip::IndexTag<IDType, NNZType>();
    const sbx_value_type vt = hip::ValueTag<ValueType>();
    const bool said_symmetric = symmetry_ == "symmetric" || symmetry_ == "skew-symmetric", skew = symmetry_ == "skew-symmetric";
    int64_t size_nnz = nnz;
    if (said_symmetric) {
      if (n != m) throw utils::WriterException("Matrix is not symmetric!");
      int64_t res[3] = {1, 0, 0};
      detail::WriterCheck(dev, sbx_coo_symmetry_check(dev.handle(), it, vt, n, nnz, row, col, val, skew ? 1 : 0, res));
      if (!res[0]) throw utils::WriterException("Matrix is not symmetric!");
      if (skew && res[2]) throw utils::WriterException("Skew-symmetric matrix with non-zero diagonal values!");
      size_nnz = nnz - (nnz - res[1]) / 2 - (skew ? res[1] : 0);  // :194-199, count_symmetric = nnz - count_diagonal
    }
    detail::TextStreamer text(dev);
    const int precision = precision_;
    if (format_ == "array") {
      const int64_t bytes = text.Format([&](void *o, int64_t cap, int64_t *b) {
        return sbx_text_format_dense(dev.handle(), it, vt, n, m, nnz, row, col, val, precision, o, cap, b);
      });
      std::ofstream out = detail::OpenText(filename_);
      out << "%%MatrixMarket " << object_ << " " << format_ << " " << field_ << " " << symmetry_ << "\n";
      out << n << " " << m << "\n";
      text.Flush(out, bytes);
      detail::CloseText(out, filename_);
      return;
    }
    const unsigned flags = (field_ == "pattern" ? SBX_TEXT_PATTERN : 0u) | (said_symmetric ? SBX_TEXT_LOWER : 0u) |
                           (skew ? SBX_TEXT_NO_DIAGONAL : 0u);
    std::ofstream out = detail::OpenText(filename_);
    out << "%%MatrixMarket " << object_ << " " << format_ << " " << field_ << " " << symmetry_ << "\n";
    out << n << " " << m << " " << size_nnz << "\n";
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    text.Stream(out, nnz, [&](int64_t b, int64_t c, void *o, int64_t cap, int64_t *bytes) {
      return sbx_text_format_coordinate(dev.handle(), it, vt, c, row + b, col + b,
                                        val ? (const void *)((const char *)val + (size_t)b * vb) : nullptr, 1, precision, flags, o,
                                        cap, bytes);
    });
    detail::CloseText(out, filename_);
  }

  std::string filename_, object_, format_, field_, symmetry_;
  int precision_;
};

}  // namespace sparsebase::io
#endif
