// sparsebase/io/mtx_reader.h — Matrix Market reader (reference: io/mtx_reader.h:16-63,
// io/mtx_reader.cc:11-585), coordinate and array format, into COO / CSR / Array.  The banner and the size
// line are parsed here exactly like the reference's ParseHeader (:29-120, same exceptions); the
// entry section — where the time goes — is shipped to the GPU and parsed there.
//   coordinate files: sbx_mtx_parse_coordinate (tokenization, exact decimal -> binary conversion,
//     symmetric expansion), followed by the COO constructor's sort, also on the GPU;
//   array files (:121-166): sbio_mtx_parse_values reads the M * N values, sbio_dense_to_coo keeps the
//     cells != 0 in (row, col) order — the COO constructor's check passes and nothing is sorted;
//   ReadArray / ReadHIPArray (:541-569): an array file's values as they stand (:496-539); a
//     coordinate file of a 1 x N or N x 1 matrix through ReadHIPCOO and sbio_coo_to_dense_vector (:265-305).
// The reference's refusals keep their words: array files that are not general or carry the field
// 'pattern', a void ValueType, a pattern file or an M x N matrix (M != 1 and N != 1) read into an Array.
//
// Deliberate divergences for array files (the reference's behaviour was observed on its own build):
//   - a file with the size line "M N" gives a matrix of M rows and N columns, as the file says and as
//     MTXWriter wrote it.  The reference constructs COO(N, M, ...) — the dimensions swapped — over row
//     ids l % M in [0, M): a "2 3" file comes back as 3 x 2 with rows in [0, 2), and converting such a
//     COO to CSR overruns row_ptr when M > N;
//   - fewer than M * N values: refused.  The reference's failed stream repeats a stale value
//     ("1 2 3" for a 2 x 2 file gave 1, 3, 2, 3);
//   - a token the ValueType cannot hold ("1.5" into an integer type, "nan"): refused, as in the
//     coordinate section.  The reference's stream fails there and every later value is lost;
//   - field 'complex': refused.  The reference reads M * N of the 2 * M * N tokens and returns a mix of
//     real and imaginary parts;
//   - ReadArray on a coordinate file: an entry outside the vector (for example every file read with
//     convert_to_zero_index = false, whose last position is max(M, N)) is refused; the reference
//     writes out of bounds.  Of two entries at one position the later one in (row, col) order wins,
//     as in the reference's loop;
//   - M * N >= 2^31 cells are refused (sbio_dense_to_coo).
#ifndef SPARSEBASE_IO_MTX_READER_H_
#define SPARSEBASE_IO_MTX_READER_H_
#include <fstream>
#include <sstream>
#include <string>

#include "sbio.h"
#include "sparsebase/converter/converter_order_two.h"
#include "sparsebase/format/array.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/utils/exception.h"

namespace sparsebase::io {

template <typename IDType, typename NNZType, typename ValueType>
class MTXReader {
 public:
  explicit MTXReader(std::string filename, bool convert_to_zero_index = true, bool upper_triangle = false)
      : filename_(std::move(filename)), convert_to_zero_index_(convert_to_zero_index), upper_triangle_(upper_triangle) {
    std::ifstream fin(filename_);
    if (!fin.is_open()) throw utils::ReaderException("Wrong matrix market file name\n");
    std::string header_line;
    std::getline(fin, header_line);
    options_ = ParseHeader(header_line);
  }

  // host COO, entries in (row, col) order as the reference's COO constructor leaves them
  format::COO<IDType, NNZType, ValueType> *ReadCOO() const {
    std::unique_ptr<format::HIPCOO<IDType, NNZType, ValueType>> d(ReadHIPCOO(context::HIPContext(hip::DefaultDevice())));
    context::CPUContext cpu;
    return static_cast<format::COO<IDType, NNZType, ValueType> *>(
        converter::HIPCooCooConditionalFunction<IDType, NNZType, ValueType>(d.get(), &cpu));
  }
  format::CSR<IDType, NNZType, ValueType> *ReadCSR() const {  // mtx_reader.cc:517-523: ReadCOO + convert
    std::unique_ptr<format::HIPCOO<IDType, NNZType, ValueType>> d(ReadHIPCOO(context::HIPContext(hip::DefaultDevice())));
    context::HIPContext gpu(d->get_hip_context()->device_id);
    std::unique_ptr<format::Format> dcsr(converter::HIPCooHIPCsrFunction<IDType, NNZType, ValueType, true>(d.get(), &gpu));
    context::CPUContext cpu;
    return static_cast<format::CSR<IDType, NNZType, ValueType> *>(
        converter::HIPCsrCsrConditionalFunction<IDType, NNZType, ValueType>(dcsr.get(), &cpu));
  }
  // the same matrix left in HBM (what a GPU pipeline wants: no host copy of the entries at all)
  format::HIPCOO<IDType, NNZType, ValueType> *ReadHIPCOO(context::HIPContext ctx) const {
    (void)hip::IndexTag<IDType, NNZType>();  // (a COO holds id arrays only: any tuple the device path takes)
    if (options_.format != kCoordinate) return ReadArrayFileIntoHIPCOO(ctx);
    long long M = 0, N = 0, L = 0;
    size_t body = 0;
    const std::string text = Load(3, &M, &N, &L, &body);
    const bool weighted = options_.field != kPattern;
    const int symmetry = options_.symmetry == kGeneral ? 0 : options_.symmetry == kSymmetric ? 1 : 2;
    // the reference honours upper_triangle for symmetric files only (:201-214)
    const bool upper = upper_triangle_ && options_.symmetry == kSymmetric;
    const bool expand = symmetry != 0 && !upper;
    auto &dev = hip::Device::Get(ctx.device_id);
    const size_t cap = (size_t)L * (expand ? 2 : 1) + 1;
    hip::Staged<char> d_text(dev, text.data() + body, text.size() - body + 1);
    IDType *row = (IDType *)dev.Malloc(cap * sizeof(IDType)), *col = (IDType *)dev.Malloc(cap * sizeof(IDType));
    void *val = nullptr;
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    if (weighted && vb) val = dev.Malloc(cap * vb);
    int64_t nnz = 0;
    unsigned flags = (convert_to_zero_index_ ? SBX_MTX_ZERO_INDEX : 0u) | (upper ? SBX_MTX_UPPER_TRIANGLE : 0u);
    const int rc = sbx_mtx_parse_coordinate(dev.handle(), hip::IndexTag<IDType>(), hip::ValueTag<ValueType>(), d_text.get(),
                                            (int64_t)(text.size() - body), M, N, L, weighted ? 3 : 2, symmetry, flags,
                                            (int64_t)cap, row, col, val, &nnz);
    if (rc != SBX_OK) {
      dev.Free(row);
      dev.Free(col);
      if (val) dev.Free(val);
      throw utils::ReaderException(std::string("matrix market coordinate section: ") + sbx_last_error(dev.handle()));
    }
    // the COO constructor checks / sorts on the device (format/coo.cc:96-157)
    return new format::HIPCOO<IDType, NNZType, ValueType>((IDType)M, (IDType)N, (NNZType)nnz, row, col, (ValueType *)val,
                                                         ctx, format::kOwned, false);
  }


  // mtx_reader.cc:541-569; the values end on the host
  format::Array<ValueType> *ReadArray() const {
    if constexpr (std::is_same_v<ValueType, void>) {
      throw utils::ReaderException("Cannot read a matrix market file into an Array whose ValueType is void");
    } else {
      std::unique_ptr<format::HIPArray<ValueType>> d(ReadHIPArray(context::HIPContext(hip::DefaultDevice())));
      const size_t count = (size_t)d->get_dimensions()[0];
      ValueType *vals = new ValueType[count ? count : 1];
      try {
        if (count) hip::Device::Get(d->get_hip_context()->device_id).ToHost(vals, d->get_vals(), count * sizeof(ValueType));
      } catch (...) {
        delete[] vals;
        throw;
      }
      return new format::Array<ValueType>((format::DimensionType)count, vals, format::kOwned);
    }
  }
  // the same vector left in HBM
  format::HIPArray<ValueType> *ReadHIPArray(context::HIPContext ctx) const {
    if constexpr (std::is_same_v<ValueType, void>) {
      throw utils::ReaderException("Cannot read a matrix market file into an Array whose ValueType is void");
    } else {
      if (options_.field == kPattern)
        throw utils::ReaderException("Cannot read a matrix market file into an Array if it is in pattern format");
      const bool array_file = options_.format == kArray;
      long long M = 0, N = 0, L = 0;
      size_t body = 0;
      const std::string text = Load(array_file ? 2 : 3, &M, &N, &L, &body);
      if (M != 1 && N != 1)
        throw utils::ReaderException(
            "Trying to read a 2D matrix with multiple rows and multiple columns into dense array");
      auto &dev = hip::Device::Get(ctx.device_id);
      if (array_file) {  // :496-539
        const int64_t count = CellCount(M, N);
        ValueType *vals = ParseValues(dev, text, body, count);
        return new format::HIPArray<ValueType>((format::DimensionType)count, vals, ctx, format::kOwned);
      }
      // :265-305: the COO, then vals[row + col] = value
      std::unique_ptr<format::HIPCOO<IDType, NNZType, ValueType>> coo(ReadHIPCOO(ctx));
      const int64_t len = (int64_t)std::max(M, N);
      ValueType *vals = (ValueType *)dev.Malloc((size_t)len * sizeof(ValueType));
      const int rc = coo->get_vals() == nullptr && coo->get_num_nnz() > 0
                         ? SBX_ERR_BAD_ARG
                         : sbio_coo_to_dense_vector(dev.handle(), hip::IndexTag<IDType, NNZType>(), hip::ValueTag<ValueType>(), len,
                                                    (int64_t)coo->get_num_nnz(), coo->get_row(), coo->get_col(),
                                                    coo->get_vals(), vals);
      if (rc != SBX_OK) {
        dev.Free(vals);
        throw utils::ReaderException(std::string("matrix market coordinate file into an Array: ") + sbx_last_error(dev.handle()));
      }
      return new format::HIPArray<ValueType>((format::DimensionType)len, vals, ctx, format::kOwned);
    }
  }

 private:
  enum Format { kCoordinate, kArray };
  enum Field { kReal, kDouble, kComplex, kInteger, kPattern };
  enum Symmetry { kGeneral, kSymmetric, kSkewSymmetric };
  struct Options {
    Format format;
    Field field;
    Symmetry symmetry;
  };
  static void NoVoidValues() {
    if constexpr (std::is_same_v<void, ValueType>)
      throw utils::ReaderException("You are reading the values of the matrix market file into a void array");
  }
  // the whole file; the banner and the comment lines skipped (:318-319), the size line's `fields` numbers read (:321);
  // *body: where the entries begin
  std::string Load(int fields, long long *M, long long *N, long long *L, size_t *body) const {
    std::ifstream fin(filename_, std::ios::binary);
    if (!fin.is_open()) throw utils::ReaderException("file does not exists!!");
    std::string text((std::istreambuf_iterator<char>(fin)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    while (pos < text.size() && text[pos] == '%') {
      const size_t eol = text.find('\n', pos);
      pos = eol == std::string::npos ? text.size() : eol + 1;
    }
    const size_t size_end = text.find('\n', pos);
    std::istringstream size_line(text.substr(pos, size_end == std::string::npos ? std::string::npos : size_end - pos));
    size_line >> *M >> *N;
    if (fields == 3) size_line >> *L;
    if (!size_line) throw utils::ReaderException("malformed size line in matrix market file");
    *body = size_end == std::string::npos ? text.size() : size_end + 1;
    return text;
  }
  static int64_t CellCount(long long M, long long N) {
    if (M < 0 || N < 0) throw utils::ReaderException("malformed size line in matrix market file");
    if (M >= (1ll << 31) || N >= (1ll << 31) || M * N >= (1ll << 31))
      throw utils::ReaderException("array-format matrix market files of 2^31 cells and more are not read by this library");
    return (int64_t)(M * N);
  }
  // the first `count` values behind the size line, on the device (the caller owns the block)
  template <typename V = ValueType>
  V *ParseValues(const hip::Device &dev, const std::string &text, size_t body, int64_t count) const {
    if (options_.field == kComplex)
      throw utils::ReaderException("complex array-format Matrix Market files are not read by this library");
    hip::Staged<char> d_text(dev, text.data() + body, text.size() - body + 1);
    V *vals = (V *)dev.Malloc((size_t)count * sizeof(V));
    const int rc = sbio_mtx_parse_values(dev.handle(), hip::ValueTag<V>(), d_text.get(), (int64_t)(text.size() - body), count, vals);
    if (rc != SBX_OK) {
      dev.Free(vals);
      throw utils::ReaderException(std::string("matrix market array section: ") + sbx_last_error(dev.handle()));
    }
    return vals;
  }
  // mtx_reader.cc:121-166 and the refusals of :171-186
  format::HIPCOO<IDType, NNZType, ValueType> *ReadArrayFileIntoHIPCOO(context::HIPContext ctx) const {
    if (options_.symmetry != kGeneral)
      throw utils::ReaderException(
          "Library does not support reading array files that are symmetric, skew-symmetric, or hermetian");
    if (options_.field == kPattern)
      throw utils::ReaderException("Matrix market files with array format cannot have the field 'pattern' ");
    if constexpr (std::is_same_v<ValueType, void>) {
      throw utils::ReaderException("Weight type for weighted graphs can not be void");
    } else {
      long long M = 0, N = 0, L = 0;
      size_t body = 0;
      const std::string text = Load(2, &M, &N, &L, &body);
      const int64_t cells = CellCount(M, N);
      auto &dev = hip::Device::Get(ctx.device_id);
      const sbx_index_type it = hip::IndexTag<IDType, NNZType>();
      const sbx_value_type vt = hip::ValueTag<ValueType>();
      ValueType *dense_raw = ParseValues(dev, text, body, cells);
      struct Freed {  // (the dense staging block goes back whichever way this function is left)
        const hip::Device &dev;
        void *p;
        ~Freed() { dev.Free(p); }
      } dense{dev, dense_raw};
      auto fail = [&]() { return utils::ReaderException(std::string("matrix market array section: ") + sbx_last_error(dev.handle())); };
      int64_t nnz = 0;
      if (sbio_dense_to_coo(dev.handle(), it, vt, M, N, dense.p, 0, nullptr, nullptr, nullptr, &nnz) != SBX_OK) throw fail();
      const size_t cap = (size_t)nnz + 1;
      IDType *row = (IDType *)dev.Malloc(cap * sizeof(IDType)), *col = (IDType *)dev.Malloc(cap * sizeof(IDType));
      ValueType *val = (ValueType *)dev.Malloc(cap * sizeof(ValueType));
      int64_t filled = 0;
      if (nnz > 0 && sbio_dense_to_coo(dev.handle(), it, vt, M, N, dense.p, nnz, row, col, val, &filled) != SBX_OK) {
        dev.Free(row);
        dev.Free(col);
        dev.Free(val);
        throw fail();
      }
      dev.Sync();  // (the fill is enqueued; the staging block is released behind it)
      // already in (row, col) order: the COO constructor's check passes, nothing is sorted
      return new format::HIPCOO<IDType, NNZType, ValueType>((IDType)M, (IDType)N, (NNZType)nnz, row, col, val, ctx,
                                                           format::kOwned, false);
    }
  }
  static Options ParseHeader(const std::string &header_line) {  // mtx_reader.cc:29-120
    std::stringstream line_ss(header_line);
    Options o;
    std::string prefix, object, format, field, symmetry;
    line_ss >> prefix >> object >> format >> field >> symmetry;
    if (prefix != "%%MatrixMarket") throw utils::ReaderException("Wrong prefix in a matrix market file");
    if (object == "vector")
      throw utils::ReaderException("Matrix market reader does not currently support reading vectors.");
    if (object != "matrix") throw utils::ReaderException("Illegal value for the 'object' option in matrix market header");
    if (format == "array") o.format = kArray;
    else if (format == "coordinate") o.format = kCoordinate;
    else throw utils::ReaderException("Illegal value for the 'format' option in matrix market header");
    if (field == "real") { o.field = kReal; NoVoidValues(); }
    else if (field == "double") { o.field = kDouble; NoVoidValues(); }
    else if (field == "complex") { o.field = kComplex; NoVoidValues(); }
    else if (field == "integer") { o.field = kInteger; NoVoidValues(); }
    else if (field == "pattern") o.field = kPattern;
    else throw utils::ReaderException("Illegal value for the 'field' option in matrix market header");
    if (symmetry == "general") o.symmetry = kGeneral;
    else if (symmetry == "symmetric") o.symmetry = kSymmetric;
    else if (symmetry == "skew-symmetric") o.symmetry = kSkewSymmetric;
    else if (symmetry == "hermitian")
      throw utils::ReaderException("Matrix market reader does not currently support hermitian symmetry.");
    else throw utils::ReaderException("Illegal value for the 'symmetry' option in matrix market header");
    return o;
  }

  std::string filename_;
  bool convert_to_zero_index_, upper_triangle_;
  Options options_;
};

}  // namespace sparsebase::io
#endif
