// sparsebase/io/writer.h — what the text writers share (reference: io/writer.h declares the WritesCOO / WritesCSR /
// WritesArray interfaces; here the shared part is how device text reaches a file).
//
// The text is produced on the device by the formatters of include/sbx_text.h and leaves it in chunks of
// SBX_TEXT_CHUNK_ENTRIES entries (a compile-time macro, default 2^24): every chunk is formatted into one device buffer,
// copied into one page-locked host buffer (sbx_host_alloc) and handed to the stream with ONE write.  Device text and
// pinned staging therefore stay bounded whatever the matrix size, and — the formatters promise that the outputs of
// sub-ranges concatenate to the output of the whole — the file's bytes do not depend on the chunk size.
#ifndef SPARSEBASE_IO_WRITER_H_
#define SPARSEBASE_IO_WRITER_H_
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <ostream>
#include <string>

#include "sbx_text.h"
#include "sparsebase/hip/device.h"
#include "sparsebase/utils/exception.h"

#ifndef SBX_TEXT_CHUNK_ENTRIES
#define SBX_TEXT_CHUNK_ENTRIES (1 << 24)
#endif

namespace sparsebase::io::detail {

inline void WriterCheck(const hip::Device &dev, int rc) {
  if (rc != SBX_OK) throw utils::WriterException(std::string("text writer: ") + sbx_last_error(dev.handle()));
}

// the file a writer fills, and its end: closed, and whatever went wrong on the way reported
inline std::ofstream OpenText(const std::string &filename) {
  std::ofstream out(filename, std::ios::binary);
  if (!out.is_open()) throw utils::WriterException("cannot open " + filename + " for writing");
  return out;
}
inline void CloseText(std::ofstream &out, const std::string &filename) {
  out.close();
  if (!out) throw utils::WriterException("writing " + filename + " failed");
}

// For the writers that cut their chunks themselves (rows of unequal length): the end of the longest run of rows from b,
// of max_rows rows and up to `end` at the most, that weighs at most `chunk` — one row at the least.  weight_at(r) is the
// weight of the rows before r, ascending; it is read at b and at O(log max_rows) places more.
template <typename W>
int64_t NextCut(int64_t b, int64_t end, int64_t max_rows, int64_t chunk, W weight_at) {
  int64_t lo = b + 1, hi = std::min(end, b + max_rows);
  if (lo < hi) {
    const int64_t limit = weight_at(b) + chunk;
    if (weight_at(hi) <= limit) lo = hi;
    while (lo + 1 < hi) {  // (weight(lo) <= limit or lo == b + 1; weight(hi) > limit)
      const int64_t mid = lo + (hi - lo) / 2;
      (weight_at(mid) <= limit ? lo : hi) = mid;
    }
  }
  return lo;
}

class TextStreamer {
 public:
  explicit TextStreamer(const hip::Device &dev) : dev_(dev) {}
  ~TextStreamer() {
    dev_.Free(d_text_);
    dev_.HostFree(h_text_);
  }
  TextStreamer(const TextStreamer &) = delete;
  TextStreamer &operator=(const TextStreamer &) = delete;

  // call(begin, count, text_out, capacity, &bytes) -> sbx status: one of the formatters on entries [begin, begin + count).
  // A chunk is formatted straight into the buffers the chunk before it needed; only a chunk that does not fit (the
  // first one always) costs a second call.
  template <typename F>
  void Stream(std::ostream &out, int64_t entries, F call) {
    const int64_t chunk = (int64_t)(SBX_TEXT_CHUNK_ENTRIES);
    for (int64_t b = 0; b < entries; b += chunk) Chunk(out, b, std::min<int64_t>(chunk, entries - b), call);
  }
  // one chunk of a caller that cuts its chunks itself (the METIS graph writer: rows of unequal length)
  template <typename F>
  void Chunk(std::ostream &out, int64_t begin, int64_t count, F call) {
    int64_t bytes = 0;
    int rc = call(begin, count, (void *)d_text_, cap_, &bytes);
    if ((d_text_ == nullptr || rc == SBX_ERR_BAD_ARG) && bytes > cap_) {
      Reserve(bytes + bytes / 8);
      rc = call(begin, count, (void *)d_text_, cap_, &bytes);
    }
    WriterCheck(dev_, rc);
    Flush(out, bytes);
  }
  // a text that one call produces whole (the array format): formatted first, so that a refusal comes before any file
  template <typename F>
  int64_t Format(F call) {
    int64_t bytes = 0;
    WriterCheck(dev_, call(nullptr, 0, &bytes));
    if (bytes > cap_) Reserve(bytes);
    if (bytes) WriterCheck(dev_, call((void *)d_text_, cap_, &bytes));
    return bytes;
  }
  void Flush(std::ostream &out, int64_t bytes) {
    if (bytes <= 0) return;
    dev_.ToHost(h_text_, d_text_, (size_t)bytes);
    out.write(h_text_, (std::streamsize)bytes);
  }

 private:
  void Reserve(int64_t bytes) {
    dev_.Free(d_text_);
    dev_.HostFree(h_text_);
    d_text_ = nullptr;
    h_text_ = nullptr;
    cap_ = 0;
    d_text_ = static_cast<char *>(dev_.Malloc((size_t)bytes));
    h_text_ = static_cast<char *>(dev_.HostMalloc((size_t)bytes));
    cap_ = bytes;
  }
  const hip::Device &dev_;
  char *d_text_ = nullptr, *h_text_ = nullptr;
  int64_t cap_ = 0;
};

// the entries of a device CSR as device COO arrays in (row, col) order, the way the reference's CSR -> COO conversion
// and the COO constructor behind it leave them (converter_order_two.cc; format/coo.cc:96-157): the row ids are
// expanded into a scratch array; columns and values are the CSR's own arrays unless a row is out of order, in which
// case sorted copies are made.  The CSR is never modified.
template <typename IDType, typename NNZType, typename ValueType>
struct CsrAsCoo {
  const hip::Device &dev;
  IDType *row = nullptr, *col_copy = nullptr;
  void *val_copy = nullptr;
  const IDType *col = nullptr;
  const void *val = nullptr;
  CsrAsCoo(const hip::Device &d, int64_t n, int64_t m, int64_t nnz, const NNZType *row_ptr, const IDType *csr_col,
           const void *csr_val)
      : dev(d), col(csr_col), val(csr_val) {
    constexpr size_t vb = hip::ValueBytes<ValueType>();
    row = static_cast<IDType *>(dev.Malloc((size_t)nnz * sizeof(IDType)));
    try {
      WriterCheck(dev, sbx_csr_to_coo(dev.handle(), hip::IndexTag<IDType, NNZType>(), hip::ValueTag<ValueType>(), n, m, nnz,
                                      row_ptr, nullptr, nullptr, row, nullptr, nullptr, SBX_FLAG_MOVE));
      int sorted = 1;
      if (nnz > 1) WriterCheck(dev, sbx_coo_is_sorted(dev.handle(), hip::IndexTag<IDType, NNZType>(), nnz, row, csr_col, &sorted));
      if (!sorted) {
        col_copy = static_cast<IDType *>(dev.Malloc((size_t)nnz * sizeof(IDType)));
        dev.Copy(col_copy, csr_col, (size_t)nnz * sizeof(IDType));
        if (vb && csr_val) {
          val_copy = dev.Malloc((size_t)nnz * vb);
          dev.Copy(val_copy, csr_val, (size_t)nnz * vb);
        }
        WriterCheck(dev, sbx_coo_sort(dev.handle(), hip::IndexTag<IDType, NNZType>(), hip::ValueTag<ValueType>(), n, m, nnz, row,
                                      col_copy, val_copy));
        col = col_copy;
        val = val_copy;
      }
    } catch (...) {
      Release();
      throw;
    }
  }
  ~CsrAsCoo() { Release(); }
  CsrAsCoo(const CsrAsCoo &) = delete;
  CsrAsCoo &operator=(const CsrAsCoo &) = delete;

 private:
  void Release() {
    dev.Free(row);
    dev.Free(col_copy);
    dev.Free(val_copy);
    row = col_copy = nullptr;
    val_copy = nullptr;
  }
};

}  // namespace sparsebase::io::detail
#endif
