// ReorderHeatmap (reference: reorder/reorder_heatmap.h, reorder_heatmap.cc:43-119) over sbx_csr_reorder_heatmap: the
// share of the nonzeros in each cell of a num_parts x num_parts grid once the rows and columns are placed by two
// orders, as a host Array<FloatType> of num_parts^2 values (cell [i][j] at i * num_parts + j).  Registered for
// (CSR, Array, Array), staged through the default device, and (HIPCSR, HIPArray, HIPArray); other inputs go through
// the converter.  The rule and where the device differs from the reference are in include/sbx.h.
#ifndef SPARSEBASE_REORDER_REORDER_HEATMAP_H_
#define SPARSEBASE_REORDER_REORDER_HEATMAP_H_
#include <memory>
#include <type_traits>
#include <vector>

#include "sparsebase/format/csr.h"
#include "sparsebase/format/format_order_one.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/reorder/reorderer.h"
#include "sparsebase/utils/exception.h"
#include "sparsebase/utils/function_matcher_mixin.h"
#include "sparsebase/utils/parameterizable.h"

namespace sparsebase::reorder {

//! Parameters for Reorder Heatmap generator
struct ReorderHeatmapParams : utils::Parameters {
  //! Number of parts to split vertices over
  int num_parts = 3;
  ReorderHeatmapParams(int b) : num_parts(b) {}
  ReorderHeatmapParams() {}
};

template <typename IDType, typename NNZType, typename ValueType, typename FloatType>
class ReorderHeatmap : public utils::FunctionMatcherMixin<format::FormatOrderOne<FloatType> *> {
  static_assert(std::is_same_v<FloatType, float> || std::is_same_v<FloatType, double>,
                "FloatType must be float or double");

 public:
  ReorderHeatmap() {
    this->params_ = std::make_unique<ReorderHeatmapParams>();
    this->RegisterFunction({format::CSR<IDType, NNZType, ValueType>::get_id_static(),
                            format::Array<IDType>::get_id_static(), format::Array<IDType>::get_id_static()},
                           ReorderHeatmapCSRArrayArray);
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static(),
                            format::HIPArray<IDType>::get_id_static(), format::HIPArray<IDType>::get_id_static()},
                           ReorderHeatmapHIPCSRHIPArrayHIPArray);
  }
  ReorderHeatmap(ReorderHeatmapParams params) : ReorderHeatmap() {
    this->params_ = std::make_unique<ReorderHeatmapParams>(params);
  }
  //! The heatmap as a host Array<FloatType> the caller owns
  format::FormatOrderOne<FloatType> *Get(format::FormatOrderTwo<IDType, NNZType, ValueType> *format,
                                         format::FormatOrderOne<IDType> *permutation_r,
                                         format::FormatOrderOne<IDType> *permutation_c,
                                         std::vector<context::Context *> contexts, bool convert_input) {
    return this->Execute(this->params_.get(), contexts, convert_input, (format::Format *)format,
                         (format::Format *)permutation_r, (format::Format *)permutation_c);
  }

 protected:
  static format::FormatOrderOne<FloatType> *Run(hip::Device &dev, int64_t n, int64_t m, int64_t nnz,
                                                const NNZType *row_ptr, const IDType *col, const IDType *order_r,
                                                const IDType *order_c, utils::Parameters *poly_params) {
    const int b = static_cast<ReorderHeatmapParams *>(poly_params)->num_parts;
    if (b < 1 || b > n || b > m)
      throw utils::ReorderException("Cannot generate heatmap for matrix when num_parts > number of rows or columns");
    const size_t cells = (size_t)b * (size_t)b;
    hip::Staged<FloatType> d_heat(dev, cells);
    dev.Check(sbx_csr_reorder_heatmap(dev.handle(), hip::IndexTag<IDType, NNZType>(), n, m, nnz, row_ptr, col, order_r,
                                      order_c, (int64_t)b, (int)sizeof(FloatType), d_heat.get()));
    return new format::Array<FloatType>((format::DimensionType)cells, dev.Download(d_heat.get(), cells), format::kOwned);
  }
  static format::FormatOrderOne<FloatType> *ReorderHeatmapCSRArrayArray(std::vector<format::Format *> formats,
                                                                        utils::Parameters *poly_params) {
    auto *csr = formats[0]->AsAbsolute<format::CSR<IDType, NNZType, ValueType>>();
    auto *ar = formats[1]->AsAbsolute<format::Array<IDType>>();
    auto *ac = formats[2]->AsAbsolute<format::Array<IDType>>();
    const int64_t n = (int64_t)csr->get_dimensions()[0], m = (int64_t)csr->get_dimensions()[1];
    const int b = static_cast<ReorderHeatmapParams *>(poly_params)->num_parts;
    if (b < 1 || b > n || b > m)  // (before anything is staged)
      throw utils::ReorderException("Cannot generate heatmap for matrix when num_parts > number of rows or columns");
    auto v = detail::DeviceCsrView<IDType, NNZType, ValueType>::Stage(csr, false);
    auto &dev = *v.dev;
    IDType *d_r = nullptr, *d_c = nullptr;
    format::FormatOrderOne<FloatType> *out = nullptr;
    try {
      d_r = dev.Upload(ar->get_vals(), (size_t)n);
      d_c = dev.Upload(ac->get_vals(), (size_t)m);
      out = Run(dev, n, m, v.nnz, v.row_ptr, v.col, d_r, d_c, poly_params);
    } catch (...) {
      if (d_r) dev.Free(d_r);
      if (d_c) dev.Free(d_c);
      v.Release();
      throw;
    }
    dev.Free(d_r);
    dev.Free(d_c);
    v.Release();
    return out;
  }
  static format::FormatOrderOne<FloatType> *ReorderHeatmapHIPCSRHIPArrayHIPArray(std::vector<format::Format *> formats,
                                                                                utils::Parameters *poly_params) {
    auto *csr = formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
    auto *ar = formats[1]->AsAbsolute<format::HIPArray<IDType>>();
    auto *ac = formats[2]->AsAbsolute<format::HIPArray<IDType>>();
    return Run(csr->device(), (int64_t)csr->get_dimensions()[0], (int64_t)csr->get_dimensions()[1],
               (int64_t)csr->get_num_nnz(), csr->get_row_ptr(), csr->get_col(), ar->get_vals(), ac->get_vals(),
               poly_params);
  }
};

}  // namespace sparsebase::reorder
#endif
