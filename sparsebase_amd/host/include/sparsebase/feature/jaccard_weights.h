// sparsebase/feature/jaccard_weights.h — feature::JaccardWeights (reference: feature/jaccard_weights.h:15-45,
// .cc:11-50, jaccard_weights_cuda.cu:14-60).  As in the reference, the only registered key is the device CSR
// (HIPCSR, the counterpart of CUDACSR, .cc:31-37): a host CSR runs after conversion when convert_input is true, throws
// DirectExecutionNotAvailableException when it is false, and FunctionNotFoundException with no HIP context at all.
// The weights stay on the device, as a HIPArray<FeatureType> of one weight per nonzero (sbx_csr_jaccard_weights).
#ifndef SPARSEBASE_FEATURE_JACCARD_WEIGHTS_H_
#define SPARSEBASE_FEATURE_JACCARD_WEIGHTS_H_
#include <type_traits>
#include <vector>

#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/utils/function_matcher_mixin.h"
#include "sparsebase/utils/parameterizable.h"

namespace sparsebase::feature {
//! An empty struct used for the parameters of JaccardWeights
struct JaccardWeightsParams : utils::Parameters {};

template <typename IDType, typename NNZType, typename ValueType, typename FeatureType>
class JaccardWeights : public utils::FunctionMatcherMixin<format::Format *> {
  static_assert(std::is_same_v<FeatureType, float> || std::is_same_v<FeatureType, double>,
                "FeatureType must be float or double");

 public:
  typedef JaccardWeightsParams ParamsType;
  JaccardWeights() {
    this->RegisterFunction({format::HIPCSR<IDType, NNZType, ValueType>::get_id_static()}, GetJaccardWeightHIPCSR);
  }
  JaccardWeights(ParamsType) : JaccardWeights() {}
  ~JaccardWeights() = default;

  //! The Jaccard weight of every nonzero of the graph `format` represents, as a 1D format (HIPArray<FeatureType>)
  format::Format *GetJaccardWeights(format::Format *format, std::vector<context::Context *> contexts,
                                    bool convert_input) {
    return this->Execute(nullptr, contexts, convert_input, format);
  }

  //! formats[0] is a HIPCSR; returns a HIPArray<FeatureType> on its device (element i: weight of the i-th nonzero)
  static format::Format *GetJaccardWeightHIPCSR(std::vector<format::Format *> formats, utils::Parameters *) {
    auto *csr = formats[0]->AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
    auto &dev = csr->device();
    const int64_t n = (int64_t)csr->get_dimensions()[0], nnz = (int64_t)csr->get_num_nnz();
    FeatureType *w = nnz ? static_cast<FeatureType *>(dev.Malloc((size_t)nnz * sizeof(FeatureType))) : nullptr;
    const int rc = sbx_csr_jaccard_weights(dev.handle(), hip::IndexTag<IDType, NNZType>(), n, nnz, csr->get_row_ptr(),
                                           csr->get_col(), (int)sizeof(FeatureType), w);
    if (rc != SBX_OK && w) dev.Free(w);
    dev.Check(rc);
    return new format::HIPArray<FeatureType>((format::DimensionType)nnz, w, *csr->get_hip_context(), format::kOwned);
  }
};

}  // namespace sparsebase::feature
#endif
