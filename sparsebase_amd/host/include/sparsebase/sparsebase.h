// Umbrella header of the MI355X-native reorder / convert / permute path.
#ifndef SPARSEBASE_SPARSEBASE_H_
#define SPARSEBASE_SPARSEBASE_H_
#include "sparsebase/bases/reorder_base.h"
#include "sparsebase/bases/graph_feature_base.h"
#include "sparsebase/context/cpu_context.h"
#include "sparsebase/context/hip_context.h"
#include "sparsebase/converter/converter_order_one.h"
#include "sparsebase/converter/converter_order_two.h"
#include "sparsebase/experiment/concrete_experiment.h"
#include "sparsebase/experiment/experiment_helper.h"
#include "sparsebase/experiment/experiment_type.h"
#include "sparsebase/format/array.h"
#include "sparsebase/feature/avg_degree.h"
#include "sparsebase/feature/avg_degree_column.h"
#include "sparsebase/feature/bandwidth.h"
#include "sparsebase/feature/bandwidth_profile.h"
#include "sparsebase/feature/coefficient_of_variation_degree_column.h"
#include "sparsebase/feature/degree_distribution.h"
#include "sparsebase/feature/degrees.h"
#include "sparsebase/feature/degrees_degree_distribution.h"
#include "sparsebase/feature/extractor.h"
#include "sparsebase/feature/feature_extractor.h"
#include "sparsebase/feature/geometric_avg_degree_column.h"
#include "sparsebase/feature/jaccard_weights.h"
#include "sparsebase/feature/max_degree.h"
#include "sparsebase/feature/max_degree_column.h"
#include "sparsebase/feature/median_degree_column.h"
#include "sparsebase/feature/min_degree.h"
#include "sparsebase/feature/min_degree_column.h"
#include "sparsebase/feature/min_max_avg_degree.h"
#include "sparsebase/feature/off_diag_block_nnz.h"
#include "sparsebase/feature/standard_deviation_degree_column.h"
#include "sparsebase/feature/triangle_count.h"
#include "sparsebase/feature/profile.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/csc.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/kernels/row_softmax.h"
#include "sparsebase/kernels/sddmm.h"
#include "sparsebase/kernels/spmm.h"
#include "sparsebase/kernels/spmm_transposed.h"
#include "sparsebase/kernels/spmv.h"
#include "sparsebase/reorder/boba_reorder.h"
#include "sparsebase/reorder/reorder_heatmap.h"
#include "sparsebase/reorder/slashburn_reorder.h"
#include "sparsebase/utils/logger.h"
#include "sparsebase/utils/symmetrize.h"
// last: the reader needs the complete conversion graph
#include "sparsebase/bases/iobase.h"
#include "sparsebase/io/metis_graph_reader.h"
#include "sparsebase/io/metis_graph_writer.h"
#include "sparsebase/io/patoh_reader.h"
#include "sparsebase/io/patoh_writer.h"
#include "sparsebase/object/object.h"

namespace sparsebase {
// pre-0.3 spelling used by north_star / older call sites (SURVEY.md "Naming drift")
namespace preprocess {
template <typename IDType>
using Reorder = reorder::Reorderer<IDType>;
template <typename IDType>
using ReorderPreprocessType = reorder::Reorderer<IDType>;
template <typename I, typename N, typename V>
using RCMReorder = reorder::RCMReorder<I, N, V>;
template <typename I, typename N, typename V>
using DegreeReorder = reorder::DegreeReorder<I, N, V>;
template <typename I, typename N, typename V>
using GrayReorder = reorder::GrayReorder<I, N, V>;
}  // namespace preprocess
}  // namespace sparsebase
#endif
