// Loaders, preprocess functions and the SpMV, SpMM, SDDMM and RowSoftmax kernel functions for experiment::ConcreteExperiment (reference:
// experiment/experiment_helper.h:21-124 for LoadFormat ... Reorder; the rest is this project's own).
//
//   LoadFormat / LoadCSR / LoadCOO / LoadCSC   file_names[0] through ReaderType into data["format"]
//   ReorderCSR / Reorder / Pass                data["processed_format"] from data["format"]
//   LoadHIPCSR / ReorderHIP                    the device-resident twins: an HIPCSR on device SBX_DEVICE in and out, so that
//                                              no kernel call of the canonical pipeline pays a trip over PCIe
//   SpMV<I, N, V, F>                           the KernelFunction: y = A x on the device (kernels/spmv.h)
//   SpMM<I, N, V, F>                           the KernelFunction: Y = A X for k columns on the device (kernels/spmm.h)
//   SpMMTransposed<I, N, V, F>                 the KernelFunction: Y = A^T X from a plan (kernels/spmm_transposed.h)
//   SDDMM<I, N, V, F>                          the KernelFunction: out = vals (.) (U V^T) on A's pattern (kernels/sddmm.h)
//   RowSoftmax<I, N, V, F>                     the KernelFunction: the softmax of every row's values (kernels/row_softmax.h)
//
// As in the reference, the ContextType of ReorderCSR and Reorder is default-constructed: that is CPUContext, whose
// formats the host layer stages through the device as it does everywhere.
#ifndef SPARSEBASE_EXPERIMENT_EXPERIMENT_HELPER_H_
#define SPARSEBASE_EXPERIMENT_EXPERIMENT_HELPER_H_
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "sparsebase/bases/reorder_base.h"
#include "sparsebase/experiment/experiment_type.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/csc.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"
#include "sparsebase/kernels/row_softmax.h"
#include "sparsebase/kernels/sddmm.h"
#include "sparsebase/kernels/spmm.h"
#include "sparsebase/kernels/spmm_transposed.h"
#include "sparsebase/kernels/spmv.h"

namespace sparsebase::experiment {

using DataMap = std::unordered_map<std::string, format::Format *>;

template <template <typename, typename, typename> typename FormatType,
          template <typename, typename, typename> typename ReaderType, typename IDType, typename NNZType,
          typename ValueType>
DataMap LoadFormat(std::vector<std::string> &file_names) {
  auto reader = ReaderType<IDType, NNZType, ValueType>(file_names[0]);
  std::unique_ptr<format::COO<IDType, NNZType, ValueType>> coo(reader.ReadCOO());
  auto *format = coo->template Convert<FormatType>();
  if ((format::Format *)format == (format::Format *)coo.get()) coo.release();  // (FormatType is COO: the same object)
  return {{"format", format}};
}

template <template <typename, typename, typename> typename ReaderType, typename IDType, typename NNZType,
          typename ValueType>
DataMap LoadCSR(std::vector<std::string> &file_names) {
  return {{"format", ReaderType<IDType, NNZType, ValueType>(file_names[0]).ReadCSR()}};
}

template <template <typename, typename, typename> typename ReaderType, typename IDType, typename NNZType,
          typename ValueType>
DataMap LoadCOO(std::vector<std::string> &file_names) {
  return {{"format", ReaderType<IDType, NNZType, ValueType>(file_names[0]).ReadCOO()}};
}

template <template <typename, typename, typename> typename ReaderType, typename IDType, typename NNZType,
          typename ValueType>
DataMap LoadCSC(std::vector<std::string> &file_names) {
  return LoadFormat<format::CSC, ReaderType, IDType, NNZType, ValueType>(file_names);
}

// the CSR of file_names[0] in the HBM of device SBX_DEVICE
template <template <typename, typename, typename> typename ReaderType, typename IDType, typename NNZType,
          typename ValueType>
DataMap LoadHIPCSR(std::vector<std::string> &file_names) {
  context::HIPContext gpu(hip::DefaultDevice());
  std::unique_ptr<format::CSR<IDType, NNZType, ValueType>> csr(
      ReaderType<IDType, NNZType, ValueType>(file_names[0]).ReadCSR());
  return {{"format", csr->template Convert<format::HIPCSR>(&gpu)}};
}

// data["processed_format"] = P A P^T as a CSR, P the order ReorderType gives for data["format"] (a FormatType)
template <template <typename, typename, typename> typename ReorderType,
          template <typename, typename, typename> typename FormatType, typename ContextType, typename IDType,
          typename NNZType, typename ValueType>
void Reorder(DataMap &data, std::any fparams, std::any params) {
  ContextType context;
  auto p = std::any_cast<typename ReorderType<IDType, NNZType, ValueType>::ParamsType>(params);
  auto *A = data["format"]->template AsAbsolute<FormatType<IDType, NNZType, ValueType>>();
  std::unique_ptr<IDType[]> perm(bases::ReorderBase::Reorder<ReorderType>(p, A, {&context}, true));
  auto *reordered = bases::ReorderBase::Permute2D<FormatType>(perm.get(), A, {&context}, true);
  auto *csr = reordered->template Convert<format::CSR>();
  if ((format::Format *)csr != (format::Format *)reordered) delete reordered;
  data["processed_format"] = csr;
}

template <template <typename, typename, typename> typename ReorderType, typename ContextType, typename IDType,
          typename NNZType, typename ValueType>
void ReorderCSR(DataMap &data, std::any fparams, std::any params) {
  Reorder<ReorderType, format::CSR, ContextType, IDType, NNZType, ValueType>(data, std::move(fparams), std::move(params));
}

// runs the kernels on the data as it was loaded
inline void Pass(DataMap &data, std::any fparams, std::any params) { data["processed_format"] = data["format"]; }

// Reorder's device-resident twin: data["format"] is an HIPCSR, the order vector and the permuted HIPCSR never leave HBM
template <template <typename, typename, typename> typename ReorderType, typename IDType, typename NNZType,
          typename ValueType>
void ReorderHIP(DataMap &data, std::any fparams, std::any params) {
  context::HIPContext gpu(hip::DefaultDevice());
  auto p = std::any_cast<typename ReorderType<IDType, NNZType, ValueType>::ParamsType>(params);
  auto *A = data["format"]->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
  std::unique_ptr<format::HIPArray<IDType>> perm(bases::ReorderBase::Reorder<ReorderType>(p, A, gpu, true));
  data["processed_format"] = bases::ReorderBase::Permute2D<format::HIPCSR>(perm.get(), A, {&gpu}, true);
}

namespace detail {
// a kernel function's array parameter on the device: an HIPArray is borrowed, a host Array staged
template <typename FloatType>
kernels::detail::DeviceVector<FloatType> OperandOf(std::any &param, const hip::Device &dev, const char *who, const char *what) {
  if (auto *d = std::any_cast<format::HIPArray<FloatType>>(&param))
    return kernels::detail::DeviceVector<FloatType>::Borrow(d, dev, what);
  if (auto *h = std::any_cast<format::Array<FloatType>>(&param)) return kernels::detail::DeviceVector<FloatType>::Stage(h, dev);
  throw utils::TypeException(std::string(who) + what + " must be an Array or an HIPArray of the kernel's FloatType");
}
}  // namespace detail

// The SpMV KernelFunction, with the contract of the reference example's kernels
// (examples/example_experiment/example_experiment.cu:32-55): data["processed_format"] is a CSR or an HIPCSR of
// <IDType, NNZType, ValueType>; fparams holds x as an Array<FloatType> or an HIPArray<FloatType>; kparams holds the values
// the same way, or nothing (then the matrix's own values where ValueType is FloatType, else a pattern).  The result is a
// host FloatType* of n values from new[], owned by the caller, returned after the device has finished.  A host CSR and host
// arrays are staged on every call — that staging is inside the harness's timing, as the reference's cuda kernels have it;
// device-resident data (LoadHIPCSR, HIPArray parameters) pays the download of y alone.
template <typename IDType, typename NNZType, typename ValueType, typename FloatType>
std::any SpMV(DataMap &data, std::any &fparams, std::any &pparams, std::any &kparams) {
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;
  format::Format *A = data.at("processed_format");
  const bool resident = A->template IsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
  auto vector_of = [](std::any &param, const hip::Device &dev, const char *what) {
    return detail::OperandOf<FloatType>(param, dev, "experiment::SpMV: ", what);
  };
  const bool own_vals = !kparams.has_value() && std::is_same_v<ValueType, FloatType>;
  View v = resident ? View::Borrow(A->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>())
                    : View::Stage(A->template AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), own_vals);
  utils::detail::CsrViewGuard<IDType, NNZType, ValueType> guard{v};
  auto x = vector_of(fparams, *v.dev, "x (the file's parameter)");
  kernels::detail::DeviceVector<FloatType> vals;
  if (kparams.has_value()) vals = vector_of(kparams, *v.dev, "the values (the kernel's parameter)");
  const size_t n = (size_t)v.n;
  hip::Staged<FloatType> d_y(*v.dev, n ? n : 1);
  kernels::detail::Multiply(v, x, kparams.has_value() ? &vals : nullptr, d_y.get());
  FloatType *y = new FloatType[n ? n : 1];
  try {
    d_y.ToHost(y);  // (a blocking copy behind the kernels on the handle's stream: the synchronise)
  } catch (...) {
    delete[] y;
    throw;
  }
  return y;
}

// The kernel parameter of SpMM: the number of columns of X and, optionally, the values (an Array<FloatType> or an
// HIPArray<FloatType>; empty: the matrix's own values where ValueType is FloatType, else a pattern).
struct SpMMParams {
  size_t k = 1;
  std::any vals;
};

// The SpMM KernelFunction, with SpMV's contract: data["processed_format"] is a CSR or an HIPCSR of <IDType, NNZType,
// ValueType>; fparams holds X, m * k values row-major, as an Array<FloatType> or an HIPArray<FloatType>; kparams holds an
// SpMMParams.  The result is a host FloatType* of n * k values from new[], owned by the caller, returned after the device
// has finished.  Host data is staged on every call, inside the harness's timing; device-resident data pays the download of
// Y alone.
template <typename IDType, typename NNZType, typename ValueType, typename FloatType>
std::any SpMM(DataMap &data, std::any &fparams, std::any &pparams, std::any &kparams) {
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;
  auto *params = std::any_cast<SpMMParams>(&kparams);
  if (!params) throw utils::TypeException("experiment::SpMM: the kernel's parameter must be an SpMMParams");
  format::Format *A = data.at("processed_format");
  const bool resident = A->template IsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
  const bool has_vals = params->vals.has_value();
  const bool own_vals = !has_vals && std::is_same_v<ValueType, FloatType>;
  View v = resident ? View::Borrow(A->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>())
                    : View::Stage(A->template AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), own_vals);
  utils::detail::CsrViewGuard<IDType, NNZType, ValueType> guard{v};
  auto x = detail::OperandOf<FloatType>(fparams, *v.dev, "experiment::SpMM: ", "X (the file's parameter)");
  kernels::detail::DeviceVector<FloatType> vals;
  if (has_vals) vals = detail::OperandOf<FloatType>(params->vals, *v.dev, "experiment::SpMM: ", "the values (the kernel's parameter)");
  const size_t count = (size_t)v.n * params->k;
  hip::Staged<FloatType> d_y(*v.dev, count ? count : 1);
  kernels::detail::MultiplyBlock(v, x, params->k, has_vals ? &vals : nullptr, d_y.get());
  FloatType *y = new FloatType[count ? count : 1];
  try {
    d_y.ToHost(y);  // (a blocking copy behind the kernels on the handle's stream: the synchronise)
  } catch (...) {
    delete[] y;
    throw;
  }
  return y;
}

// The kernel parameter of SpMMTransposed: the number of columns of X, optionally the values (an Array<FloatType> or an
// HIPArray<FloatType> in the matrix's CSR order; empty: a pattern, the plan holds no values) and optionally a plan, a
// std::shared_ptr<kernels::TransposePlan<IDType, NNZType>> built from the format the kernel will see (empty: the plan is
// built inside every call, a sort of all stored entries inside the harness's timing).
struct SpMMTransposedParams {
  size_t k = 1;
  std::any vals;
  std::any plan;
};

// The SpMMTransposed KernelFunction, with SpMM's contract: data["processed_format"] is a CSR or an HIPCSR of <IDType,
// NNZType, ValueType>; fparams holds X, n * k values row-major, as an Array<FloatType> or an HIPArray<FloatType>; kparams
// holds an SpMMTransposedParams.  The result is a host FloatType* of m * k values from new[], owned by the caller,
// returned after the device has finished.
template <typename IDType, typename NNZType, typename ValueType, typename FloatType>
std::any SpMMTransposed(DataMap &data, std::any &fparams, std::any &pparams, std::any &kparams) {
  typedef kernels::TransposePlan<IDType, NNZType> Plan;
  auto *params = std::any_cast<SpMMTransposedParams>(&kparams);
  if (!params) throw utils::TypeException("experiment::SpMMTransposed: the kernel's parameter must be an SpMMTransposedParams");
  std::shared_ptr<Plan> plan;
  if (params->plan.has_value()) {
    auto *given = std::any_cast<std::shared_ptr<Plan>>(&params->plan);
    if (!given || !*given)
      throw utils::TypeException("experiment::SpMMTransposed: the plan must be a shared_ptr to a TransposePlan of the kernel's index types");
    plan = *given;
  } else {
    format::Format *A = data.at("processed_format");
    if (A->template IsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>())
      plan = std::make_shared<Plan>(A->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>());
    else
      plan = std::make_shared<Plan>(A->template AsAbsolute<format::CSR<IDType, NNZType, ValueType>>());
  }
  hip::Device &dev = plan->device();
  auto x = detail::OperandOf<FloatType>(fparams, dev, "experiment::SpMMTransposed: ", "X (the file's parameter)");
  const bool has_vals = params->vals.has_value();
  kernels::detail::DeviceVector<FloatType> vals;
  if (has_vals)
    vals = detail::OperandOf<FloatType>(params->vals, dev, "experiment::SpMMTransposed: ", "the values (the kernel's parameter)");
  const size_t count = (size_t)plan->columns() * params->k;
  hip::Staged<FloatType> d_y(dev, count ? count : 1);
  kernels::detail::MultiplyTransposed(*plan, x, params->k, has_vals ? &vals : nullptr, d_y.get());
  FloatType *y = new FloatType[count ? count : 1];
  try {
    d_y.ToHost(y);  // (a blocking copy behind the kernels on the handle's stream: the synchronise)
  } catch (...) {
    delete[] y;
    throw;
  }
  return y;
}

// The kernel parameter of SDDMM: the number of columns of U and V, U (n * k values row-major, an Array<FloatType> or an
// HIPArray<FloatType>) and, optionally, the values (the same two types; empty: the matrix's own values where ValueType is
// FloatType, else a pattern).
struct SDDMMParams {
  size_t k = 1;
  std::any u;
  std::any vals;
};

// The SDDMM KernelFunction, with SpMM's contract: data["processed_format"] is a CSR or an HIPCSR of <IDType, NNZType,
// ValueType>; fparams holds V, m * k values row-major, as an Array<FloatType> or an HIPArray<FloatType>; kparams holds an
// SDDMMParams.  The result is a host FloatType* of nnz values from new[], owned by the caller, returned after the device
// has finished.  Host data is staged on every call, inside the harness's timing; device-resident data pays the download of
// the result alone.
template <typename IDType, typename NNZType, typename ValueType, typename FloatType>
std::any SDDMM(DataMap &data, std::any &fparams, std::any &pparams, std::any &kparams) {
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;
  auto *params = std::any_cast<SDDMMParams>(&kparams);
  if (!params) throw utils::TypeException("experiment::SDDMM: the kernel's parameter must be an SDDMMParams");
  format::Format *A = data.at("processed_format");
  const bool resident = A->template IsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
  const bool has_vals = params->vals.has_value();
  const bool own_vals = !has_vals && std::is_same_v<ValueType, FloatType>;
  View v = resident ? View::Borrow(A->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>())
                    : View::Stage(A->template AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), own_vals);
  utils::detail::CsrViewGuard<IDType, NNZType, ValueType> guard{v};
  auto x = detail::OperandOf<FloatType>(fparams, *v.dev, "experiment::SDDMM: ", "V (the file's parameter)");
  auto u = detail::OperandOf<FloatType>(params->u, *v.dev, "experiment::SDDMM: ", "U (the kernel's parameter)");
  kernels::detail::DeviceVector<FloatType> vals;
  if (has_vals) vals = detail::OperandOf<FloatType>(params->vals, *v.dev, "experiment::SDDMM: ", "the values (the kernel's parameter)");
  const size_t count = (size_t)v.nnz;
  hip::Staged<FloatType> d_out(*v.dev, count ? count : 1);
  kernels::detail::SampleBlock(v, u, x, params->k, has_vals ? &vals : nullptr, d_out.get());
  FloatType *out = new FloatType[count ? count : 1];
  try {
    d_out.ToHost(out);  // (a blocking copy behind the kernel on the handle's stream: the synchronise)
  } catch (...) {
    delete[] out;
    throw;
  }
  return out;
}

// The RowSoftmax KernelFunction, with SDDMM's contract: data["processed_format"] is a CSR or an HIPCSR of <IDType, NNZType,
// ValueType>; kparams holds the values, one per stored entry, as an Array<FloatType> or an HIPArray<FloatType>, or nothing
// (then the matrix's own values where ValueType is FloatType, else a pattern: 1 / the entries of the row); fparams is not
// read.  The result is a host FloatType* of nnz values from new[], owned by the caller, returned after the device has
// finished.  Host data is staged on every call, inside the harness's timing; device-resident data pays the download of the
// result alone.
template <typename IDType, typename NNZType, typename ValueType, typename FloatType>
std::any RowSoftmax(DataMap &data, std::any &fparams, std::any &pparams, std::any &kparams) {
  typedef reorder::detail::DeviceCsrView<IDType, NNZType, ValueType> View;
  format::Format *A = data.at("processed_format");
  const bool resident = A->template IsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>();
  const bool has_vals = kparams.has_value();
  const bool own_vals = !has_vals && std::is_same_v<ValueType, FloatType>;
  View v = resident ? View::Borrow(A->template AsAbsolute<format::HIPCSR<IDType, NNZType, ValueType>>())
                    : View::Stage(A->template AsAbsolute<format::CSR<IDType, NNZType, ValueType>>(), own_vals);
  utils::detail::CsrViewGuard<IDType, NNZType, ValueType> guard{v};
  kernels::detail::DeviceVector<FloatType> vals;
  if (has_vals) vals = detail::OperandOf<FloatType>(kparams, *v.dev, "experiment::RowSoftmax: ", "the values (the kernel's parameter)");
  const size_t count = (size_t)v.nnz;
  hip::Staged<FloatType> d_out(*v.dev, count ? count : 1);
  kernels::detail::NormalizeRows(v, has_vals ? &vals : nullptr, d_out.get());
  FloatType *out = new FloatType[count ? count : 1];
  try {
    d_out.ToHost(out);  // (a blocking copy behind the kernels on the handle's stream: the synchronise)
  } catch (...) {
    delete[] out;
    throw;
  }
  return out;
}

}  // namespace sparsebase::experiment
#endif
