// sparsebase/feature/degree_stats.h — what the eleven degree-statistic features share (avg_degree.h, min_degree.h,
// max_degree.h, min_max_avg_degree.h and the seven *_degree_column.h): one call of sbxstat_degree_stats
// (include/sbx_stats.h) on a CSR's row_ptr or a CSC's col_ptr, on the device, and the value computed on the host from
// the exact integers it returns.  Every feature registers two implementations: the host format is staged through the
// default device, its HIP twin runs in place.
//
// With F the feature type, each operation sequence is the definition:
//   Avg                     (F)sum / (F)n, the division in F                       bit-identical to the reference
//   Min, Max                NNZType(min), NNZType(max)                             bit-identical
//   Median                  n even: F((F)(median_lo + median_hi) / 2.0), n odd: F(median_hi)      bit-identical
//   StandardDeviation       T = (double)N / (double)n with N = n * sumsq - sum^2 exact in 128 bits; (F)sqrt(T)
//   CoefficientOfVariation  (F)(sqrt(T) / ((double)sum / (double)n))
//   GeometricAvg            zeros > 0: (F)0 (the reference's exp(-inf)), else (F)exp(sum_log / (double)n)
// The last three cannot be bit-identical: the reference accumulates in F, row after row, and no parallel sum repeats
// that.  They come from exact integers instead and lie closer to the true value than the reference does.
// Like the reference's, "StandardDeviation" is the root of the sum of squared deviations, not divided by n.
#ifndef SPARSEBASE_FEATURE_DEGREE_STATS_H_
#define SPARSEBASE_FEATURE_DEGREE_STATS_H_
#include <cmath>
#include <string>
#include <tuple>

#include "sbx_stats.h"
#include "sparsebase/feature/feature_preprocess_type.h"
#include "sparsebase/format/csc.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/format/hip_formats.h"

namespace sparsebase::feature::detail {

// An offset array of n + 1 words on a device: borrowed from an HIP format, or staged from a host one.
template <typename N>
struct DevicePtrView {
  hip::Device *dev = nullptr;
  int64_t n = 0;
  N *ptr = nullptr;
  bool staged = false;

  static DevicePtrView Borrow(hip::Device &d, N *device_ptr, int64_t n) {
    DevicePtrView v;
    v.dev = &d;
    v.n = n;
    v.ptr = device_ptr;
    return v;
  }
  static DevicePtrView Stage(const N *host_ptr, int64_t n) {
    DevicePtrView v;
    v.dev = &hip::Device::Get(hip::DefaultDevice());
    v.n = n;
    v.ptr = v.dev->Upload(host_ptr, (size_t)n + 1);
    v.staged = true;
    return v;
  }
  void Release() {
    if (staged) dev->Free(ptr);
    staged = false;
  }
};

template <typename N>
sbxstat_degrees RunDegreeStats(DevicePtrView<N> v, unsigned flags) {
  sbxstat_degrees s;
  const int rc = sbxstat_degree_stats(v.dev->handle(), sizeof(N) == 4 ? SBX_I32 : SBX_I64, v.n, v.ptr, flags, &s);
  v.Release();
  v.dev->Check(rc);
  return s;
}

// the degrees of a CSR's rows
struct OverRows {
  template <typename I, typename N, typename V> using Host = format::CSR<I, N, V>;
  template <typename I, typename N, typename V> using Device = format::HIPCSR<I, N, V>;
  template <typename I, typename N, typename V>
  static sbxstat_degrees Stats(format::Format *f, bool on_device, unsigned flags) {
    const int64_t n = (int64_t)f->get_dimensions()[0];
    if (n == 0) throw utils::FeatureException("a degree statistic of a matrix without rows is not defined");
    if (on_device) {
      auto *d = f->AsAbsolute<format::HIPCSR<I, N, V>>();
      return RunDegreeStats(DevicePtrView<N>::Borrow(d->device(), d->get_row_ptr(), n), flags);
    }
    return RunDegreeStats(DevicePtrView<N>::Stage(f->AsAbsolute<format::CSR<I, N, V>>()->get_row_ptr(), n), flags);
  }
};

// the degrees of a CSC's columns.  The count is get_dimensions()[0], as in the reference (*_degree_column.cc): the row
// count, a quirk that is reproduced where it is defined (dims[0] <= dims[1]); where the reference reads past col_ptr
// (dims[0] > dims[1]) the feature is an exception here.
struct OverColumns {
  template <typename I, typename N, typename V> using Host = format::CSC<I, N, V>;
  template <typename I, typename N, typename V> using Device = format::HIPCSC<I, N, V>;
  template <typename I, typename N, typename V>
  static sbxstat_degrees Stats(format::Format *f, bool on_device, unsigned flags) {
    const int64_t n = (int64_t)f->get_dimensions()[0], m = (int64_t)f->get_dimensions()[1];
    if (n == 0) throw utils::FeatureException("a degree statistic of a matrix without columns is not defined");
    if (n > m)
      throw utils::FeatureException("column degree statistics count get_dimensions()[0] columns: not defined for " +
                                    std::to_string(n) + " rows and " + std::to_string(m) + " columns");
    if (on_device) {
      auto *d = f->AsAbsolute<format::HIPCSC<I, N, V>>();
      return RunDegreeStats(DevicePtrView<N>::Borrow(d->device(), d->get_col_ptr(), n), flags);
    }
    return RunDegreeStats(DevicePtrView<N>::Stage(f->AsAbsolute<format::CSC<I, N, V>>()->get_col_ptr(), n), flags);
  }
};

// ---- the values (the header comment's table) ---------------------------------------------------------------------
template <typename F>
F StatAvg(const sbxstat_degrees &s) {
  return (F)s.sum / (F)s.count;
}
template <typename F>
F StatMedian(const sbxstat_degrees &s) {
  if (s.count % 2 == 0) return F((F)(s.median_lo + s.median_hi) / 2.0);
  return F(s.median_hi);
}
// T = (n * sumsq - sum^2) / n: the sum of squared deviations from the mean
inline double StatSquaredDeviations(const sbxstat_degrees &s) {
  typedef unsigned __int128 u128;
  const u128 sumsq = ((u128)s.sumsq_hi << 64) | s.sumsq_lo, n = (u128)s.count;
  if (sumsq > ((((u128)1) << 127) - 1) / n)
    throw utils::FeatureException("the sum of squared degrees times the count does not fit 127 bits");
  const u128 N = n * sumsq - (u128)s.sum * (u128)s.sum;  // >= 0 (Cauchy-Schwarz)
  return (double)N / (double)s.count;
}
template <typename F>
F StatStandardDeviation(const sbxstat_degrees &s) {
  return (F)std::sqrt(StatSquaredDeviations(s));
}
template <typename F>
F StatCoefficientOfVariation(const sbxstat_degrees &s) {
  return (F)(std::sqrt(StatSquaredDeviations(s)) / ((double)s.sum / (double)s.count));
}
template <typename F>
F StatGeometricAvg(const sbxstat_degrees &s) {
  if (s.zeros > 0) return (F)0;
  return (F)std::exp(s.sum_log / (double)s.count);
}

// The façade every single-valued statistic shares (the one of feature/bandwidth.h).  Derived supplies
//   static constexpr unsigned kFlags                      what sbxstat_degree_stats has to fill
//   static Result *Compute(const sbxstat_degrees &)       the value, a `new Result` the caller deletes
// and the reference's names Get<Feature>, Get<Feature>Cached and Get<Feature>CSR / CSC, which forward here.
template <typename Derived, typename Axis, typename Result, typename Params, typename I, typename N, typename V>
class DegreeStatistic : public FeaturePreprocessType<Result *> {
 public:
  typedef Params ParamsType;
  DegreeStatistic() {
    Register();
    this->params_ = std::shared_ptr<ParamsType>(new ParamsType());
    this->pmap_.insert({get_id_static(), this->params_});
  }
  DegreeStatistic(ParamsType) : DegreeStatistic() {}
  DegreeStatistic(const DegreeStatistic &d) {
    Register();
    this->params_ = d.params_;
    this->pmap_ = d.pmap_;
  }
  DegreeStatistic(std::shared_ptr<ParamsType> p) {
    Register();
    this->params_ = p;
    this->pmap_[get_id_static()] = p;
  }
  ~DegreeStatistic() override = default;

  std::unordered_map<std::type_index, std::any> Extract(format::Format *format, std::vector<context::Context *> c,
                                                        bool convert_input) override {
    return {{this->get_id(), std::forward<Result *>(Get(format, c, convert_input))}};
  }
  std::vector<std::type_index> get_sub_ids() override { return {typeid(Derived)}; }
  std::vector<utils::Extractable *> get_subs() override { return {new Derived(static_cast<const Derived &>(*this))}; }
  static std::type_index get_id_static() { return typeid(Derived); }

 protected:
  Result *Get(format::Format *format, std::vector<context::Context *> c, bool convert_input) {
    return this->Execute(this->params_.get(), c, convert_input, format);
  }
  std::tuple<std::vector<std::vector<format::Format *>>, Result *> GetCached(format::Format *format,
                                                                             std::vector<context::Context *> c,
                                                                             bool convert_input) {
    return this->CachedExecute(this->params_.get(), c, convert_input, false, format);
  }
  void Register() {
    this->RegisterFunction({Axis::template Host<I, N, V>::get_id_static()}, OnHost);
    this->RegisterFunction({Axis::template Device<I, N, V>::get_id_static()}, OnDevice);
  }
  static Result *OnHost(std::vector<format::Format *> formats, utils::Parameters *) {
    return Derived::Compute(Axis::template Stats<I, N, V>(formats[0], false, Derived::kFlags));
  }
  static Result *OnDevice(std::vector<format::Format *> formats, utils::Parameters *) {
    return Derived::Compute(Axis::template Stats<I, N, V>(formats[0], true, Derived::kFlags));
  }
};

}  // namespace sparsebase::feature::detail
#endif
