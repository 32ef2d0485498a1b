// ExperimentType — the interface of the experiment harness: data x preprocessing x kernel, every kernel call timed
// (reference: experiment/experiment_type.h:24-118).
#ifndef SPARSEBASE_EXPERIMENT_EXPERIMENT_TYPE_H_
#define SPARSEBASE_EXPERIMENT_EXPERIMENT_TYPE_H_
#include <any>
#include <chrono>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "sparsebase/format/format.h"
#include "sparsebase/format/format_order_one.h"
#include "sparsebase/format/format_order_two.h"

namespace sparsebase::experiment {

// file paths in, named formats out: everything an experiment works on comes from one of these
using LoadDataFunction =
    std::function<std::unordered_map<std::string, format::Format *>(std::vector<std::string> &file_paths)>;
// works on what the loader returned and adds to it; fparams belong to the file, params to the preprocess
using PreprocessFunction = std::function<void(std::unordered_map<std::string, format::Format *> &data, std::any &fparams,
                                              std::any &params)>;
// the timed call; what it returns is kept under the run's id
using KernelFunction = std::function<std::any(std::unordered_map<std::string, format::Format *> &data, std::any &fparams,
                                              std::any &pparams, std::any &kparams)>;

class ExperimentType {
 public:
  // every target through every preprocess, every kernel `times` times on each; store_auxiliary keeps what loaders and
  // preprocesses produced
  virtual void Run(unsigned int times, bool store_auxiliary) = 0;
  // targets: (file paths, file-specific parameters) pairs, each loaded by `func`
  virtual void AddDataLoader(LoadDataFunction func,
                             std::vector<std::pair<std::vector<std::string>, std::any>> targets) = 0;
  virtual void AddPreprocess(std::string id, PreprocessFunction func, std::any params) = 0;
  virtual void AddKernel(std::string id, KernelFunction func, std::any params) = 0;
  virtual std::map<std::string, std::vector<double>> GetRunTimes() = 0;
  virtual std::map<std::string, std::vector<std::any>> GetResults() = 0;
  virtual std::map<std::string, std::any> GetAuxiliary() = 0;
  virtual ~ExperimentType() = default;
};

}  // namespace sparsebase::experiment
#endif
