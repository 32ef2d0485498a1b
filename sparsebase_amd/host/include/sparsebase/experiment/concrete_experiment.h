// ConcreteExperiment — the harness itself (reference: experiment/concrete_experiment.h:17-103 and
// concrete_experiment.cc:5-90), header-only.  The id strings are part of the behaviour:
//
//   file id              "-" + name for each file name of the target, concatenated
//   result / run time    file_id,pid,kid,i      one key per repetition i; a second Run appends to the same keys
//   auxiliary            name,file_id           what the loader returned
//                        name,file_id,pid       what a preprocess added — stored only while name,file_id is absent
//
// AddPreprocess and AddKernel keep the first function registered under an id.  Run times are std::chrono seconds around
// the kernel call alone: a kernel function that enqueues work on a device synchronises before it returns
// (experiment::SpMV does).  As in the reference, the harness frees nothing a loader or a preprocess returned: with
// store_auxiliary the caller finds every format under GetAuxiliary(), and owns it.
#ifndef SPARSEBASE_EXPERIMENT_CONCRETE_EXPERIMENT_H_
#define SPARSEBASE_EXPERIMENT_CONCRETE_EXPERIMENT_H_
#include "sparsebase/experiment/experiment_type.h"

namespace sparsebase::experiment {

class ConcreteExperiment : public ExperimentType {
 public:
  void Run(unsigned int times = 1, bool store_auxiliary = false) override {
    for (size_t l = 0; l < dataLoaders_.size(); l++) {
      for (auto &[file_names, file_param] : targets_[l]) {
        auto data = dataLoaders_[l](file_names);
        std::string file_id;
        for (const auto &name : file_names) file_id += "-" + name;
        if (store_auxiliary)
          for (const auto &d : data) auxiliary_[d.first + "," + file_id] = d.second;
        for (auto &[pid, preprocess] : preprocesses_) {
          preprocess.first(data, file_param, preprocess.second);
          for (auto &[kid, kernel] : kernels_) {
            for (unsigned int i = 0; i < times; i++) {
              const auto start = std::chrono::high_resolution_clock::now();
              std::any res = kernel.first(data, file_param, preprocess.second, kernel.second);
              const auto end = std::chrono::high_resolution_clock::now();
              const std::string id = file_id + "," + pid + "," + kid + "," + std::to_string(i);
              results_[id].push_back(std::move(res));
              runtimes_[id].push_back(std::chrono::duration<double>(end - start).count());
            }
          }
          if (store_auxiliary)
            for (const auto &d : data)
              if (auxiliary_.find(d.first + "," + file_id) == auxiliary_.end())
                auxiliary_[d.first + "," + file_id + "," + pid] = d.second;
        }
      }
    }
  }
  void AddDataLoader(LoadDataFunction func, std::vector<std::pair<std::vector<std::string>, std::any>> targets) override {
    targets_.push_back(std::move(targets));
    dataLoaders_.emplace_back(std::move(func));
  }
  void AddPreprocess(std::string id, PreprocessFunction func, std::any params) override {
    preprocesses_.insert(std::make_pair(std::move(id), std::make_pair(std::move(func), std::move(params))));
  }
  void AddKernel(std::string id, KernelFunction func, std::any params) override {
    kernels_.insert(std::make_pair(std::move(id), std::make_pair(std::move(func), std::move(params))));
  }
  std::map<std::string, std::vector<double>> GetRunTimes() override { return runtimes_; }
  std::map<std::string, std::vector<std::any>> GetResults() override { return results_; }
  std::map<std::string, std::any> GetAuxiliary() override { return auxiliary_; }

 protected:
  std::vector<std::vector<std::pair<std::vector<std::string>, std::any>>> targets_;  // per loader: its targets
  std::vector<LoadDataFunction> dataLoaders_;
  std::unordered_map<std::string, std::pair<PreprocessFunction, std::any>> preprocesses_;
  std::unordered_map<std::string, std::pair<KernelFunction, std::any>> kernels_;
  std::map<std::string, std::any> auxiliary_;
  std::map<std::string, std::vector<double>> runtimes_;
  std::map<std::string, std::vector<std::any>> results_;
};

}  // namespace sparsebase::experiment
#endif
