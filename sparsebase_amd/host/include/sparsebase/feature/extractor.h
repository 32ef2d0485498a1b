// sparsebase/feature/extractor.h — feature::Extractor: add the features you want, get all of them from one Extract call
// that runs the fewest registered classes (reference: feature/extractor.h:16-86, extractor.cc:10-93).  A subclass
// registers the classes it can run (feature/feature_extractor.h); the choice among them is utils::ClassMatcherMixin's.
//
// Ownership, which the reference leaves open (it deletes the added features in its destructor, never the registered
// classes, and its own idiom `Extractor engine = FeatureExtractor<...>();` copies the raw pointers of a temporary):
// the registered classes and the added features are held through shared_ptr, next to the raw-pointer map the matcher
// works on.  A copy of an Extractor — the slice of that idiom included — shares the instances with its source and
// every instance is freed with its last holder.  What is shared is never mutated except for the params a match hands
// to a registered class, so copies that extract different things do not disturb each other's results.
//
// No device header is included here: a program that only matches classes links nothing of the device library.
#ifndef SPARSEBASE_FEATURE_EXTRACTOR_H_
#define SPARSEBASE_FEATURE_EXTRACTOR_H_
#include <any>
#include <iostream>
#include <memory>
#include <typeindex>
#include <unordered_map>
#include <vector>

#include "sparsebase/utils/class_matcher_mixin.h"
#include "sparsebase/utils/exception.h"
#include "sparsebase/utils/extractable.h"
#include "sparsebase/utils/utils.h"

namespace sparsebase::feature {

using Feature = utils::Implementation<utils::Extractable>;

class Extractor : public utils::ClassMatcherMixin<utils::Extractable *> {
  typedef utils::ClassMatcherMixin<utils::Extractable *> Matcher;

 public:
  typedef std::unordered_map<std::type_index, std::any> FeatureMap;
  virtual ~Extractor() = default;

  // every feature of `features` on its own, the maps merged: the first writer of a key stays (a value that loses is
  // dropped as it is; if it is a pointer nobody frees it, so ask for a feature once)
  static FeatureMap Extract(std::vector<Feature> &features, format::Format *format,
                            const std::vector<context::Context *> &contexts, bool convert_input) {
    FeatureMap res;
    for (auto &f : features) {
      FeatureMap one = f->Extract(format, contexts, convert_input);
      res.merge(one);
    }
    return res;
  }
  // the added features, through the classes GetClasses() names
  FeatureMap Extract(format::Format *format, const std::vector<context::Context *> &contexts, bool convert_input) {
    FeatureMap res;
    for (utils::Extractable *cls : GetClasses()) {
      FeatureMap one = cls->Extract(format, contexts, convert_input);
      res.merge(one);
    }
    return res;
  }

  // adds the sub-features of `f`; throws utils::FeatureException if no class is registered under f's get_sub_ids()
  void Add(Feature f) {
    if (map_.find(f->get_sub_ids()) == map_.end())
      throw utils::FeatureException(utils::demangle(f->get_id()), utils::demangle(typeid(*this)));
    for (utils::Extractable *sub : f->get_subs()) {
      std::shared_ptr<utils::Extractable> owned(sub);  // (freed here if the id is there already)
      in_.insert({owned->get_id(), owned});
    }
  }
  void Subtract(Feature f) {
    for (auto id : f->get_sub_ids()) in_.erase(id);
  }
  std::vector<std::type_index> GetList() {
    std::vector<std::type_index> res;
    for (auto &el : in_) res.push_back(el.first);
    return res;
  }
  // the classes the next Extract runs, in the order it runs them (owned by the extractor)
  std::vector<utils::Extractable *> GetClasses() {
    if (in_.empty()) return {};
    std::unordered_map<std::type_index, utils::Extractable *> source;
    for (auto &el : in_) source.insert({el.first, el.second.get()});
    return Matcher::GetClasses(source);
  }
  // the registered classes (owned by the extractor)
  std::vector<utils::Extractable *> GetFuncList() {
    std::vector<utils::Extractable *> res;
    for (auto &cls : map_) res.push_back(cls.second);
    return res;
  }
  void PrintFuncList() {
    std::cout << std::endl << "Registered functions: " << std::endl;
    for (auto &cls : map_) {
      for (auto id : cls.first) std::cout << utils::demangle(id) << " ";
      std::cout << "-> " << utils::demangle(cls.second->get_id()) << std::endl;
    }
    std::cout << std::endl;
  }

 protected:
  Extractor() = default;
  // takes `cls` over; registered under `ids`, which are sorted (get_sub_ids() of every feature class is)
  void RegisterClass(std::vector<std::type_index> ids, utils::Extractable *cls) {
    registered_.emplace_back(cls);
    Matcher::RegisterClass(std::move(ids), cls);
  }

 private:
  std::vector<std::shared_ptr<utils::Extractable>> registered_;
  std::unordered_map<std::type_index, std::shared_ptr<utils::Extractable>> in_;
};

}  // namespace sparsebase::feature
#endif
