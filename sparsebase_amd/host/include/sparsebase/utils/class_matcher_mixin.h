// sparsebase/utils/class_matcher_mixin.h — picks, for a set of requested ids, the registered classes that compute them
// in the fewest passes (reference: utils/class_matcher_mixin.h:11-125).  A class is registered under the sorted ids it
// computes; a class registered under several ids is a fused one.
//
// The choice is the reference's: among the requested ids, sorted, the largest registered key wins; among keys of one
// size the first one in the order std::prev_permutation walks the selection masks (the selection of the smallest ids
// first); then the same on the remainder.  The merged class gets the params of every matched id through set_params.
//
// Two departures:
//   - the selection mask has the size of what is left to match, not of `source`: the reference indexes the shrinking
//     `ordered` with a mask as long as `source` (:45-54) and reads past the vector once a match leaves a remainder;
//   - the search starts at min(remaining ids, largest registered key), not at the number of requested ids: no larger
//     subset can be a key, so the choice is the same, and 2^N lookups become at most C(N, largest key) per class.
// Ids that no registered key covers end the search with a FeatureException (the reference recurses without end).
//
// No device header is included here: a program that matches classes links nothing of the device library.
#ifndef SPARSEBASE_UTILS_CLASS_MATCHER_MIXIN_H_
#define SPARSEBASE_UTILS_CLASS_MATCHER_MIXIN_H_
#include <algorithm>
#include <functional>
#include <string>
#include <tuple>
#include <typeindex>
#include <unordered_map>
#include <vector>

#include "sparsebase/utils/exception.h"
#include "sparsebase/utils/utils.h"

namespace sparsebase::utils {

template <class ClassType, typename Key = std::vector<std::type_index>, typename KeyHash = utils::TypeIndexVectorHash,
          typename KeyEqualTo = std::equal_to<std::vector<std::type_index>>>
class ClassMatcherMixin {
 protected:
  std::unordered_map<Key, ClassType, KeyHash, KeyEqualTo> map_;
  std::size_t largest_key_ = 0;  // ids of the largest registered key

  // the first registration of a key stays (unordered_map::insert, as in the reference)
  void RegisterClass(std::vector<std::type_index> instants, ClassType val) {
    largest_key_ = std::max(largest_key_, instants.size());
    map_.insert({instants, val});
  }

  // the first registered key among the K-subsets of `ordered`, and what it leaves; {nullptr, ordered} if there is none
  std::tuple<ClassType, std::vector<std::type_index>> MatchClass(std::unordered_map<std::type_index, ClassType> &source,
                                                                 std::vector<std::type_index> &ordered, unsigned int K) {
    const std::size_t N = ordered.size();
    if (K == 0 || K > N) return std::make_tuple(ClassType(nullptr), ordered);
    std::string mask(K, 1);  // K chosen ids, then N - K that are not
    mask.resize(N, 0);
    do {
      std::vector<std::type_index> chosen;
      for (std::size_t i = 0; i < N; ++i)
        if (mask[i]) chosen.push_back(ordered[i]);
      auto hit = map_.find(chosen);
      if (hit == map_.end()) continue;
      ClassType merged = hit->second;
      for (auto id : chosen) merged->set_params(id, source[id]->get_params());
      std::vector<std::type_index> rest;
      for (std::size_t i = 0; i < N; ++i)
        if (!mask[i]) rest.push_back(ordered[i]);
      return std::make_tuple(merged, rest);
    } while (std::prev_permutation(mask.begin(), mask.end()));
    return std::make_tuple(ClassType(nullptr), ordered);
  }

  void GetClassesHelper(std::unordered_map<std::type_index, ClassType> &source, std::vector<std::type_index> &ordered,
                        std::vector<ClassType> &res) {
    while (!ordered.empty()) {
      bool found = false;
      for (std::size_t c = std::min(ordered.size(), largest_key_); !found && c > 0; c--) {
        auto r = MatchClass(source, ordered, (unsigned int)c);
        if (std::get<0>(r)) {
          res.push_back(std::get<0>(r));
          ordered = std::get<1>(r);
          found = true;
        }
      }
      if (!found) throw FeatureException(demangle(ordered[0]), "the class matcher (no registered class computes it)");
    }
  }

  std::vector<ClassType> GetClasses(std::unordered_map<std::type_index, ClassType> &source) {
    std::vector<ClassType> res;
    std::vector<std::type_index> ordered;
    for (auto &el : source) ordered.push_back(el.first);
    std::sort(ordered.begin(), ordered.end());
    GetClassesHelper(source, ordered, res);
    return res;
  }
};

}  // namespace sparsebase::utils
#endif
