// mvc_posterior_host.h — host-only pieces of the posterior summary
// (mvc_posterior.hip): the limits, the dish-id compaction of
// mvc_result_labels and the split of the draw pairs between the LDS and the
// global-scratch kernels.  Plain C++ (no HIP types), so a stand-alone program
// can exercise it under a host sanitizer (tests/posterior_host_check.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mvc.h"

namespace mvc {

constexpr int64_t kPostMaxCells = (int64_t)1 << 26;          // contingency cells of one pair (as mvc_ari.hip)
constexpr int kPostLdsCells = MVC_POSTERIOR_LDS_CELLS;       // table + margins of one pair in LDS (128 KiB)
constexpr int64_t kPostBatchCells = (int64_t)1 << 24;        // global scratch shared by one batch of pairs (64 MiB)
constexpr int64_t kPostMaxDraws = MVC_POSTERIOR_MAX_DRAWS;
constexpr int64_t kPostPsmMaxN = MVC_POSTERIOR_PSM_MAX_N;

// Raw dish ids of one draw's tables -> 0..K-1 in ascending raw id (rank
// preserving, so the relabelled draw is the same partition).  Returns K.
inline int compact_ids(const int32_t *raw, int64_t T, int32_t *out) {
  std::vector<int32_t> ids(raw, raw + T);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  for (int64_t t = 0; t < T; ++t)
    out[t] = (int32_t)(std::lower_bound(ids.begin(), ids.end(), raw[t]) - ids.begin());
  return (int)ids.size();
}

// Scratch words of the pair (ranges ra, rb): table, row margin, column margin.
inline int64_t pair_words(int64_t ra, int64_t rb) { return ra * rb + ra + rb; }

// One pair that goes through global scratch, and where its table starts.
struct GlobalPair {
  int32_t s, t;
  int64_t off;     // first scratch word of the pair within its batch
};
struct PairPlan {
  bool too_wide = false;             // some pair has more than kPostMaxCells cells
  int lds_words = 0;                 // dynamic LDS words the LDS kernel needs (0: no LDS pair)
  std::vector<GlobalPair> global;    // pairs beyond kPostLdsCells, s < t, row-major order
  std::vector<int64_t> batch_begin;  // batch b = global[batch_begin[b] .. batch_begin[b+1])
  int64_t scratch_words = 0;         // largest batch
};

// range[s] = max - min + 1 of draw s's labels (1 .. 2^32).
inline PairPlan plan_pairs(const std::vector<int64_t> &range, int64_t lds_limit = kPostLdsCells,
                           int64_t batch_limit = kPostBatchCells) {
  PairPlan P;
  const int64_t S = (int64_t)range.size();
  P.batch_begin.push_back(0);
  int64_t used = 0;
  for (int64_t s = 0; s < S; ++s)
    for (int64_t t = s + 1; t < S; ++t) {
      // ranges reach 2^32: compare by division, the product may not fit
      if (range[s] > kPostMaxCells / range[t]) {
        P.too_wide = true;
        return P;
      }
      const int64_t w = pair_words(range[s], range[t]);
      if (w <= lds_limit) {
        P.lds_words = (int)std::max<int64_t>(P.lds_words, w);
        continue;
      }
      if (used > 0 && used + w > batch_limit) {   // a batch holds at least one pair
        P.batch_begin.push_back((int64_t)P.global.size());
        used = 0;
      }
      P.global.push_back({(int32_t)s, (int32_t)t, used});
      used += w;
      P.scratch_words = std::max(P.scratch_words, used);
    }
  if (P.batch_begin.back() != (int64_t)P.global.size()) P.batch_begin.push_back((int64_t)P.global.size());
  return P;
}

}  // namespace mvc
