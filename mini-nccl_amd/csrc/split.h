// split.h -- the plan of ncclCommSplit (mini_nccl_ext.h), as a pure function.
//
// Every rank of the parent publishes (color, key) over the parent's bootstrap star and runs this
// on the same n pairs, so every rank computes the same plan without another word: ranks of one
// color >= 0 form one group; within it the new ranks follow the key, ascending, ties broken by
// the rank in the parent; the group's leader -- its new rank 0, which opens the child's
// bootstrap star -- is named by its parent rank.  A rank whose color is kSplitNoColor is in no
// group.  Header-only, like p2p.h / varblock.h: the simulator library exports it
// (sim.cpp mnccl_split_plan) and tests/native/split_selftest.cpp runs it under the sanitizers.
#pragma once
#include <stdint.h>

namespace mnccl {

constexpr int kSplitNoColor = -1;  // NCCL_SPLIT_NOCOLOR

struct SplitSlot {
  int32_t size;    // ranks in this rank's group; 0: none (kSplitNoColor)
  int32_t rank;    // its rank in the group; -1: none
  int32_t leader;  // parent rank of the group's new rank 0; -1: none
};

// colors[r] < 0 other than kSplitNoColor is the caller's error (api.cpp refuses it before any rank
// is contacted); here such a rank is in no group, like kSplitNoColor.  O(n^2): n <= kMaxRanks.
inline void split_plan(int n, const int32_t* colors, const int32_t* keys, SplitSlot* out) {
  for (int r = 0; r < n; ++r) {
    SplitSlot s{0, -1, -1};
    if (colors[r] >= 0) {
      // the leader: the member that no other member comes before
      int lead = r;
      for (int q = 0; q < n; ++q) {
        if (colors[q] != colors[r]) continue;
        ++s.size;
        // q comes before r: a smaller key, or the same key and a smaller parent rank
        if (keys[q] < keys[r] || (keys[q] == keys[r] && q < r)) ++s.rank;
        if (keys[q] < keys[lead] || (keys[q] == keys[lead] && q < lead)) lead = q;
      }
      ++s.rank;  // (from -1: the members before r)
      s.leader = lead;
    }
    out[r] = s;
  }
}

}  // namespace mnccl
