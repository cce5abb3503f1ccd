// meepo_mixed_plan.h — the class bookkeeping of a mixed group (SPEC.md §3 "Mixed groups"): plain host C++, no HIP, so that it can be
// compiled and tested on its own.  A class = the members that share one dim4; classes ordered by ascending dim4, members inside a class
// in the caller's order; member j's B bag rows are one [B, dim_j] block and the blocks follow each other class by class.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mee {

struct MixedPlan {
    std::vector<uint32_t> cls, rank;      // per member: its class and its rank among the class's members
    std::vector<uint64_t> off4;           // per member: the sum of dim4 over the blocks before its own (block start = B * off4 float4)
    std::vector<uint32_t> class_dim4;     // per class, ascending
    std::vector<uint32_t> class_size;     // per class: number of members
    std::vector<uint64_t> class_off4;     // per class: off4 of its first member
    std::vector<std::vector<uint32_t>> class_members;   // per class: the members, caller's order
    uint64_t total4 = 0;                  // the sum of dim4 over all members: the output holds B * total4 float4
};

inline MixedPlan mixed_plan(const uint32_t* dim4, uint32_t n) {
    MixedPlan p;
    p.cls.assign(n, 0); p.rank.assign(n, 0); p.off4.assign(n, 0);
    p.class_dim4.assign(dim4, dim4 + n);
    std::sort(p.class_dim4.begin(), p.class_dim4.end());
    p.class_dim4.erase(std::unique(p.class_dim4.begin(), p.class_dim4.end()), p.class_dim4.end());
    const size_t nc = p.class_dim4.size();
    p.class_size.assign(nc, 0); p.class_off4.assign(nc, 0); p.class_members.assign(nc, {});
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t c = (uint32_t)(std::lower_bound(p.class_dim4.begin(), p.class_dim4.end(), dim4[j]) - p.class_dim4.begin());
        p.cls[j] = c; p.rank[j] = p.class_size[c]++;
        p.class_members[c].push_back(j);
    }
    for (size_t c = 0; c < nc; ++c) {
        p.class_off4[c] = p.total4;
        p.total4 += (uint64_t)p.class_size[c] * p.class_dim4[c];
    }
    for (uint32_t j = 0; j < n; ++j) p.off4[j] = p.class_off4[p.cls[j]] + (uint64_t)p.rank[j] * dim4[j];
    return p;
}

}  // namespace mee
