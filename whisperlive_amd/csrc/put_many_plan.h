// put_many_plan.h — the host arithmetic of wlx_pcm_put_many (put_many.hip) that needs no device: which entries share the scratch
// (sub-batches under a byte budget), where the workgroups of the ragged resample launch start (tile prefix), and the verdict on an
// entry's FLAC status words. Plain C++: tests/put_many_plan_check.cpp runs it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wlx {

constexpr size_t PUT_MANY_BUDGET = 256u << 20;      // bytes of device scratch one wlx_pcm_put_many call may hold (wlx_debug_put_many_budget)
constexpr size_t PUT_MANY_MIN_BUDGET = 64u << 10;

inline size_t pm_up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct PutBatch { int first, last; size_t bytes; };   // entries [first, last) share the scratch; bytes = the sum of their needs

// need[k]: scratch bytes of entry k; live[k] == 0: the entry enqueues nothing (refused or damaged on the host) and belongs to no batch's
// sum. An entry that is alone over the budget is marked in over[k] and takes no part. The others, in order: a batch is closed in front
// of the entry that would take its sum past the budget, so every batch holds at least one entry and none exceeds the budget.
inline std::vector<PutBatch> put_many_pack(const std::vector<size_t>& need, const std::vector<char>& live, size_t budget,
                                           std::vector<char>& over) {
    const int n = (int)need.size();
    over.assign((size_t)n, 0);
    std::vector<PutBatch> out;
    PutBatch cur{0, 0, 0};
    bool open = false;
    for (int k = 0; k < n; ++k) {
        if (!live[(size_t)k]) continue;
        if (need[(size_t)k] > budget) { over[(size_t)k] = 1; continue; }
        if (open && need[(size_t)k] > budget - cur.bytes) {
            out.push_back(cur);
            open = false;
        }
        if (!open) { cur = PutBatch{k, k, 0}; open = true; }
        cur.bytes += need[(size_t)k];
        cur.last = k + 1;
    }
    if (open) out.push_back(cur);
    return out;
}

// first_tile[k] of the ragged resample launch: entry k owns workgroups [first_tile[k], first_tile[k + 1]); -> the grid, or -1 when it
// would pass 2^31 - 1 workgroups
inline long long put_many_tiles(const std::vector<long long>& n_out, const std::vector<int>& tile, std::vector<int>& first_tile) {
    long long at = 0;
    first_tile.assign(n_out.size(), 0);
    for (size_t k = 0; k < n_out.size(); ++k) {
        first_tile[k] = (int)at;
        if (n_out[k] > 0 && tile[k] > 0) at += (n_out[k] + tile[k] - 1) / tile[k];
        if (at > 0x7FFFFFFFLL) return -1;
    }
    return at;
}

// the first frame of status[0 .. n) whose low byte is not 0 (flac_core.h FLAC_OK), or -1
inline long long put_many_first_bad(const int* status, size_t n) {
    for (size_t f = 0; f < n; ++f)
        if ((status[f] & 0xFF) != 0) return (long long)f;
    return -1;
}

}  // namespace wlx
