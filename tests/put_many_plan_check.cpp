// Stand-alone check of csrc/put_many_plan.h on the host (tests/test_put_many_host.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it as a child process): the sub-batch packing, the tile prefix of the ragged resample launch
// and the status verdict of wlx_pcm_put_many, on fixed cases and on seeded random ones checked against their defining properties.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "../whisperlive_amd/csrc/put_many_plan.h"

using namespace wlx;

static int fails = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) { ++fails; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

static void check_pack(const std::vector<size_t>& need, const std::vector<char>& live, size_t budget) {
    std::vector<char> over;
    const std::vector<PutBatch> b = put_many_pack(need, live, budget, over);
    const int n = (int)need.size();
    EXPECT((int)over.size() == n);
    std::vector<int> seen((size_t)n, 0);
    int at = 0;
    for (size_t i = 0; i < b.size(); ++i) {
        EXPECT(b[i].first >= at && b[i].first < b[i].last && b[i].last <= n);      // in order, disjoint, not empty
        size_t sum = 0;
        int members = 0;
        for (int k = b[i].first; k < b[i].last; ++k)
            if (live[(size_t)k] && !over[(size_t)k]) { sum += need[(size_t)k]; ++seen[(size_t)k]; ++members; }
        EXPECT(members >= 1 && sum == b[i].bytes && sum <= budget);
        EXPECT(live[(size_t)b[i].first] && !over[(size_t)b[i].first]);               // a batch starts at a member ...
        if (i + 1 < b.size()) {                                                        // ... and was closed only because the next did not fit
            int nx = b[i + 1].first;
            EXPECT(need[(size_t)nx] > budget - sum);
        }
        at = b[i].last;
    }
    for (int k = 0; k < n; ++k) {
        EXPECT(over[(size_t)k] == (live[(size_t)k] && need[(size_t)k] > budget ? 1 : 0));
        EXPECT(seen[(size_t)k] == (live[(size_t)k] && !over[(size_t)k] ? 1 : 0));       // every member exactly once
    }
}

int main() {
    {   // the fixed cases
        std::vector<char> over;
        std::vector<PutBatch> b = put_many_pack({100, 200, 300, 50}, {1, 1, 1, 1}, 300, over);
        EXPECT(b.size() == 3 && b[0].first == 0 && b[0].last == 2 && b[0].bytes == 300 && b[1].first == 2 && b[1].last == 3 && b[2].bytes == 50);
        b = put_many_pack({100, 400, 0, 100}, {1, 1, 1, 1}, 300, over);
        EXPECT(b.size() == 1 && over[1] == 1 && b[0].first == 0 && b[0].last == 4 && b[0].bytes == 200);
        b = put_many_pack({100, 100}, {0, 0}, 300, over);
        EXPECT(b.empty() && !over[0] && !over[1]);
        b = put_many_pack({}, {}, 300, over);
        EXPECT(b.empty() && over.empty());
        b = put_many_pack({0, 0, 0}, {1, 0, 1}, 64, over);
        EXPECT(b.size() == 1 && b[0].first == 0 && b[0].last == 3 && b[0].bytes == 0);
        EXPECT(pm_up256(0) == 0 && pm_up256(1) == 256 && pm_up256(256) == 256 && pm_up256(257) == 512);
    }
    std::mt19937_64 rng(20261020);
    for (int it = 0; it < 20000; ++it) {
        const int n = (int)(rng() % 65);
        const size_t budget = 1 + rng() % 5000;
        std::vector<size_t> need((size_t)n);
        std::vector<char> live((size_t)n);
        for (int k = 0; k < n; ++k) {
            need[(size_t)k] = rng() % 7 == 0 ? 0 : rng() % (budget + budget / 3 + 2);
            live[(size_t)k] = rng() % 5 != 0;
        }
        check_pack(need, live, budget);
    }
    {   // the tile prefix
        std::vector<int> first;
        EXPECT(put_many_tiles({1, 1024, 1025, 0, 64}, {1024, 1024, 1024, 512, 64}, first) == 5);
        EXPECT(first.size() == 5 && first[0] == 0 && first[1] == 1 && first[2] == 2 && first[3] == 4 && first[4] == 4);
        EXPECT(put_many_tiles({}, {}, first) == 0 && first.empty());
        EXPECT(put_many_tiles({57600000, 57600000}, {64, 64}, first) == 1800000 && first[1] == 900000);
        std::vector<long long> big(64, 16000LL * 3600);
        std::vector<int> one(64, 1);
        EXPECT(put_many_tiles(big, one, first) == -1);                    // 64 x 57.6 M workgroups: refused, not wrapped
        for (int it = 0; it < 2000; ++it) {
            const size_t n = rng() % 65;
            std::vector<long long> no(n);
            std::vector<int> tile(n);
            long long want = 0;
            for (size_t k = 0; k < n; ++k) { no[k] = (long long)(rng() % 100000); tile[k] = 64 << (rng() % 5); }
            const long long grid = put_many_tiles(no, tile, first);
            for (size_t k = 0; k < n; ++k) { EXPECT(first[k] == want); want += (no[k] + tile[k] - 1) / tile[k]; }
            EXPECT(grid == want);
        }
    }
    {   // the status verdict
        const int ok[4] = {0, 0x800, 0xA00, 0x900};                       // FLAC_OK with a channel assignment above the low byte
        const int bad[4] = {0, 0x800, 0xA04, 1};
        EXPECT(put_many_first_bad(ok, 4) == -1 && put_many_first_bad(ok, 0) == -1);
        EXPECT(put_many_first_bad(bad, 4) == 2 && put_many_first_bad(bad + 3, 1) == 0 && put_many_first_bad(bad, 2) == -1);
    }
    printf("put_many_plan_check: %d failures\n", fails);
    return fails ? 1 : 0;
}
