// pattern_pool_check.cpp — the pool functions of csrc/pattern_table.h under the host sanitizers (tests/test_pattern_items_host.py compiles
// and runs it): a good set packs to the layout dec_pattern_items_kernel reads, every table's cells start on a 16-byte boundary, every
// violation is refused with a message, and the check reads nothing past the arrays (each a heap block of exactly its format's size).
#include <string>
#include <vector>
#include "../whisperlive_amd/csrc/pattern_table.h"
using namespace wlx;
static int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { ++fails; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

struct Set {
    int V = 60000, eot = 50257;
    std::vector<int32_t> ns, nc;
    std::vector<uint8_t> cls, accept;
    std::vector<uint16_t> trans;
    // a table of n states x c classes: byte b has class b % c, state s moves to (s + class) % n, class c - 1 is dead, odd states accept
    void add(int n, int c) {
        ns.push_back(n); nc.push_back(c);
        for (int b = 0; b < 256; ++b) cls.push_back((uint8_t)(b % c));
        for (int s = 0; s < n; ++s) {
            for (int k = 0; k < c; ++k) trans.push_back(k == c - 1 && c > 1 ? (uint16_t)PATTERN_DEAD : (uint16_t)((s + k) % n));
            accept.push_back((uint8_t)(s & 1));
        }
    }
    bool check(std::string* why = nullptr, int* cells = nullptr, int* states = nullptr, int tables = -1) const {
        char msg[280] = "";
        std::vector<int32_t> n(ns), c(nc);                      // exact-size heap copies: a read past an array is an ASan report
        std::vector<uint8_t> k(cls), a(accept);
        std::vector<uint16_t> t(trans);
        const bool ok = pattern_pool_check(V, eot, tables < 0 ? (int)ns.size() : tables, n.data(), c.data(), k.data(), t.data(), a.data(), cells, states,
                                           msg, sizeof(msg));
        if (why) *why = msg;
        return ok;
    }
};
static Set of(std::initializer_list<std::pair<int, int>> shapes) {
    Set s;
    for (const auto& p : shapes) s.add(p.first, p.second);
    return s;
}
static Set uniform(int tables, int n, int c) {
    Set s;
    for (int t = 0; t < tables; ++t) s.add(n, c);
    return s;
}
static void refused(const Set& s, const char* needle, int tables = -1) {
    std::string why;
    EXPECT(!s.check(&why, nullptr, nullptr, tables) && why.find(needle) != std::string::npos, needle);
}
int main() {
    {
        // 1 x 1 in front (the next table would start at cell 1), 37 x 3 = 111 cells (the next at 119), the table at the cap, 5 x 2 behind it
        Set s = of({{1, 1}, {37, 3}, {4096, 6}, {5, 2}});
        int cells = 0, states = 0;
        EXPECT(s.check(nullptr, &cells, &states) && states == 1 + 37 + 4096 + 5 && cells == 120 + 24576 + 10, "four tables pass; the cells count the pads");
        std::vector<uint32_t> block((size_t)PATTERN_POOL_WORDS, 0xABABABABu);
        pattern_pool_pack(block.data(), 4, s.ns.data(), s.nc.data(), s.cls.data(), s.trans.data(), s.accept.data());
        const uint32_t hdr[16] = {0, 0, 1, 1, 8, 1, 37, 3, 120, 38, 4096, 6, 24696, 4134, 5, 2};
        EXPECT(memcmp(block.data(), hdr, sizeof(hdr)) == 0 && block[16] == 0 && block[PATTERN_POOL_CLASS_AT - 1] == 0, "headers; the unused slots are empty");
        EXPECT(memcmp(block.data() + PATTERN_POOL_CLASS_AT, s.cls.data(), 4 * 256) == 0 && block[PATTERN_POOL_CLASS_AT + 4 * 64] == 0xABABABABu, "class maps");
        const uint16_t* cl = reinterpret_cast<const uint16_t*>(block.data() + PATTERN_POOL_TRANS_AT);
        const uint8_t* ac = reinterpret_cast<const uint8_t*>(block.data() + PATTERN_POOL_ACCEPT_AT);
        int src = 0, sb = 0;
        for (int t = 0; t < 4; ++t) {
            const uint32_t* h = block.data() + 4 * t;
            const int n = s.ns[t] * s.nc[t];
            EXPECT(h[0] % 8 == 0 && (PATTERN_POOL_TRANS_AT * 4 + h[0] * 2) % 16 == 0, "every table's cells start on a 16-byte boundary");
            EXPECT(memcmp(cl + h[0], s.trans.data() + src, 2 * (size_t)n) == 0 && memcmp(ac + h[1], s.accept.data() + sb, (size_t)s.ns[t]) == 0, "cells and accept bytes");
            src += n; sb += s.ns[t];
        }
        EXPECT(cl[1] == 0 && cl[7] == 0 && cl[119] == 0 && cl[24706] == 0 && cl[24711] == 0 && cl[24712] == 0xABAB && ac[4139] == 0xAB, "pads are zero; nothing past the used parts");
        EXPECT(uniform(16, 4096, 6).check(nullptr, &cells, &states) && cells == PATTERN_SET_MAX_CELLS && states == PATTERN_SET_MAX_STATES, "the caps themselves pass");
        Set w = uniform(64, 1, 1);
        EXPECT(w.check(nullptr, &cells, &states) && cells == 63 * 8 + 1 && cells <= PATTERN_POOL_TRANS_CELLS, "64 tables, 63 pads");
        pattern_pool_pack(block.data(), 64, w.ns.data(), w.nc.data(), w.cls.data(), w.trans.data(), w.accept.data());
        EXPECT(block[63 * 4] == 63 * 8 && block[63 * 4 + 1] == 63, "the last slot's header");
    }
    refused(uniform(17, 4096, 6), "cells in all");              // each table within its own limits
    { Set s = uniform(16, 4096, 1); s.add(1, 1); refused(s, "states in all"); }
    refused(uniform(65, 1, 1), "tables outside");
    refused(of({{1, 1}, {2, 2}}), "tables outside", 0);
    { Set s = of({{1, 1}, {2, 2}}); s.ns[1] = 4097; refused(s, "table 1: pattern: 4097 states"); }     // (refused on the counts: the arrays stay short)
    { Set s = of({{1, 1}, {2, 2}}); s.ns[1] = 0; refused(s, "table 1: pattern: 0 states"); }
    { Set s = of({{1, 1}, {2, 2}}); s.nc[1] = 257; refused(s, "table 1: pattern: 257 byte classes"); }
    { Set s = of({{1, 1}, {2, 2}}); s.ns[1] = 3073; s.nc[1] = 8; refused(s, "table 1: pattern: 3073 states x 8 classes"); }
    { Set s = of({{1, 1}, {37, 3}, {2, 2}}); s.cls[256 + 7] = 3; refused(s, "table 1: pattern: byte 7 has class 3"); }
    { Set s = of({{1, 1}, {37, 3}, {2, 2}}); s.trans[1 + 4] = 37; refused(s, "table 1: pattern: state 1 moves to state 37"); }   // a state only another table has
    { Set s = of({{1, 1}, {37, 3}, {2, 2}}); s.accept[1 + 36] = 2; refused(s, "table 1: pattern: accept[36] is 2"); }
    { Set s = of({{1, 1}}); s.eot = s.V; refused(s, "eot"); }
    Set s = of({{1, 1}, {37, 3}});
    for (int k = 0; k < 5; ++k) {               // a null array
        const void* a[5] = {s.ns.data(), s.nc.data(), s.cls.data(), s.trans.data(), s.accept.data()};
        a[k] = nullptr;
        EXPECT(!pattern_pool_check(s.V, s.eot, 2, (const int32_t*)a[0], (const int32_t*)a[1], (const uint8_t*)a[2], (const uint16_t*)a[3], (const uint8_t*)a[4],
                                   nullptr, nullptr, nullptr, 0), "a null array, no message buffer");
    }
    printf("pattern_pool_check: %d failures\n", fails);
    return fails ? 1 : 0;
}
