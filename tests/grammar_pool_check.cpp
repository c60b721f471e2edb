// grammar_pool_check.cpp — csrc/grammar_pool.h under the host sanitizers (tests/test_grammar_items_host.py compiles this with
// -fsanitize=address,undefined and runs it): a good set packs to the layout dec_grammar_items_kernel reads, every violation is refused
// with a message, and the check reads nothing past the arrays (each is a heap block of exactly the size the format gives it).
#include <string>
#include <vector>
#include "../whisperlive_amd/csrc/grammar_pool.h"
using namespace wlx;
typedef std::vector<int32_t> Ints;
static int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { ++fails; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

struct Set {
    int V = 60000, eot = 50257;
    Ints ns, off, tok, next, accept;
    void add(const Ints& o, const Ints& t, const Ints& x, const Ints& a) {
        ns.push_back((int32_t)a.size());
        off.insert(off.end(), o.begin(), o.end()); tok.insert(tok.end(), t.begin(), t.end());
        next.insert(next.end(), x.begin(), x.end()); accept.insert(accept.end(), a.begin(), a.end());
    }
    bool check(std::string* why = nullptr, int* states = nullptr, int* edges = nullptr, int tables = -1) const {
        char msg[240] = "";
        Ints n(ns), o(off), t(tok), x(next), a(accept);          // exact-size heap copies: a read past an array is an ASan report
        const bool ok = grammar_pool_check(V, eot, tables < 0 ? (int)ns.size() : tables, n.data(), o.data(), t.empty() ? nullptr : t.data(),
                                           x.empty() ? nullptr : x.data(), a.data(), states, edges, msg, sizeof(msg));
        if (why) *why = msg;
        return ok;
    }
};
// the phrases a, a b c, b d with repeat (tests/grammar_table_check.cpp), a one-state table without edges, and a two-state table
static Set three() {
    Set s;
    s.add({0, 2, 4, 5, 7}, {1, 2, 1, 2, 4, 3, 4}, {1, 2, 1, 3, 0, 0, 0}, {1, 1, 0, 0});
    s.add({0, 0}, {}, {}, {1});
    s.add({0, 1, 2}, {7, 8}, {1, 0}, {0, 1});
    return s;
}
// `tables` tables of `states` states with `per` edges each
static Set uniform(int tables, int states, int per) {
    Set s;
    for (int t = 0; t < tables; ++t) {
        Ints o, k, x;
        for (int n = 0; n <= states; ++n) o.push_back(n * per);
        for (int n = 0; n < states; ++n)
            for (int i = 0; i < per; ++i) { k.push_back(i * 3 + n % 3); x.push_back((n + i) % states); }
        s.add(o, k, x, Ints((size_t)states, 0));
    }
    return s;
}
static void refused(const Set& s, const char* needle, int tables = -1) {
    std::string why;
    EXPECT(!s.check(&why, nullptr, nullptr, tables) && why.find(needle) != std::string::npos, needle);
}
int main() {
    {
        Set s = three();
        int states = 0, edges = 0;
        EXPECT(s.check(nullptr, &states, &edges) && states == 7 && edges == 9, "three tables pass");
        std::vector<int> block((size_t)GRAMMAR_POOL_INTS, -7);
        grammar_pool_pack(block.data(), 3, s.ns.data(), s.off.data(), s.tok.data(), s.next.data(), s.accept.data());
        const int hdr[12] = {0, 0, 4, 7, 4, 7, 1, 0, 5, 7, 2, 2};
        EXPECT(memcmp(block.data(), hdr, sizeof(hdr)) == 0 && block[14] == 0 && block[GRAMMAR_POOL_OFF_AT - 1] == 0, "headers; the unused slots are empty");
        EXPECT(memcmp(block.data() + GRAMMAR_POOL_OFF_AT, s.off.data(), 10 * 4) == 0, "offsets, local per table, table t at state base + t");
        EXPECT(memcmp(block.data() + GRAMMAR_POOL_TOK_AT, s.tok.data(), 9 * 4) == 0 && memcmp(block.data() + GRAMMAR_POOL_NEXT_AT, s.next.data(), 9 * 4) == 0 &&
               memcmp(block.data() + GRAMMAR_POOL_ACCEPT_AT, s.accept.data(), 7 * 4) == 0, "edges and accept flags");
        EXPECT(block[GRAMMAR_POOL_OFF_AT + 10] == -7 && block[GRAMMAR_POOL_TOK_AT + 9] == -7 && block[GRAMMAR_POOL_NEXT_AT + 9] == -7 &&
               block[GRAMMAR_POOL_ACCEPT_AT + 7] == -7 && GRAMMAR_POOL_OFF_AT % 4 == 0, "nothing past the used parts");
        EXPECT(uniform(64, 256, 4).check(nullptr, &states, &edges) && states == GRAMMAR_SET_MAX_STATES && edges == GRAMMAR_SET_MAX_EDGES, "the caps themselves pass");
    }
    refused(uniform(5, 4000, 1), "states in all");               // each table within its own limits
    refused(uniform(5, 1000, 16), "edges in all");
    refused(uniform(65, 1, 0), "tables outside");
    refused(three(), "tables outside", 0);
    { Set s = three(); s.next[8] = 2; refused(s, "table 2: "); }            // a state only another table has: numbers are local
    { Set s = three(); s.off[5] = 1; refused(s, "table 1: "); }
    { Set s = three(); s.ns[1] = 0; refused(s, "table 1 has 0 states"); }
    Set s = three();
    int32_t* arrays[5] = {s.ns.data(), s.off.data(), s.tok.data(), s.next.data(), s.accept.data()};
    for (int k = 0; k < 5; ++k) {               // a null array
        int32_t* a[5] = {arrays[0], arrays[1], arrays[2], arrays[3], arrays[4]};
        a[k] = nullptr;
        EXPECT(!grammar_pool_check(s.V, s.eot, 3, a[0], a[1], a[2], a[3], a[4], nullptr, nullptr, nullptr, 0), "a null array, no message buffer");
    }
    printf("grammar_pool_check: %d failures\n", fails);
    return fails ? 1 : 0;
}
