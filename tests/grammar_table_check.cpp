// grammar_table_check.cpp — csrc/grammar_table.h under the host sanitizers (tests/test_grammar_host.py compiles this with
// -fsanitize=address,undefined and runs it): good tables pass and pack to the layout the kernel reads, every violation of the format of
// include/wlx_grammar.h is refused with a message, and the check reads nothing past what the arrays hold (every array here is a heap
// block of exactly the size the format gives it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../whisperlive_amd/csrc/grammar_table.h"

using namespace wlx;

static int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { ++fails; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

struct Table {
    int V = 100, eot = 90, n = 0;
    std::vector<int32_t> off, tok, next, accept;
    bool check(std::string* why = nullptr) const {
        char msg[200] = "";
        // exact-size heap copies: a read past an array is an ASan report
        std::vector<int32_t> o(off), t(tok), x(next), a(accept);
        const bool ok = grammar_table_check(V, eot, n, o.data(), t.empty() ? nullptr : t.data(), x.empty() ? nullptr : x.data(), a.data(), msg, sizeof(msg));
        if (why) *why = msg;
        return ok;
    }
};

// the phrases a, a b c, b d with repeat, as whisperlive_amd/grammar.py determinises them
static Table abc() {
    Table g;
    g.n = 4;
    g.off = {0, 2, 4, 5, 7};
    g.tok = {1, 2, 1, 2, 4, 3, 4};
    g.next = {1, 2, 1, 3, 0, 0, 0};
    g.accept = {1, 1, 0, 0};
    return g;
}

static void refused(const Table& g, const char* needle, const char* what) {
    std::string why;
    const bool ok = g.check(&why);
    EXPECT(!ok, what);
    EXPECT(why.find(needle) != std::string::npos, what);
    if (ok || why.find(needle) == std::string::npos) printf("  (%s: got '%s', wanted '%s')\n", what, why.c_str(), needle);
}

int main() {
    {
        Table g = abc();
        std::string why;
        EXPECT(g.check(&why), "the a / a b c / b d table passes");
        std::vector<int> block((size_t)GRAMMAR_TABLE_INTS, -7);
        grammar_table_pack(block.data(), g.eot, g.n, g.off.data(), g.tok.data(), g.next.data(), g.accept.data());
        EXPECT(block[0] == 4 && block[1] == 7 && block[2] == 90 && block[3] == 0, "header");
        EXPECT(memcmp(block.data() + GRAMMAR_OFF_AT, g.off.data(), 5 * 4) == 0, "offsets");
        EXPECT(memcmp(block.data() + GRAMMAR_TOK_AT, g.tok.data(), 7 * 4) == 0, "tokens");
        EXPECT(memcmp(block.data() + GRAMMAR_NEXT_AT, g.next.data(), 7 * 4) == 0, "nexts");
        EXPECT(memcmp(block.data() + GRAMMAR_ACCEPT_AT, g.accept.data(), 4 * 4) == 0, "accept");
        EXPECT(block[GRAMMAR_OFF_AT + 5] == -7 && block[GRAMMAR_TOK_AT + 7] == -7 && block[GRAMMAR_ACCEPT_AT + 4] == -7, "nothing past the used parts");
        EXPECT(GRAMMAR_ACCEPT_AT + GRAMMAR_MAX_STATES == GRAMMAR_TABLE_INTS, "layout");
    }
    {   // one state without edges (only end-of-text survives); the caps themselves
        Table g;
        g.n = 1; g.off = {0, 0}; g.accept = {1};
        EXPECT(g.check(), "one state, no edges");
        Table full;
        full.V = 60000; full.eot = 50257; full.n = GRAMMAR_MAX_STATES;
        full.off.assign((size_t)GRAMMAR_MAX_STATES + 1, 0);
        for (int n = 0; n <= GRAMMAR_MAX_STATES; ++n) full.off[(size_t)n] = 4 * n;
        for (int i = 0; i < GRAMMAR_MAX_EDGES; ++i) { full.tok.push_back((i % 4) * 1000 + i / 4); full.next.push_back(i % GRAMMAR_MAX_STATES); }
        full.accept.assign((size_t)GRAMMAR_MAX_STATES, 0);
        EXPECT(full.check(), "4096 states, 16384 edges");
        std::vector<int> block((size_t)GRAMMAR_TABLE_INTS, 0);
        grammar_table_pack(block.data(), full.eot, full.n, full.off.data(), full.tok.data(), full.next.data(), full.accept.data());
        EXPECT(block[GRAMMAR_NEXT_AT + GRAMMAR_MAX_EDGES - 1] == (GRAMMAR_MAX_EDGES - 1) % GRAMMAR_MAX_STATES, "the last edge");
    }
    // ---- every violation
    { Table g = abc(); g.n = 0; g.off = {0}; g.accept = {}; refused(g, "states outside", "no state"); }
    { Table g = abc(); g.n = GRAMMAR_MAX_STATES + 1; g.off.assign((size_t)g.n + 1, 0); g.accept.assign((size_t)g.n, 0); g.tok.clear(); g.next.clear();
      refused(g, "states outside", "too many states"); }
    { Table g = abc(); g.off[0] = 1; refused(g, "edge_off[0]", "offsets start past 0"); }
    { Table g = abc(); g.off[2] = 1; refused(g, "offsets ascend", "offsets descend"); }
    { Table g = abc(); g.off[4] = GRAMMAR_MAX_EDGES + 1; refused(g, "at most", "too many edges"); }      // (refused before any edge is read)
    { Table g = abc(); g.off[1] = -1; refused(g, "offsets ascend", "a negative offset"); }
    { Table g = abc(); g.tok[1] = 1; refused(g, "do not ascend", "equal tokens in a state"); }
    { Table g = abc(); g.tok[0] = 2; g.tok[1] = 1; refused(g, "do not ascend", "descending tokens"); }
    { Table g = abc(); g.tok[4] = 90; refused(g, "no text token", "end-of-text as an edge token"); }
    { Table g = abc(); g.tok[4] = 95; refused(g, "no text token", "a special as an edge token"); }
    { Table g = abc(); g.tok[4] = 100; refused(g, "no text token", "a token outside the vocabulary"); }
    { Table g = abc(); g.tok[0] = -1; refused(g, "no text token", "a negative token"); }
    { Table g = abc(); g.next[3] = 4; refused(g, "leads to state", "a next state past the last"); }
    { Table g = abc(); g.next[3] = -1; refused(g, "leads to state", "a negative next state"); }
    { Table g = abc(); g.accept[2] = 2; refused(g, "not 0 or 1", "accept 2"); }
    { Table g = abc(); g.accept[0] = -1; refused(g, "not 0 or 1", "accept -1"); }
    { Table g = abc(); g.eot = 100; refused(g, "eot", "end-of-text outside the vocabulary"); }
    { Table g = abc(); g.eot = 0; refused(g, "eot", "end-of-text 0"); }
    {   // null arrays
        Table g = abc();
        char msg[64];
        EXPECT(!grammar_table_check(g.V, g.eot, g.n, nullptr, g.tok.data(), g.next.data(), g.accept.data(), msg, sizeof(msg)), "null offsets");
        EXPECT(!grammar_table_check(g.V, g.eot, g.n, g.off.data(), nullptr, g.next.data(), g.accept.data(), msg, sizeof(msg)), "null tokens");
        EXPECT(!grammar_table_check(g.V, g.eot, g.n, g.off.data(), g.tok.data(), nullptr, g.accept.data(), msg, sizeof(msg)), "null nexts");
        EXPECT(!grammar_table_check(g.V, g.eot, g.n, g.off.data(), g.tok.data(), g.next.data(), nullptr, msg, sizeof(msg)), "null accept");
        EXPECT(!grammar_table_check(g.V, g.eot, g.n, g.off.data(), g.tok.data(), g.next.data(), nullptr, nullptr, 0), "no message buffer");
        EXPECT(strlen(msg) < sizeof(msg), "the message fits its buffer");
    }
    {   // random tables: a valid one passes; one word changed to a value out of range is refused
        std::mt19937 rng(20250);
        for (int trial = 0; trial < 200; ++trial) {
            Table g;
            g.V = 3000; g.eot = 2500;
            g.n = 1 + (int)(rng() % 40);
            g.off = {0};
            for (int n = 0; n < g.n; ++n) {
                const int k = (int)(rng() % 9);
                int t = (int)(rng() % 50);
                for (int i = 0; i < k; ++i) { g.tok.push_back(t); g.next.push_back((int32_t)(rng() % (unsigned)g.n)); t += 1 + (int)(rng() % 200); }
                g.off.push_back((int32_t)g.tok.size());
                g.accept.push_back((int32_t)(rng() % 2));
            }
            EXPECT(g.check(), "a random valid table");
            if (g.tok.empty()) continue;
            Table b = g;
            const size_t i = rng() % b.tok.size();
            switch (trial % 3) {
                case 0: b.tok[i] = b.eot + (int)(rng() % 600); break;
                case 1: b.next[i] = b.n + (int)(rng() % 5); break;
                default: b.accept[rng() % b.accept.size()] = 2 + (int)(rng() % 5); break;
            }
            EXPECT(!b.check(), "a random table with one bad word");
        }
    }
    printf("grammar_table_check: %d failures\n", fails);
    return fails ? 1 : 0;
}
