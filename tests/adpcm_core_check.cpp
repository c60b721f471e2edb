// Stand-alone check of csrc/adpcm_core.h as ordinary host C++ (tests/test_adpcm_core_host.py builds it with -fsanitize=address,undefined).
// Input file: int32 count, then records { int32 kind, ch, block_align, want, n_coef, must; int16 coefs[2 * n_coef]; uint8 block[block_align];
// int16 expect[want * ch] }. must 1: the decode has to equal `expect` (an intact block, or a corrupted one the oracle decodes); must 2:
// run for the sanitizers alone (the oracle refuses the block's header: the core clamps the index, no right answer exists).
// Every buffer is a heap allocation of exactly the size the core is told, so one byte read or written past it stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../whisperlive_amd/csrc/adpcm_core.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    long wrong = 0, short_n = 0;
    for (int r = 0; r < count; ++r) {
        int32_t h[6];
        if (std::fread(h, 4, 6, f) != 6) return 2;
        const int kind = h[0], ch = h[1], ba = h[2], want = h[3], n_coef = h[4], must = h[5];
        int16_t* coefs = static_cast<int16_t*>(std::malloc(n_coef ? 4 * (size_t)n_coef : 1));
        uint8_t* blk = static_cast<uint8_t*>(std::malloc(ba ? (size_t)ba : 1));
        const size_t ns = (size_t)want * ch;
        int16_t* expect = static_cast<int16_t*>(std::malloc(ns ? 2 * ns : 1));
        int16_t* out = static_cast<int16_t*>(std::calloc(ns ? ns : 1, 2));
        if ((n_coef && std::fread(coefs, 4, n_coef, f) != (size_t)n_coef) || (ba && std::fread(blk, 1, ba, f) != (size_t)ba) ||
            (ns && std::fread(expect, 2, ns, f) != ns)) return 2;
        for (int c = 0; c < ch; ++c) {
            const int n = kind == ADPCM_IMA ? adpcm_ima_block(blk, ba, ch, c, want, out + c, ch)
                                            : adpcm_ms_block(blk, ba, ch, c, want, coefs, n_coef, out + c, ch);
            if (n != want) ++short_n;
        }
        if (must == 1 && std::memcmp(out, expect, 2 * ns)) {
            if (wrong < 5) std::printf("record %d (kind %d, ch %d, block_align %d) decodes wrong\n", r, kind, ch, ba);
            ++wrong;
        }
        std::free(coefs); std::free(blk); std::free(expect); std::free(out);
    }
    std::fclose(f);
    std::printf("records %d wrong %ld short %ld \n", count, wrong, short_n);
    return wrong || short_n ? 1 : 0;
}
