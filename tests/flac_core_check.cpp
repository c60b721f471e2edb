// Stand-alone check of csrc/flac_core.h on the host (tests/test_flac_core_host.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it as a child process): decodes the frames of a record file and compares them with the
// integers written beside them.
// Record file, little endian: int32 count, then per record
//     int32 stream_bps, channels, blocksize, n_bytes, must_decode;  n_bytes of frame;  int32 expected[blocksize][channels]
// must_decode = 1: the frame is intact: status FLAC_OK and equal samples. 0: a corruption: a non-ok status, or equal samples.
// 3: a corruption the oracle decoder rejects: a non-ok status. 2: any outcome (run for the sanitizers alone).
// Every frame is decoded out of a heap copy of exactly its own bytes into a heap buffer of exactly blocksize * channels values, so
// AddressSanitizer sees any read past `end` and any write past the block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../whisperlive_amd/csrc/flac_core.h"

static bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: flac_core_check <records>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t count = 0;
    if (!get(f, &count, 4)) return 2;
    long intact_bad = 0, wrong_ok = 0, rejected = 0, same = 0, unjudged = 0;
    int by_status[8] = {0};
    for (int32_t r = 0; r < count; ++r) {
        int32_t h[5];
        if (!get(f, h, sizeof h)) return 2;
        const int bps = h[0], ch = h[1], n = h[2], nb = h[3], must = h[4];
        uint8_t* bytes = (uint8_t*)malloc((size_t)nb);
        std::vector<int32_t> want((size_t)n * ch);
        if (!get(f, bytes, (size_t)nb) || !get(f, want.data(), want.size() * 4)) return 2;
        int32_t* planes = (int32_t*)malloc((size_t)n * ch * sizeof(int32_t));
        memset(planes, 0x5A, (size_t)n * ch * sizeof(int32_t));
        int assign = -1;
        const int rc = flac_decode_frame(bytes, 0, nb, bps, ch, n, planes, n, &assign);
        if (rc >= 0 && rc < 8) by_status[rc]++;
        bool equal = rc == FLAC_OK;
        for (int i = 0; equal && i < n; ++i) {
            if (assign != FLAC_CH_INDEPENDENT) {
                int32_t l, rr;
                flac_stereo(assign, planes[i], planes[n + i], &l, &rr);
                equal = l == want[(size_t)i * ch] && rr == want[(size_t)i * ch + 1];
            } else {
                for (int c = 0; equal && c < ch; ++c) equal = planes[(size_t)c * n + i] == want[(size_t)i * ch + c];
            }
        }
        if (must == 1) {
            if (!equal) { ++intact_bad; fprintf(stderr, "record %d: intact frame: status %d, samples %s\n", r, rc, equal ? "equal" : "differ"); }
        } else if (must == 2) ++unjudged;
        else if (rc != FLAC_OK) ++rejected;
        else if (must == 3) { ++wrong_ok; fprintf(stderr, "record %d: status ok for a frame the oracle rejects\n", r); }
        else if (equal) ++same;
        else { ++wrong_ok; fprintf(stderr, "record %d: corrupted frame decoded with status ok to other samples\n", r); }
        free(planes);
        free(bytes);
    }
    fclose(f);
    printf("records %d intact_bad %ld corrupt_rejected %ld corrupt_same %ld corrupt_wrong_ok %ld unjudged %ld status", count, intact_bad, rejected, same, wrong_ok, unjudged);
    for (int i = 0; i < 6; ++i) printf(" %d:%d", i, by_status[i]);
    printf("\n");
    return intact_bad || wrong_ok ? 1 : 0;
}
