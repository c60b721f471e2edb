// Which dec_gemv2_kernel instantiation the launcher picks per projection (host only, no GPU): the rules of dec_gemv.hip gemv2_cfg made visible.
//   hipcc -std=c++17 -O1 scripts/gemv_pick_probe.cpp -o /tmp/gemv_pick_probe -Lwhisperlive_amd -l:libwlx.so -Wl,-rpath,$PWD/whisperlive_amd
//   /tmp/gemv_pick_probe                  (WLX_DECODE_V1=1 in front: the answers with the first-generation kernels selected)
// --heads: per listed projection the argument head the launcher fills (dec_gemv_internal.h GemvHead), checked field by field against the struct as launched
//   (host only: also runs under host AddressSanitizer as this stand-alone program); exit status 1 on a mismatch.
// --sweep: the whole decision space instead of the listed projections (tests/test_gemv_picks.py compares it with tests/golden/gemv_pick_sweep.txt.gz).
// First line "M <every row count>", then one line per (in, out, xsrc, K, N, bias, busy_device, slab, KTS) series:
//   in out xsrc K N b<bias?> u<busy> s<slab?> k<KTS>|<M first>-<M last>:<slab_split>,<lean>,<kernel name>|...      (run-length over M)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../whisperlive_amd/csrc/common.h"
#include "../whisperlive_amd/csrc/decoder.h"
#include "../whisperlive_amd/csrc/dec_gemv_internal.h"
using namespace wlx;
static float bias = 0.f;
static int sweep() {
    static float slab = 0.f;
    int Ms[63], nM = 0;
    for (int m = 1; m <= 50; ++m) Ms[nM++] = m;
    for (int m : {60, 64, 65, 80, 96, 112, 120, 128, 160, 224, 240, 320, 321}) Ms[nM++] = m;
    printf("M");
    for (int i = 0; i < nM; ++i) printf(" %d", Ms[i]);
    printf("\n");
    for (int in = 0; in < 3; ++in) for (int out = 0; out < 6; ++out) for (int xsrc = 0; xsrc < 3; ++xsrc)
    for (int d : {384, 512, 768, 1024, 1280, 96, 128, 640, 1536}) {
        const struct { int K, N; bool vocab; } shapes[] = {{d, d, false}, {d, 3 * d, false}, {d, 4 * d, false}, {4 * d, d, false},
                                                             {d, 51864, true}, {d, 51865, true}, {d, 51866, true}};
        for (auto& sh : shapes) for (int wb = 0; wb < 2; ++wb) for (int busy = 0; busy < 2; ++busy) for (int ws = 0; ws < 2; ++ws)
        for (int wk = 0; wk < (out == GEMV_OUT_SLAB ? 2 : 1); ++wk) {
            const int KTS = wk ? sh.K / 32 / WLX_FC2_KS : 0;
            printf("%d %d %d %d %d b%d u%d s%d k%d", in, out, xsrc, sh.K, sh.N, wb, busy, ws, KTS);
            char prev[160] = "", cur[160];
            int first = 0;
            for (int i = 0; i <= nM; ++i) {
                if (i < nM) {
                    GemvParams p; memset(&p, 0, sizeof p);
                    p.in_mode = in; p.out_mode = out; p.M = Ms[i]; p.K = sh.K; p.KT = sh.K / 32; p.N = sh.N; p.xsrc = xsrc;
                    p.bias = wb ? &bias : nullptr; p.busy_device = busy; p.slab = ws ? &slab : nullptr; p.KTS = KTS;
                    p.H = sh.K / 64; p.R = 5;
                    snprintf(cur, sizeof cur, "%d,%d,%s", dec_gemv_slab_split(Ms[i], sh.K, sh.N), (int)dec_gemv_is_lean(p), dec_gemv_kernel_name(p));
                }
                if (i == nM || (i > 0 && strcmp(cur, prev))) { printf("|%d-%d:%s", Ms[first], Ms[i - 1], prev); first = i; }
                strcpy(prev, cur);
            }
            printf("\n");
        }
    }
    return 0;
}
int main(int argc, char** argv) {
    if (const char* v1 = getenv("WLX_DECODE_V1")) g_decode_v1 = v1[0] == '1';   // (the engine sets it when it is created)
    if (argc > 1 && !strcmp(argv[1], "--sweep")) return sweep();
    struct { const char* what; int in, out, M, K, N, xsrc, KS; } cases[] = {
        {"small o-proj M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 768, 768, GEMV_X_PLAIN, 0},
        {"small fc2 slab M5", GEMV_IN_F16, GEMV_OUT_SLAB, 5, 3072, 768, GEMV_X_PLAIN, WLX_FC2_KS},
        {"small o-proj slabs M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 768, 768, GEMV_X_SLABS, 0},
        {"small o-proj M60", GEMV_IN_F16, GEMV_OUT_RESID, 60, 768, 768, GEMV_X_PLAIN, 0},
        {"small fc2 slab M60", GEMV_IN_F16, GEMV_OUT_SLAB, 60, 3072, 768, GEMV_X_PLAIN, WLX_FC2_KS},
        {"small fc2 resid M60", GEMV_IN_F16, GEMV_OUT_RESID, 60, 3072, 768, GEMV_X_PLAIN, 0},
        {"small xattn M5", GEMV_IN_XATTN, GEMV_OUT_RESID, 5, 768, 768, GEMV_X_PLAIN, 0},
        {"large o-proj M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 1280, 1280, GEMV_X_PLAIN, 0},
        {"large fc2 slab M5", GEMV_IN_F16, GEMV_OUT_SLAB, 5, 5120, 1280, GEMV_X_PLAIN, WLX_FC2_KS},
        {"large fc2 resid M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 5120, 1280, GEMV_X_PLAIN, 0},
        {"large o-proj slabs M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 1280, 1280, GEMV_X_SLABS, 0},
        {"large xattn M5", GEMV_IN_XATTN, GEMV_OUT_RESID, 5, 1280, 1280, GEMV_X_PLAIN, 0},
        {"medium o-proj M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 1024, 1024, GEMV_X_PLAIN, 0},
        {"medium fc2 slab M5", GEMV_IN_F16, GEMV_OUT_SLAB, 5, 4096, 1024, GEMV_X_PLAIN, WLX_FC2_KS},
        {"medium fc2 resid M16", GEMV_IN_F16, GEMV_OUT_RESID, 16, 4096, 1024, GEMV_X_PLAIN, 0},
        {"base o-proj M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 512, 512, GEMV_X_PLAIN, 0},
        {"small mlp-up M5", GEMV_IN_LN, GEMV_OUT_GELU_F16, 5, 768, 3072, GEMV_X_PLAIN, 0},
        {"small mlp-up M16", GEMV_IN_LN, GEMV_OUT_GELU_F16, 16, 768, 3072, GEMV_X_PLAIN, 0},
        {"small mlp-up M60", GEMV_IN_LN, GEMV_OUT_GELU_F16, 60, 768, 3072, GEMV_X_PLAIN, 0},
        {"small q-proj M5", GEMV_IN_LN, GEMV_OUT_F16, 5, 768, 768, GEMV_X_PLAIN, 0},
        {"large mlp-up M5", GEMV_IN_LN, GEMV_OUT_GELU_F16, 5, 1280, 5120, GEMV_X_PLAIN, 0},
        {"large q-proj M5", GEMV_IN_LN, GEMV_OUT_F16, 5, 1280, 1280, GEMV_X_PLAIN, 0},
        {"large mlp-up M16", GEMV_IN_LN, GEMV_OUT_GELU_F16, 16, 1280, 5120, GEMV_X_PLAIN, 0},
        {"medium mlp-up M5", GEMV_IN_LN, GEMV_OUT_GELU_F16, 5, 1024, 4096, GEMV_X_PLAIN, 0},
        {"medium q-proj M5", GEMV_IN_LN, GEMV_OUT_F16, 5, 1024, 1024, GEMV_X_PLAIN, 0},
        {"small qkv slabs M5", GEMV_IN_LN, GEMV_OUT_QKV, 5, 768, 2304, GEMV_X_SLABS, 0},
        {"small qkv embed M5", GEMV_IN_LN, GEMV_OUT_QKV, 5, 768, 2304, GEMV_X_EMBED, 0},
        {"medium qkv slabs M5", GEMV_IN_LN, GEMV_OUT_QKV, 5, 1024, 3072, GEMV_X_SLABS, 0},
        {"large qkv slabs M5", GEMV_IN_LN, GEMV_OUT_QKV, 5, 1280, 3840, GEMV_X_SLABS, 0},
        {"large qkv slabs M16", GEMV_IN_LN, GEMV_OUT_QKV, 16, 1280, 3840, GEMV_X_SLABS, 0},
        {"tiny o-proj M5", GEMV_IN_F16, GEMV_OUT_RESID, 5, 384, 384, GEMV_X_PLAIN, 0},
    };
    const bool heads = argc > 1 && !strcmp(argv[1], "--heads");
    int bad = 0;
    // --heads: distinct addresses and strides per field, so that a head slot filled from the wrong field shows
    static float xrows[4], gam[4], bet[4], slabs[4], pml[4];
    static half_t wts[8], xh[8], po[8];
    for (auto& c : cases) {
        GemvParams p; memset(&p, 0, sizeof p);
        p.in_mode = c.in; p.out_mode = c.out; p.M = c.M; p.K = c.K; p.KT = c.K / 32; p.N = c.N; p.xsrc = c.xsrc; p.bias = &bias;
        p.H = c.K / 64; p.R = 5;
        if (c.KS) p.KTS = p.KT / c.KS;
        if (heads) {
            p.X = xrows; p.ldx = c.K + 1; p.Xh = xh; p.ldxh = c.K + 2; p.gamma = gam; p.beta = bet; p.Wp = wts; p.slab = slabs; p.slab_stride = 7L * c.N + 3;
            p.part_o = po; p.part_ml = pml;
            GemvHead h; GemvParams q;
            if (!dec_gemv_head(p, &h, &q)) { printf("%-24s no head (%s)\n", c.what, dec_gemv_kernel_name(p)); continue; }
            const void* rows = q.in_mode == GEMV_IN_LN ? (q.xsrc == GEMV_X_EMBED ? nullptr : (const void*)q.X) : q.in_mode == GEMV_IN_F16 ? (const void*)q.Xh : (const void*)q.part_o;
            const void* aux = q.in_mode == GEMV_IN_XATTN ? (const void*)q.part_ml : (q.in_mode == GEMV_IN_LN && q.xsrc == GEMV_X_SLABS) ? (const void*)q.slab : nullptr;
            const long ld = q.in_mode == GEMV_IN_LN ? (q.xsrc == GEMV_X_EMBED ? 0 : q.ldx) : q.in_mode == GEMV_IN_F16 ? q.ldxh : 0;
            const long auxi = q.in_mode == GEMV_IN_XATTN ? (q.R | (q.H << 16)) : (q.in_mode == GEMV_IN_LN && q.xsrc == GEMV_X_SLABS) ? q.slab_stride : 0;
            const bool ok = h.rows == rows && h.aux == aux && h.gamma == q.gamma && h.beta == q.beta && h.wp == q.Wp && h.ld == ld && h.aux_i == auxi &&
                            (h.dims & 0xff) == q.M && ((h.dims >> 8) & 0xff) == q.nwm && ((h.dims >> 16) & 0xff) == q.KTW && ((h.dims >> 24) & 1) == q.xstage &&
                            (h.kt & 0xff) == q.KT && ((h.kt >> 8) & 0xff) == q.KTS && (int)((unsigned)h.kt >> 16) == q.Mtot && q.K == q.KT * 32;
            bad += !ok;
            printf("%-24s %s  rows=%s ld=%d aux=%s aux_i=%d M=%d nwm=%d KTW=%d xstage=%d KT=%d KTS=%d Mtot=%d  %s\n", c.what, ok ? "head==struct" : "MISMATCH",
                   h.rows == xrows ? "X" : h.rows == xh ? "Xh" : h.rows == po ? "part_o" : h.rows ? "?" : "-", h.ld, h.aux == slabs ? "slab" : h.aux == pml ? "part_ml" : h.aux ? "?" : "-",
                   h.aux_i, h.dims & 0xff, (h.dims >> 8) & 0xff, (h.dims >> 16) & 0xff, (h.dims >> 24) & 1, h.kt & 0xff, (h.kt >> 8) & 0xff, (int)((unsigned)h.kt >> 16), dec_gemv_kernel_name(p));
            continue;
        }
        printf("%-24s slab_split=%d lean=%d  %s\n", c.what, dec_gemv_slab_split(c.M, c.K, c.N), (int)dec_gemv_is_lean(p), dec_gemv_kernel_name(p));
    }
    return bad ? 1 : 0;
}
