// engine.h — host-side state of libwlx: weights in kernel layout, per-slot device buffers, the device PCM rings, and PcmLease, the
// one way an engine on another stream reads audio that is resident in a slot or a ring.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>
#include "../../include/wlx.h"
#include "align.h"
#include "decoder.h"
#include "host.h"

namespace wlx {

// the launch of a slot's decode step between the vocabulary projection and the search: none, keyword boosting with one table or a table per
// item, or a grammar (wlx_grammar_set: masks where the others add). One mode at a time: the last set call decides.
enum BiasMode : int { BIAS_NONE = 0, BIAS_ONE = 1, BIAS_ITEMS = 2, BIAS_GRAMMAR = 3 };

// what a captured decode-step graph depends on (engine_decode.hip get_step_graph)
struct StepGraphKey {
    int rows, R, groups, nsteps;
    bool busy, sampling;
    int bias;                   // BiasMode of the slot: the step launches dec_bias_kernel (one table: wlx_bias_set) or dec_bias_items_kernel (per item:
                                // wlx_bias_set_items) or dec_grammar_kernel (wlx_grammar_set) in front of the search, or nothing; a graph captured for
                                // one mode is never replayed for another
    bool operator<(const StepGraphKey& o) const {
        return std::tie(rows, R, groups, nsteps, busy, sampling, bias) < std::tie(o.rows, o.R, o.groups, o.nsteps, o.busy, o.sampling, o.bias);
    }
};

// the decoder pass's working set (scratch rows + row tables); a slot holds two (Slot::step, Slot::pf; engine.hip alloc_decbufs)
struct DecBufs {
    float* xd; half_t *qd, *attnd, *hd;
    float* slab; int slab_rows;                      // [WLX_FC2_KS][slab_rows][d] partial sums of the K-split MLP output projection (dec_gemv.hip GEMV_OUT_SLAB)
    half_t* part_o; float* part_ml;
    int *d_token, *d_pos, *d_cache, *d_ancrow, *d_group_item;
    bool prefill;                                    // the prompt-prefill set: decoder_pass picks its launch forms by it
};

// decode-step profiler (wlx_debug_profile_step): pass 1 only lists the launches of a step (name, algorithmic bytes);
// pass 2 replays, per kernel name, a captured graph holding just that kernel's launches of the step
struct ProfRec { std::string name; double bytes; };
struct Prof { std::vector<ProfRec> recs; bool list_only = true; std::string only; int t = 0; };

struct Slot {
    std::mutex call_mu;      // held by the entry point currently using the slot (engine.hip slot_acquire)
    int B = 0, R = 0, rows_cap = 0, cache_rows = 0, groups_cap = 0;
    hipStream_t stream = nullptr;
    bool dedicated_queue = false;       // the stream owns a hardware queue (engine.hip create_slot_stream); counted per device
    int device_of = -1;
    bool counted = false;               // in the per-device live-slot count
    unsigned promote_epoch = 0;         // the last "crowd left" event this slot tried to take a hardware queue at (engine.hip slot_acquire)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_lm0 = nullptr, ev_lm1 = nullptr;   // the last log-mel launch (its time is read lazily: wlx_logmel_resident does not wait)
    hipEvent_t ev_en0 = nullptr, ev_en1 = nullptr;   // the last encoder pass (wlx_encode does not wait either)
    bool en_pending = false;
    bool lm_pending = false;
    bool gen_pending = false;                  // the last generate's device time / step count: read in wlx_timings_get, not in wlx_generate
    std::vector<int> lm_items;          // items whose log-mel was requested and not launched yet (engine.hip flush_logmel)
    bool busy_variant = false;          // the decode launches of this slot use the work-saving shapes (three or more live slots on the device; engine_decode.hip device_is_busy)
    std::vector<void*> allocs, host_allocs;   // device / pinned buffers of the slot's whole life (slot_free)
    // features
    float* pcm = nullptr; size_t pcm_cap = 0;       // [B][pcm_cap]
    float* feats = nullptr; long feat_ld = 0;        // [B][n_mels][feat_ld]
    std::vector<int> nframes;
    std::vector<int64_t> npcm;                       // samples resident per item
    unsigned* gmax = nullptr;
    ResampleStage rs{};                              // staging of wlx_pcm_put_frames, allocated at its first call (engine.hip)
    bool rs_ready = false;
    // wlx_pcm_put_flac (flac.hip): ONE device scratch for file bytes | frame table | status words | int32 planes | float32 frames, grown
    // on demand and owned by name; a call keeps at most 2 * RS_BLOCK_BYTES of it afterwards. ev: upload / frames / finish / resample marks
    // wlx_pcm_put_wav (adpcm.hip) lays its data chunk | float32 frames into the same buf / cap, under the same rule.
    struct FlacScratch { unsigned char* buf = nullptr; size_t cap = 0; hipEvent_t ev[5] = {}; float index_ms = 0.f; bool timed = false; } flac;
    int* h_put_status = nullptr; size_t h_put_status_cap = 0;   // wlx_pcm_put_many (put_many.hip): pinned copy of a call's FLAC status words, in ints
    long long* d_rng = nullptr;                      // [2 * WLX_LM_MAXRANGES] range table of the last wlx_logmel_ring
    // wlx_logmel_chunks: [B] chunk descriptors and [B][WLX_LM_MAXRANGES][2] range pairs, pinned staging and device copy (allocated at
    // its first call); `ck_staged` is recorded behind the copy: the next call waits for it before it rewrites the pinned side
    LogmelChunk *h_chunks = nullptr, *d_chunks = nullptr;
    long long *h_crng = nullptr, *d_crng = nullptr;
    hipEvent_t ck_staged = nullptr; bool ck_pending = false;
    hipEvent_t ev_pcm = nullptr;                     // recorded on `stream` for a reader on another stream (engine.hip PcmLease::order)
    // encoder
    half_t *featT = nullptr, *h1 = nullptr, *ln = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr,
           *attn = nullptr, *h2 = nullptr, *enc16 = nullptr;
    float *x = nullptr, *enc32 = nullptr;
    long featT_stride = 0, h1_stride = 0;
    half_t *ck = nullptr, *cvt = nullptr;            // cross K [L][B][TPAD][d], V^T [L][B][d][TPAD]
    int enc_batch = 0;
    // decoder
    half_t *kc = nullptr, *vc = nullptr;             // self cache [L][cache_rows][448][d]
    float* logits = nullptr;
    long ldl = 0;
    // the decoder pass's working sets: `step` = the decode steps and chunked passes (rows_cap rows), `pf` = the one-pass and the joint
    // prompt prefill (up to WLX_T_TEXT rows: engine_decode.hip prefill_tokens, gen_prefill)
    DecBufs step{}, pf{};
    bool pf_ok = false;                 // every projection of this model runs on the lean kernel in row chunks (decided at creation)
    short* d_anc = nullptr; int* d_intok = nullptr;
    bool anc_ident = false;                          // the uploaded row tables have ancrow[r] == r (decode steps; upload_rows)
    SearchState st{};
    SearchParams* d_sp = nullptr;
    // keyword boosting (wlx_bias_set / wlx_bias_clear; dec_bias.hip): the table's device block and the per-(cache row, position) states, allocated
    // at the first wlx_bias_set and kept at those addresses for the slot's life; `h_bias` is the block's pinned staging (rewritten only behind a
    // wait for the stream); `bias_mode`: what the decode steps launch in front of the search (engine_decode.hip launch_bias)
    BiasTable bias{}; int* d_bias = nullptr; int* h_bias = nullptr; int bias_mode = BIAS_NONE;
    short* bias_state = nullptr;                     // [max(cache_rows, rows_cap)][448], shared by the two modes (allocated by whichever comes first)
    // per-item tables (wlx_bias_set_items / wlx_bias_select): the pool, its pinned staging, the selection and its pinned staging, allocated at the
    // first wlx_bias_set_items and kept at those addresses. `sel_n`: items the selection covers; `ev_sel` is recorded behind the selection's copy,
    // the next select waits for it before it rewrites the pinned side (the pool's staging waits for the stream, like h_bias)
    BiasItems bias_items{}; int* d_pool = nullptr; int* h_pool = nullptr; int* d_sel = nullptr; int* h_sel = nullptr;
    int bias_tables = 0, sel_n = 0; hipEvent_t ev_sel = nullptr; bool sel_pending = false;
    // grammar (wlx_grammar_set / wlx_grammar_clear; dec_grammar.hip): the table's device block and its pinned staging, allocated at the first
    // wlx_grammar_set and kept at those addresses; the states are `bias_state`. `grammar_eot`: the end-of-text id the table was checked against
    GrammarTable grammar{}; int* d_grammar = nullptr; int* h_grammar = nullptr; int grammar_eot = -1;
    unsigned* d_suppress = nullptr;
    int* d_lang_ids = nullptr; float* d_probs = nullptr; float* d_tokprob = nullptr;
    // pinned host staging
    int* h_stage = nullptr; size_t h_stage_ints = 0;
    // pinned staging of wlx_generate: set-up tables in (one async copy each, no synchronisation); the results come back through h_hyp
    unsigned char* h_gen = nullptr; size_t h_gen_bytes = 0;      // laid out by gen_staging
    int* h_pf = nullptr; bool h_pf_used = false;   // pinned staging of the one-pass prompt prefill's row tables (its own: no wait for the stream before the first prefill of a call; engine_decode.hip prefill_tokens)
    int* h_hyp = nullptr;                      // pinned result area the update kernels write: [n_hyp B | hyp_len B*H | hyp_score B*H | no_speech B | hyp_tokens B*H*448]
    int max_items = 0;                         // B of that layout
    std::vector<int> last_suppress; bool suppress_valid = false;   // the suppress mask on the device was built from this list
    std::map<StepGraphKey, hipGraphExec_t> graphs;
    wlx_timings tm{};
    Prof* prof = nullptr;
    // word alignment (wlx_align): while `align` is set, decoder_pass also writes the raw cross-attention scores of the
    // alignment heads for the rows of the current chunk
    struct AlignCapture { float* scores; const int32_t* heads; int n_heads, n_tok, row0, item; }* align = nullptr;
    float* align_scores = nullptr; size_t align_cap = 0;     // [n_heads][n_tok][1536] fp32, grown on demand (so owned by name, not by `allocs`)
    int* d_align_tgt = nullptr; float* d_align_prob = nullptr;   // [448]
    // wlx_align_batch (allocated at its first call): pinned staging laid out by align_staging (entry table, per-chunk row tables and targets in;
    // paths, counts and probabilities out), the device entry table, and ONE device scratch for stats | cost matrices | DTW traces, grown on demand
    unsigned char* h_align = nullptr;
    AlignEnt* d_align_ent = nullptr;
    float* align_post = nullptr; size_t align_post_cap = 0;   // in floats (owned by name, like align_scores)
    hipEvent_t ev_al0 = nullptr, ev_al1 = nullptr, ev_al2 = nullptr;
    float align_pass_ms = 0.f, align_post_ms = 0.f;
};

// Device-resident PCM of one client stream (include/wlx.h: wlx_ring_*, wlx_ring_group_*; ring.hip). A Ring is what a READER needs:
// samples [base, base + resident) of the stream live contiguously at buf[0 .. resident) (a trim moves the survivors to the front, once
// per 30 s of audio: <= 1 MB device to device), so every reader sees plain contiguous memory. Readers are kernels of the VAD object's,
// the speaker engine's and a slot's stream, each behind a PcmLease (below); `mu` serialises them against the writer, `last_read` (recorded
// on the reader's stream behind its launch) is what a trim or a growth waits for before it moves data under a reader that was launched
// but has not run yet. Those three fields are ring.hip's alone.
struct RingStore;
struct Ring {
    std::mutex mu;
    int device = 0;
    float* buf = nullptr;                                   // this lane's row of the store's allocation
    int64_t base = 0, resident = 0;
    hipEvent_t last_read = nullptr; bool read_pending = false; hipStream_t last_read_stream = nullptr;
    RingStore* store = nullptr;
};

// The WRITE side of every ring: `lanes` rings in ONE allocation [lanes][cap], filled by one append (the socket thread). A mono ring
// (wlx_ring_create) is a store with one lane that down-mixes: the caller's handle is that lane (`lone`), packets are 16 kHz floats or,
// after wlx_ring_set_format, wire frames. A ring group (wlx_ring_group_create) is a store with one lane per channel in `split` mode, one
// launch of the split stream form of resample.hip per packet; its lanes are borrowed by readers and refuse the writer entry points.
// base and resident are equal on all lanes at all times, and base + resident == fmt.M with a format. Lock order: the store's `mu`, then
// the lanes' `mu` in lane order; a reader only ever holds ONE lane's mutex, so the order cannot cycle.
struct RingStore {
    std::mutex mu;
    int device = 0;
    float* buf = nullptr; size_t cap = 0;                   // [lanes][cap]
    hipStream_t stream = nullptr;
    std::vector<wlx_ring*> lanes;
    bool lone = false, split = false;
    bool has_format = false, appended = false;              // `appended`: some append call has succeeded (no format after that)
    ResampleStream fmt{};                                   // J, M, the tail of whole interleaved frames: shared by all lanes
};

struct Engine {
    wlx_spec spec{};
    int device = 0;
    int H = 0;
    std::vector<void*> allocs;
    LogmelConsts lm{};
    half_t *conv1_w = nullptr, *conv2_w = nullptr;
    float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *enc_ln_g = nullptr, *enc_ln_b = nullptr;
    int conv1_KT = 0;
    std::vector<LayerW> enc;
    half_t* Wckv = nullptr; float* bckv = nullptr;
    half_t *tok_emb16 = nullptr, *Wvocab = nullptr;
    float *dec_pos = nullptr, *dec_ln_g = nullptr, *dec_ln_b = nullptr;
    std::vector<LayerW> dec;
    std::mutex mu;
    std::vector<Slot*> slots;
    bool use_graph = true;
};

}  // namespace wlx

struct wlx_engine : public wlx::Engine {};
struct wlx_ring : public wlx::Ring {};
struct wlx_ring_group : public wlx::RingStore {};   // (also the store behind a mono wlx_ring)

// ------------------------------------------------------------------------------------------------
// shared between engine.hip (slots, streams), engine_decode.hip (decode) and engine_debug.hip (hooks)
namespace wlx {

// Every entry point holds the slot's call mutex for its duration: a slot is one unit of concurrency (one stream, one set
// of scratch buffers), so a second call on it is refused rather than corrupting the first, and wlx_slot_destroy waits for
// a call in flight instead of freeing buffers under it.
struct SlotGuard {
    Slot* s = nullptr;
    ~SlotGuard() { if (s) s->call_mu.unlock(); }
};
int slot_acquire(wlx_engine* e, int slot, SlotGuard& g);                                  // engine.hip
int create_slot_stream(int device, hipStream_t* out, bool* dedicated_out);
int flush_logmel(Engine* e, Slot* s);                      // engine.hip: the recorded log-mel requests go out
int slot_grow_audio(Engine* e, Slot* s, size_t n_samples); // engine.hip: PCM + feature buffers for n_samples per item
int slot_resample_stage(Slot* s);                          // engine.hip: Slot::rs, allocated at the first call

// The READER's side of resident audio: 16 kHz mono float32 in device memory that belongs to a slot item (wlx_pcm_put*) or to a ring
// lane, held still for one reader whose kernels run on a stream of its own. The one invariant: nothing moves, frees or rewrites the
// samples while a reader launched on another stream may still read them. Who holds what, in which order:
//   slot item   the slot's call mutex (open_slot, for the lease's life), THEN the reader's own mutex. order() puts the reader's stream
//               behind whatever wrote the PCM on the slot's stream; the reader waits for its pass before it returns.
//   ring lane   the reader's own mutex, THEN the lane's `mu` (open_ring, for the lease's life); wlx_logmel_ring, whose reader is a slot,
//               holds that slot's call mutex first. A synchronous reader (it waits for its pass under the lease) owes the ring nothing
//               more: samples are final when their append returns. An asynchronous reader (it returns behind its launch) brackets the
//               launch with before_launch / launched: the lane remembers the launch, and a trim or a growth waits for it (ring.hip).
// The lease never takes the reader's mutex and decides no policy: the entry point refuses its own arguments between same_device and
// open_*, and takes its mutex where the order above says. view: samples [base, base + resident) lie at buf[0 .. resident).
struct PcmLease {
    const float* buf = nullptr;
    int64_t base = 0, resident = 0;
    static int same_device(const char* who, const char* what, int device, const char* reader, int reader_device);
    int open_slot(wlx_engine* e, int slot);                                   // engine.hip
    int item(const char* who, int first, int count = 1);                     // slot: [first, first + count) inside [0, B); views `first`
    void view(int item);                                                      // slot: another item of that span
    int range(const char* who, int64_t start, int64_t n, const float** p = nullptr) const;   // the residency refusal (WLX_ERR_STATE), else the samples
    int order(hipStream_t reader);                                            // before the reader's launches (nothing to do on a ring)
    void open_ring(wlx_ring* r);                                              // ring.hip
    int before_launch(hipStream_t reader);
    int launched(hipStream_t reader);

private:
    SlotGuard sg_;
    std::unique_lock<std::mutex> lane_;
    wlx_ring* r_ = nullptr;
    int item_ = -1;
};

extern std::atomic<int> g_dedicated_live[64];      // live slots with a hardware queue of their own, per device (create_slot_stream)
extern std::atomic<int> g_slots_live[64];          // live slots per device

// wlx_generate's pinned set-up staging (Slot::h_gen): [SearchParams | cum | rule | nsp | plen | ancestry rows | decode row tables].
// One layout for the allocation (wlx_slot_create: base = nullptr, only `bytes` is read) and the call (generate_impl).
struct GenStaging {
    SearchParams* sp; float* cum; int* rule; int* nsp; int* plen; short* anc; int* rows;
    size_t bytes;
};
GenStaging gen_staging(unsigned char* base, int rows_cap, int B);                         // engine_decode.hip

bool device_is_busy(const Slot* s);
void decoder_pass(Engine* e, Slot* s, const DecBufs& b, int rows, int R, int groups, bool with_logits, bool check_done, bool one_pass_prefill = false);
int upload_rows(Slot* s, const std::vector<int>& token, const std::vector<int>& pos, const std::vector<int>& cache,
                const std::vector<int>& ancrow, const std::vector<int>& group_item);
int prefill_tokens(Engine* e, Slot* s, int item, int crow, const int* tokens, int pos0, int n, float* logits_host, int nsp_index, int nsp_token,
                   float* nsp_out);
int set_anc_rows(Slot* s, const std::vector<short>& anc_host, int first_row, int nrows);
void launch_search(Engine* e, Slot* s, int rows, int R, int groups, bool sampling);
void launch_bias(Slot* s, int rows);                       // in front of launch_search: nothing without a bias table
int generate_impl(Engine* e, Slot* s, int batch, const int32_t* prompts, const int32_t* plens, int pstride, const int32_t* enc_items,
                  const wlx_gen_opts* o, bool injected_logits, const float* inj, int inj_steps, int32_t* tokens_out, int tstride,
                  int32_t* n_tokens_out, float* scores_out, float* nsp_out);

}  // namespace wlx
