/*
 * wlx.h — C-ABI of libwlx.so, the MI355X-native (gfx950) Whisper streaming-inference engine.
 *
 * This is the drop-in boundary #3 of SURVEY.md §8(b): it replaces the five call sites through
 * which collabora/WhisperLive reaches its un-vendored numerical engines (faster-whisper /
 * CTranslate2), each entry point citing the reference interface it stands in for
 * (paths relative to the reference checkout):
 *
 *   wlx_logmel            <- faster_whisper FeatureExtractor.__call__
 *                            (whisper_live/transcriber/transcriber_faster_whisper.py:655,862;
 *                             whisper_live/batch_inference.py:258; recipe restated in-tree at
 *                             whisper_live/transcriber/tensorrt_utils.py:177-190)
 *   wlx_encode            <- ctranslate2.models.Whisper.encode
 *                            (transcriber_faster_whisper.py:1339-1348; batch_inference.py:270-271)
 *   wlx_generate          <- ctranslate2.models.Whisper.generate
 *                            (transcriber_faster_whisper.py:1394-1407; batch_inference.py:355-357)
 *   wlx_detect_language   <- ctranslate2.models.Whisper.detect_language
 *                            (transcriber_faster_whisper.py:1140,1771; batch_inference.py:283)
 *   wlx_features_set/get  <- ctranslate2.StorageView.from_array
 *                            (transcriber_faster_whisper.py:1820-1823)
 *
 * Conventions: plain pointers and sizes only (no torch / C++ types); every function returns
 * 0 on success and a non-zero wlx_status otherwise (no exceptions cross the boundary, no
 * callbacks into the host language); wlx_last_error() returns a thread-local message.
 * Threading: concurrent calls are safe on DISTINCT slots (each slot owns a HIP stream and all
 * of its scratch); calls on the same slot are to be serialised by the caller, which is what the
 * reference does (one transcription thread per client, faster_whisper_backend.py:121; or the
 * single batch-worker thread, batch_inference.py:155-187). The library enforces it: a second call
 * on a busy slot returns WLX_ERR_STATE instead of running, wlx_slot_destroy waits for the call in
 * flight, slot ids are never reused. No entry point uses the legacy (null) HIP stream, so slot
 * creation and destruction are safe while other slots are decoding.
 * NULL-stream caveat for embedding applications: by default a slot's stream is created with
 * hipExtStreamCreateWithCUMask (all CUs enabled) so that it owns a hardware queue (the first
 * WLX_DEDICATED_QUEUES = 4 live slots of a device). That constructor takes no flags:
 * the stream is a BLOCKING stream (hipStreamGetFlags == 0), i.e. it synchronises implicitly with
 * the legacy NULL stream of the process. Work that the embedding process issues on the NULL stream
 * of the same device (a framework's default stream, a synchronous hipMemcpy) therefore serialises
 * with every slot, and if it is issued while a slot captures its decode-step graph that one
 * wlx_generate call fails with WLX_ERR_HIP (the slot's stream is replaced, the next call works).
 * Such processes should set WLX_SLOT_CU_MASK=off (ordinary non-blocking streams on the shared queue
 * pool) — and get exactly that by DEFAULT (round 5) once any weight tensor has been handed to
 * wlx_engine_create with on_device = 1, i.e. when the process demonstrably holds device memory of
 * another runtime; an explicit WLX_SLOT_CU_MASK always wins. The flag is process-wide and sticky; a
 * slot created BEFORE the first such engine gives its blocking stream back at its next call
 * (round 6), so no creation order has to be observed. The library states the mode on stderr at the
 * first slot creation in each mode (WLX_QUIET silences it). wlx_slot_create estimates the slot's
 * device memory first and refuses (WLX_ERR_NOMEM, with the figure) what the device cannot hold.
 */
#ifndef WLX_H
#define WLX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WLX_ABI_VERSION 1

typedef enum {
    WLX_OK = 0,
    WLX_ERR_ARG = 1,      /* bad argument / shape */
    WLX_ERR_HIP = 2,      /* a HIP runtime call failed */
    WLX_ERR_WEIGHT = 3,   /* missing / mis-shaped weight tensor */
    WLX_ERR_STATE = 4,    /* call order (e.g. generate before encode) */
    WLX_ERR_NOMEM = 5,
    WLX_ERR_TOO_SHORT = 6,/* speaker embedding: under 0.3 s of audio (the caller labels the segment with no speaker) */
    WLX_ERR_DATA = 7      /* damaged input (wlx_flac_probe, wlx_pcm_put_flac, wlx_wav_probe, wlx_pcm_put_wav: a file that is not a refused SHAPE but broken) */
} wlx_status;

/* Whisper architecture. n_audio_ctx = 1500, n_text_ctx = 448, head_dim = 64. */
typedef struct {
    int32_t n_mels;       /* 80 | 128 */
    int32_t d_model;
    int32_t n_heads;
    int32_t enc_layers;
    int32_t dec_layers;
    int32_t ffn;
    int32_t vocab;
    int32_t n_audio_ctx;  /* 1500 */
    int32_t n_text_ctx;   /* 448  */
} wlx_spec;

/* One weight tensor, named with the Hugging Face Whisper state-dict key (e.g.
 * "model.encoder.layers.0.self_attn.q_proj.weight"), **float32 only**, C-contiguous, in host or device
 * memory (there is no dtype field: a half-precision checkpoint must be widened by the caller — the Python binding,
 * whisperlive_amd/engine.py, does `tensor.to(float32)` for fp16 / bf16 torch tensors, a transient device copy of that ONE
 * tensor list; the values are unchanged, the engine rounds projection matrices to fp16 itself). The engine copies/repacks
 * every tensor into its own MFMA-fragment layout during create; the caller may free the tensors afterwards. */
typedef struct {
    const char* name;
    const void* data;
    int32_t ndim;
    int64_t shape[4];
    int32_t on_device;    /* 0 = host pointer, 1 = HIP device pointer on `device` */
} wlx_tensor;

typedef struct wlx_engine wlx_engine;

/* Token ids the decoding rules need; resolved by NAME on the host side from tokenizer.json
 * (never hard-coded). */
typedef struct {
    int32_t sot, eot, no_timestamps, timestamp_begin, no_speech, blank /* id of " " or -1 */;
} wlx_token_ids;

/* Decoding options = the keyword arguments of ctranslate2 Whisper.generate as the reference
 * passes them (transcriber_faster_whisper.py:1380-1407). */
typedef struct {
    int32_t beam_size;                 /* T=0: 5 ; T>0: 1 */
    float   patience;                  /* 1 ; round(beam_size * patience) <= 32, else WLX_ERR_ARG */
    int32_t num_hypotheses;            /* T=0: 1 ; T>0: best_of=5 */
    float   length_penalty;            /* 1 */
    float   repetition_penalty;        /* 1 */
    int32_t no_repeat_ngram_size;      /* 0 */
    int32_t max_length;                /* prompt + generated, <= 448 */
    int32_t suppress_blank;            /* bool */
    const int32_t* suppress_tokens;    /* may be NULL */
    int32_t n_suppress_tokens;
    int32_t max_initial_timestamp_index; /* 50 */
    int32_t sampling_topk;             /* 0 = whole vocabulary (only value used by the reference for T>0); 1 = greedy */
    float   sampling_temperature;      /* 0 -> beam search */
    uint64_t seed;                     /* counter-based RNG seed for T>0 */
    wlx_token_ids ids;
} wlx_gen_opts;

/* Per-stage GPU times of the last calls on a slot, milliseconds (HIP events on the slot stream). */
typedef struct {
    float logmel_ms, encode_ms, generate_ms;
    int32_t decode_steps;
} wlx_timings;

int32_t wlx_abi_version(void);
const char* wlx_last_error(void);

int32_t wlx_engine_create(const wlx_spec* spec, const wlx_tensor* weights, int32_t n_weights,
                          int32_t device, wlx_engine** out);
void    wlx_engine_destroy(wlx_engine* e);
int32_t wlx_engine_spec(const wlx_engine* e, wlx_spec* out);

/* A slot = one unit of concurrency: its own HIP stream plus every device buffer a call needs
 * (feature ring, encoder activations, cross-attention K/V, self-attention KV cache, beam state),
 * sized for `max_batch` audio items (<= 64) and `max_rows_per_item` decoder rows (beams, <= 16) per item;
 * max_batch * max_rows_per_item <= 320 decoder rows per step (64 clips x beam 5: the reference's worker takes any
 * max_batch_size, whisper_live/batch_inference.py:113-121 — wider batches than a slot holds are decoded as consecutive
 * groups over the same resident encoder output by the host side). */
int32_t wlx_slot_create(wlx_engine* e, int32_t max_batch, int32_t max_rows_per_item, int32_t* slot_out);
int32_t wlx_slot_destroy(wlx_engine* e, int32_t slot);

/* log-mel of `n` float32 PCM samples (host pointer, 16 kHz mono) for item `item` of the slot.
 * Result stays on the device as float32 [n_mels, n_frames], n_frames = (n+160)/160. */
int32_t wlx_logmel(wlx_engine* e, int32_t slot, int32_t item, const float* pcm, int64_t n,
                   int32_t* n_frames_out);
/* The same in two halves, for callers that keep the stream's PCM resident in HBM (the device-side
 * counterpart of the session buffer of whisper_live/backend/base.py:173-234): wlx_pcm_put copies
 * `n` host samples into the item's device PCM buffer; wlx_logmel_resident computes the features of
 * whatever is resident. wlx_logmel == wlx_pcm_put + wlx_logmel_resident.
 * Neither waits for the device, and the feature launches of a slot's items are RECORDED and issued together — one launch of each
 * kernel for all requested items — in front of the first call that consumes them (wlx_encode, wlx_features_get, wlx_features_set,
 * wlx_timings_get, wlx_sync) or that replaces a requested item's PCM: n_frames_out is a function of n alone, errors of the launch
 * itself surface at that later call. */
int32_t wlx_pcm_put(wlx_engine* e, int32_t slot, int32_t item, const float* pcm, int64_t n);
int32_t wlx_logmel_resident(wlx_engine* e, int32_t slot, int32_t item, int32_t* n_frames_out);
/* ---- file audio front end (PRODUCT entry points of the file path: transcribe(path), the REST endpoint) ----
 * Replaces the host-side down-mix and float64 scipy.signal.resample_poly of whisperlive_amd/audio_io.py load_audio (which stands in
 * for faster_whisper.audio.decode_audio, whisper_live/transcriber/transcriber_faster_whisper.py:821): the file's samples cross
 * PCIe ONCE, in their file format, and arrive as 16 kHz mono float32 in the item's PCM buffer.
 * `frames`: host pointer, interleaved [n_frames][channels], 1 <= channels <= WLX_PCM_MAX_CHANNELS; sample_format WLX_PCM_F32 (values
 * used as they are) or WLX_PCM_S16 (int16 scaled by 1 / 32768). Mono = the float32 mean (channels added in order, one division).
 * Output m = sum_j mono[j] * h[half_len + m * down - j * up] with up / down = 16000 / sample_rate reduced, half_len = 10 * max(up, down)
 * and h = up * firwin(2 * half_len + 1, 1 / max(up, down), window = ("kaiser", 5.0)) — the filter of scipy.signal.resample_poly's
 * defaults, designed by the library in double, rounded to float32 once, cached per ratio; float32 accumulation in a fixed order.
 * *n_out = ceil(n_frames * up / down) samples are resident afterwards and a following wlx_logmel_resident behaves exactly as after
 * a wlx_pcm_put of those samples. sample_rate == 16000 converts and down-mixes only: the samples are copied, not filtered (mono F32:
 * bit-identical to wlx_pcm_put, negative zeros included).
 * RATES: a rate is served when max(up, down) <= 640 AND the tap table with the input span of 64 outputs fits 64 KB of LDS:
 *     (2 * half_len + 1) + floor((63 * down + 2 * half_len) / up) + 2 <= 16384 floats.
 * The second condition binds steep down-sampling only (up = 1: down <= 159, i.e. up to 2.544 MHz); every ratio with up >= down and
 * max <= 640 passes it. Served: 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 352800, 384000,
 * 768000 Hz among others. Any other rate (44101 Hz, say) is REFUSED with WLX_ERR_ARG before any launch: nothing is read, nothing
 * becomes resident, and the caller resamples on the host (whisperlive_amd/engine.py resample_supported restates the rule;
 * transcribe() answers a refusal with its host route). n_frames is bounded by the 3600 s of OUTPUT (plus one second of input).
 * The file streams through a bounded pinned staging buffer in blocks (8 MB of file bytes each, two in flight), each block carrying
 * the filter's history and look-ahead; the result does not depend on where the block seams fall. wlx_pcm_put's conventions hold:
 * at most 3600 s of OUTPUT, the PCM buffer grows, recorded log-mel requests that read the item go out first, one call per slot at
 * a time, never the null stream; the caller's frames may be reused on return. */
#define WLX_PCM_F32 0
#define WLX_PCM_S16 1
#define WLX_PCM_MAX_CHANNELS 8
int32_t wlx_pcm_put_frames(wlx_engine* e, int32_t slot, int32_t item, const void* frames, int64_t n_frames, int32_t channels,
                           int32_t sample_format, int32_t sample_rate, int64_t* n_out);
/* The CHANNEL-SPLIT form (BatchedInferencePipeline.transcribe(multichannel=True): a two-party call recording, one transcript per
 * channel): the same ONE upload of the interleaved frames through the same pinned staging blocks, but no down-mix — channel c
 * (0 <= c < channels) arrives as 16 kHz mono float32 in the PCM buffer of item first_item + c, *n_out samples resident in EACH of the
 * `channels` items. The kernel is the split instantiation of the one above (blockIdx.y = channel; it reads sample r * channels + c, no
 * mean, no division; same taps, tile, accumulation order and seam logic), so item first_item + c is BIT-IDENTICAL to
 * wlx_pcm_put_frames of the one-channel array frames[:, c], both formats, the 16 kHz copy path with its negative zeros included, and
 * independent of where block seams fall. Refused with WLX_ERR_ARG before any launch, every item's resident PCM left as it was:
 * first_item < 0 or first_item + channels > max_batch, and everything wlx_pcm_put_frames refuses. A failed run leaves no PCM resident
 * in any of the `channels` items; recorded log-mel requests that read any of them go out first. */
int32_t wlx_pcm_put_frames_split(wlx_engine* e, int32_t slot, int32_t first_item, const void* frames, int64_t n_frames, int32_t channels,
                                 int32_t sample_format, int32_t sample_rate, int64_t* n_out);
/* ---- FLAC front end (PRODUCT entry points of the file path, beside wlx_pcm_put_frames) ----
 * Replaces the Python FLAC decoder of whisperlive_amd/audio_io.py (read_flac: a loop over Rice symbols and LPC samples at well under
 * real time) in front of wlx_pcm_put_frames: the file's COMPRESSED bytes cross PCIe once, the frames are decoded in HBM — FLAC frames are
 * independent of one another, one lane each — and the existing resampler reads the decoded float32 frames there.
 * wlx_flac_probe is HOST ONLY (no device work, like wlx_vad_segments): the metadata blocks up to the last one, STREAMINFO, and the frame
 * index, built WITHOUT decoding: a position starts a frame only if its header parses with no reserved code, its CRC-8 matches, its
 * coded frame / sample number (UTF-8 style, up to 36 bits; fixed and variable block size) is the expected next one and the CRC-16 of the
 * previous frame's bytes up to it matches; anything less is a false sync inside a frame. The last frame ends at the end of the data
 * (bytes behind the last frame, a trailing tag for instance, fail its CRC-16). *out: the stream's shape, its frame count, and
 * served = 1 when wlx_pcm_put_flac takes it: 1..8 channels, <= 24 bits per sample, <= 3600 s, a rate wlx_pcm_put_frames serves (RATES).
 * WLX_ERR_DATA, a DAMAGED stream: no fLaC magic, metadata past the end, no STREAMINFO, lost sync, a frame number out of sequence, no
 * CRC-consistent continuation, a sample count that disagrees with STREAMINFO. WLX_ERR_ARG, a container or shape the index does not take
 * apart: Ogg FLAC, an ID3 tag in front of the magic, a frame that changes the rate, width, channel count or blocking mid-stream.
 * wlx_pcm_put_flac: afterwards the item's resident PCM is BIT-IDENTICAL to that of wlx_pcm_put_frames(read_flac(bytes), WLX_PCM_F32,
 * channels, sample_rate): integers of at most 24 bits are exact in float32 and the scale 2^-(bps - 1) is a power of two, so the device
 * frames are read_flac's float64 quotients rounded to float32, and from there it is the same kernel on the same values (one launch
 * over the whole file; the result does not depend on block seams). *info_out (nullable) as wlx_flac_probe, written whenever the index
 * succeeds; *n_out = samples resident. Everything wlx_flac_probe can find, a stream with served = 0 (WLX_ERR_ARG: the caller decodes on
 * the host, as for an unserved WAV rate) and a scratch that cannot be had (WLX_ERR_NOMEM) are answered BEFORE any launch and leave the
 * item's resident PCM exactly as it was. Then: one upload of the bytes and the frame table through the slot's pinned staging blocks (two
 * in flight), the frame decode, the finish (stereo decorrelation, scale, interleave), the resample, ONE wait, and the per-frame status
 * words are read: a frame that does not decode (ran past its end, reserved code, inconsistent partition order, did not end exactly at
 * its CRC-16) gives WLX_ERR_DATA and leaves NO PCM resident in the item, as a failed wlx_pcm_put_frames run does. The decoder is
 * memory-safe on any bit pattern. The STREAMINFO MD5 is NOT checked on this route (it would mean downloading the samples): the CRC-16
 * of every frame on the host and the end check of every frame on the device stand in for it. The scratch (bytes, table, int32 planes,
 * float32 frames: ~8 bytes per sample and channel) is the slot's, grows on demand, and at most 16 MB of it stay allocated after the
 * call. wlx_pcm_put's conventions hold: recorded log-mel requests that read the item go out first, one call per slot at a time, never
 * the null stream; the caller's bytes may be reused on return. */
typedef struct {
    int32_t sample_rate, channels, bits_per_sample;
    int64_t total_samples;
    int32_t n_frames, max_blocksize;
    int32_t served;   /* 1: wlx_pcm_put_flac takes it; 0: host route */
} wlx_flac_info;
int32_t wlx_flac_probe(const void* bytes, int64_t n_bytes, wlx_flac_info* out);
int32_t wlx_pcm_put_flac(wlx_engine* e, int32_t slot, int32_t item, const void* bytes, int64_t n_bytes, wlx_flac_info* info_out,
                         int64_t* n_out);
/* The CHANNEL-SPLIT form: the same probe, upload, frame decode and finish, then ONE split resample launch over the device frames (the
 * kernel of wlx_pcm_put_frames_split) and ONE wait. Item first_item + c is BIT-IDENTICAL to wlx_pcm_put_frames(read_flac(bytes)[:, c]);
 * *n_out samples are resident in each of the stream's `channels` items. WLX_ERR_DATA, WLX_ERR_ARG and WLX_ERR_NOMEM as
 * wlx_pcm_put_flac, and first_item < 0 or first_item + channels > max_batch is WLX_ERR_ARG: all before any launch, every item's
 * resident PCM left as it was. A frame that does not decode gives WLX_ERR_DATA and leaves NO PCM resident in any of the items. */
int32_t wlx_pcm_put_flac_split(wlx_engine* e, int32_t slot, int32_t first_item, const void* bytes, int64_t n_bytes,
                               wlx_flac_info* info_out, int64_t* n_out);
/* ---- telephony WAV front end (PRODUCT entry points of the file path, beside wlx_pcm_put_flac) ----
 * The WAVE formats call recorders write — G.711 mu-law / A-law (format tags 7 / 6), IMA / DVI ADPCM (0x11), Microsoft ADPCM (0x02),
 * WAVE_FORMAT_EXTENSIBLE wrappers included — go to the device as they are: the data chunk crosses PCIe once, one byte (G.711) or half a
 * byte (ADPCM) per sample, and is decoded in HBM in front of the resampler. whisperlive_amd/audio_io.py read_wav is the host decoder of
 * the same formats: the oracle of the tests and the fallback for what this route refuses.
 * wlx_wav_probe is HOST ONLY: the RIFF chunks up to `data` (`fmt `, `fact`), the frame count, and for the ADPCM tags every block's
 * header. IMA: per channel a 4-byte block header (int16 predictor, uint8 step index, reserved), then 4-byte words interleaved by
 * channel, low nibble first; samples_per_block = (block_align - 4 ch) * 2 / ch + 1. MS: predictor index (uint8), delta, sample1,
 * sample2 (int16), each field for all channels in turn, then nibbles, high first, interleaved by channel; samples_per_block =
 * (block_align - 7 ch) * 2 / ch + 2; coefficient pairs from the fmt extension (wNumCoef, pairs), the 7 standard pairs without one.
 * n_frames = whole blocks * samples_per_block (a trailing partial block is dropped), cut to the `fact` chunk's count when that is
 * present, non-zero and smaller; G.711: data bytes / channels. served = 1 when wlx_pcm_put_wav takes the file: one of the four tags,
 * 8 bits (G.711) or 4 bits (ADPCM) per sample, 1..8 channels, at least one frame and at most 3600 s, a rate wlx_pcm_put_frames serves
 * (RATES), and for ADPCM a block_align the formulas accept (IMA: whole words; MS: whole nibble rounds; at least the header), at most
 * 32 coefficient pairs, and a block whose bytes and samples fit the decoder's 64 KB of LDS (5 * block_align, about 13000 bytes).
 * Tags 1 and 3 and anything else: served = 0 with the header fields filled in (the caller keeps the route it has).
 * WLX_ERR_DATA, a DAMAGED file: no RIFF / WAVE magic, no `fmt ` or `data` chunk, 0 channels, an IMA step index above 88, an MS
 * predictor index >= wNumCoef.
 * wlx_pcm_put_wav: afterwards the item's resident PCM is BIT-IDENTICAL to that of wlx_pcm_put_frames(read_wav(bytes), WLX_PCM_F32,
 * channels, sample_rate): every decoded value is an int16 scaled by 2^-15, exact in float32, so both routes feed the same kernel the
 * same floats, and a resampler output depends on nothing but the absolute input indices (not on block seams). *info_out (nullable) as
 * wlx_wav_probe, written whenever the probe succeeds; *n_out = samples resident. Everything the probe can find, a file with served = 0
 * (WLX_ERR_ARG: the caller decodes on the host) and a scratch that cannot be had (WLX_ERR_NOMEM) are answered BEFORE any launch and
 * leave the item's resident PCM exactly as it was. Then, tags 6 / 7: no decode launch, the code bytes are the resampler's input
 * (wlx_pcm_put_frames's staging, one byte per sample; wlx_pcm_put_frames itself keeps refusing the 8-bit codes). Tags 0x11 / 0x02:
 * one upload of the data chunk through the slot's pinned staging blocks (two in flight), the block decode (one lane per block and
 * channel, memory-safe on any bytes) into float32 interleaved frames in the slot's scratch, the resample launch over them, ONE wait.
 * A failed run leaves NO PCM resident in the item. The scratch (data chunk and float32 frames) is the one wlx_pcm_put_flac uses: the
 * slot's, grown on demand, at most 16 MB of it stay allocated after the call. wlx_pcm_put's conventions hold: recorded log-mel
 * requests that read the item go out first, one call per slot at a time, never the null stream; the caller's bytes may be reused on
 * return. */
typedef struct {
    int32_t format_tag;          /* the real tag behind a WAVE_FORMAT_EXTENSIBLE wrapper */
    int32_t channels, sample_rate, bits_per_sample, block_align;
    int32_t samples_per_block;   /* per channel; 1 for G.711 and PCM; 0 for a layout the formulas refuse */
    int64_t data_offset, data_bytes;   /* the data chunk's body within `bytes` (clipped to n_bytes) */
    int64_t n_frames;
    int32_t served;              /* 1: wlx_pcm_put_wav takes it; 0: the caller's other routes */
} wlx_wav_info;
int32_t wlx_wav_probe(const void* bytes, int64_t n_bytes, wlx_wav_info* out);
int32_t wlx_pcm_put_wav(wlx_engine* e, int32_t slot, int32_t item, const void* bytes, int64_t n_bytes, wlx_wav_info* info_out,
                        int64_t* n_out);
/* The CHANNEL-SPLIT form: the same probe, upload and decode, then ONE split resample launch (G.711: per staged block) and ONE wait.
 * Item first_item + c is BIT-IDENTICAL to wlx_pcm_put_frames(read_wav(bytes)[:, c]); *n_out samples are resident in each of the file's
 * `channels` items. WLX_ERR_DATA, WLX_ERR_ARG and WLX_ERR_NOMEM as wlx_pcm_put_wav, and first_item < 0 or first_item + channels >
 * max_batch is WLX_ERR_ARG: all before any launch, every item's resident PCM left as it was. */
int32_t wlx_pcm_put_wav_split(wlx_engine* e, int32_t slot, int32_t first_item, const void* bytes, int64_t n_bytes,
                              wlx_wav_info* info_out, int64_t* n_out);
/* ---- a WAVE of files in one call (PRODUCT entry point of BatchedInferencePipeline.transcribe_many(wave_put=True); csrc/put_many.hip) ----
 * Entry k (k < n <= WLX_PUT_MANY_MAX) goes into item first_item + k, in the down-mix (mono) form, under the contract of the single-file
 * entry point of its kind: results[k].status == WLX_OK: the item holds results[k].n_out samples, BIT-IDENTICAL to what wlx_pcm_put /
 * wlx_pcm_put_frames / wlx_pcm_put_flac / wlx_pcm_put_wav leaves for that input, and a following wlx_logmel_resident behaves as after
 * that call. WLX_ERR_ARG, a REFUSED entry (an unserved rate, a stream with served = 0, more than 3600 s, an unknown kind, an entry whose
 * scratch need alone exceeds the budget below): decided on the host before any launch, the item is left exactly as it was. WLX_ERR_DATA,
 * a DAMAGED entry: what the probe finds is answered before any launch and leaves the item as it was; a FLAC frame that does not decode
 * on the device leaves NO PCM resident in that item. In every case the other entries are unaffected.
 * The CALL returns WLX_OK whenever it ran, even if entries failed. WLX_ERR_ARG before anything is touched: n < 1, n > WLX_PUT_MANY_MAX,
 * first_item < 0, first_item + n > max_batch, a null pointer. WLX_ERR_NOMEM before any launch. A HIP error is the call's error: no item
 * of the call keeps PCM.
 * ONE WAIT: every upload (through the slot's pinned staging blocks; waiting for the event that frees a staging half is the only other
 * wait, as in wlx_pcm_put_frames) and every launch is enqueued on the slot's stream, the host waits once, then reads the FLAC status
 * words. Launches per call: one ragged resample launch for all entries that are not waveforms, one frame-decode and one finish launch
 * for all FLAC entries, one decode launch per ADPCM file (it takes no wait) - a count that depends on the kinds present, not on n.
 * Scratch (file bytes, frame tables, status words, int32 planes, float32 frames) is the slot's FLAC / WAV scratch, bounded by a BUDGET
 * of 256 MB per call: entries whose needs do not fit it together run as consecutive sub-batches that reuse the scratch in stream order,
 * still behind the one wait; at most 16 MB stay allocated after the call. wlx_pcm_put's conventions hold: the PCM buffers grow once, to
 * the longest served entry, before any launch; recorded log-mel requests that read a target item go out first; one call per slot at a
 * time; never the null stream; the caller's memory may be reused on return. */
#define WLX_PUT_PCM    0   /* float32 16 kHz mono samples: what wlx_pcm_put takes            */
#define WLX_PUT_FRAMES 1   /* interleaved frames: what wlx_pcm_put_frames takes (F32 / S16)   */
#define WLX_PUT_FLAC   2   /* the bytes of a FLAC file: what wlx_pcm_put_flac takes           */
#define WLX_PUT_WAV    3   /* the bytes of a telephony WAV file: what wlx_pcm_put_wav takes   */
#define WLX_PUT_MANY_MAX 64
typedef struct { int32_t kind; const void* data; int64_t n;   /* samples | frames | bytes */
                 int32_t channels, sample_format, sample_rate; /* WLX_PUT_FRAMES only */ } wlx_put_entry;
typedef struct { int32_t status; int64_t n_out; } wlx_put_result;
int32_t wlx_pcm_put_many(wlx_engine* e, int32_t slot, int32_t first_item, int32_t n,
                         const wlx_put_entry* entries, wlx_put_result* results);
/* ---- batched long-form front end (PRODUCT entry points of BatchedInferencePipeline: whisperlive_amd/batched.py) ----
 * Replaces faster_whisper.vad.collect_chunks + one FeatureExtractor call per chunk of the reference's BatchedInferencePipeline.transcribe
 * (whisper_live/transcriber/transcriber_faster_whisper.py:424-429): B chunks are cut out of ONE resident PCM buffer into B feature items
 * by one launch of each log-mel kernel, nothing crosses PCIe but the range tables.
 * Chunk c (0 <= c < n_chunks) is the concatenation of the ranges [ranges[2 i], ranges[2 i + 1]) for range_off[c] <= i < range_off[c + 1]
 * (range_off[0] = 0): sample positions in the resident PCM of `src_item` as wlx_pcm_put / wlx_pcm_put_frames left it; within a chunk
 * ascending, non-empty, touching allowed, overlapping not; 1..WLX_LM_MAXRANGES ranges per chunk. The features of chunk c land in item
 * first_item + c (first_item + n_chunks <= max_batch) and are bit-identical to wlx_logmel on the concatenated samples;
 * n_frames_out[c] = (n_c + 160) / 160. The range tables are staged through a pinned buffer of the slot. Log-mel requests recorded
 * earlier go out first; the launch is issued at once.
 * AFTERWARDS the source item's PCM is still resident and unchanged (the next group of chunks reads it again), also when the source is
 * one of the destination items: wlx_logmel_resident on it then computes the features of the WHOLE resident PCM again. Every OTHER
 * destination item holds features its own PCM buffer does not stand for, so — as after wlx_logmel_ring — it counts as having no PCM
 * resident: wlx_logmel_resident on it returns WLX_ERR_STATE until a wlx_pcm_put.
 * Every refusal happens before any launch and nothing is written. WLX_ERR_ARG: null pointers, a chunk with 0 or more than
 * WLX_LM_MAXRANGES ranges, a range that is empty, out of order or overlapping, items out of range. WLX_ERR_STATE: no PCM resident in
 * src_item, a range that ends past the resident count. */
#define WLX_LM_MAXRANGES 256
int32_t wlx_logmel_chunks(wlx_engine* e, int32_t slot, int32_t src_item, const int64_t* ranges, const int32_t* range_off,
                          int32_t n_chunks, int32_t first_item, int32_t* n_frames_out);
/* wlx_logmel_chunks with a source PER CHUNK (the channels of a file, wlx_pcm_put_frames_split): chunk c is cut out of the resident PCM
 * of item src_items[c] (src_items: n_chunks entries), everything else as above — still ONE launch of each log-mel kernel for the whole
 * group whatever the mix of sources, the features of chunk c bit-identical to wlx_logmel on the concatenated samples of ITS source.
 * (A slot's PCM is one allocation with one row per item: the launch gets the row of the lowest source as its base and the range
 * starts of the other sources are offset on the host; the kernel is the one wlx_logmel_chunks launches.)
 * AFTERWARDS every item named in src_items keeps its PCM resident and unchanged; a destination item that is not a source counts as
 * having no PCM resident. Refusals before any launch, nothing written: everything wlx_logmel_chunks refuses, checked per chunk
 * against the resident count of that chunk's own source; a null src_items (WLX_ERR_ARG); a source item outside the slot (WLX_ERR_ARG)
 * or with no PCM resident (WLX_ERR_STATE); sources whose rows lie more than 2^31 - 1 samples apart (WLX_ERR_ARG: hours of audio in
 * items far apart — use neighbouring items). */
int32_t wlx_logmel_chunks_multi(wlx_engine* e, int32_t slot, const int32_t* src_items, const int64_t* ranges, const int32_t* range_off,
                                int32_t n_chunks, int32_t first_item, int32_t* n_frames_out);
/* Copy the item's resident PCM (wlx_pcm_put / wlx_pcm_put_frames) to the host: *n_out samples (nullable `out`: the count only). */
int32_t wlx_pcm_get(wlx_engine* e, int32_t slot, int32_t item, float* out, int64_t cap, int64_t* n_out);
/* Copy an item's device features to host / replace them from host (float32 [n_mels, n_frames]). */
int32_t wlx_features_get(wlx_engine* e, int32_t slot, int32_t item, float* out, int64_t cap_floats,
                         int32_t* n_frames_out);
int32_t wlx_features_set(wlx_engine* e, int32_t slot, int32_t item, const float* feats,
                         int32_t n_mels, int32_t n_frames);

/* Encoder forward for items 0..batch-1. Item i uses feature frames [seek[i], seek[i]+seg[i]),
 * zero-padded (in log-mel space) to 3000 = pad_or_trim (transcriber_faster_whisper.py:1125-1127).
 * Leaves encoder output [batch,1500,d] and the cross-attention K/V of every decoder layer on the device. */
int32_t wlx_encode(wlx_engine* e, int32_t slot, int32_t batch, const int32_t* seek, const int32_t* seg);
/* float32 copy of the encoder output of one item, [1500, d_model]. */
int32_t wlx_encoder_output_get(wlx_engine* e, int32_t slot, int32_t item, float* out, int64_t cap_floats);

/* Autoregressive decode for items 0..batch-1 (item i uses prompt i). Outputs, per item and
 * hypothesis h < num_hypotheses (best first): generated token ids (prompt and EOT excluded),
 * their count, the CT2-style score (sum of log-probs incl. EOT / len^length_penalty), and per
 * item the no-speech probability (softmax prob. of ids.no_speech at the sot position).
 * The call returns when the results are final, which can be BEFORE the slot's stream is idle: the search kernels store the
 * results in pinned host memory and order them before the "done" word the host polls, so a decode that ends on an end-of-text
 * does not wait for the one step that was already enqueued behind the finish (~0.4 ms on Whisper-small). Later calls on the
 * slot are ordered behind it on the stream; wlx_timings_get / wlx_sync wait for it. */
int32_t wlx_generate(wlx_engine* e, int32_t slot, int32_t batch,
                     const int32_t* prompts, const int32_t* prompt_lens, int32_t prompt_stride,
                     const wlx_gen_opts* opts,
                     int32_t* tokens_out, int32_t tokens_stride /* per hypothesis */,
                     int32_t* n_tokens_out, float* scores_out, float* no_speech_prob_out);

/* The same with an item map: decoder item i attends to the encoder output of item enc_items[i]
 * (NULL = identity). Lets the batched fallback of whisper_live/batch_inference.py:318-384 retry a subset
 * of a batch without re-encoding it (the reference re-encodes, :334-339). */
int32_t wlx_generate_ex(wlx_engine* e, int32_t slot, int32_t batch, const int32_t* enc_items,
                        const int32_t* prompts, const int32_t* prompt_lens, int32_t prompt_stride,
                        const wlx_gen_opts* opts,
                        int32_t* tokens_out, int32_t tokens_stride,
                        int32_t* n_tokens_out, float* scores_out, float* no_speech_prob_out);

/* ---- keyword boosting: a bias table on the slot (the host compiler is whisperlive_amd/biasing.py) ----
 * While a table is installed every decode step of the slot (wlx_generate / wlx_generate_ex in beam and sampling mode, and the
 * wlx_debug_search hooks) runs ONE more launch between the vocabulary projection and the token search, which adds to each live row's
 * logits, BEFORE anything of the search reads them (pre-softmax, like OpenAI's logit_bias: normalisation, suppress mask, timestamp
 * rules, penalties and sampling all see the biased row, and the scores / avg_logprob move with it):
 *   1. `boost` on every edge token of the row's node, one float32 add;
 *   2. then tok_vals[i] on tok_ids[i] for every entry of the token list, one float32 add (in every node).
 * The table is an Aho-Corasick automaton over token ids with its failure links closed: node n (0 = root) owns the edges
 * [edge_off[n], edge_off[n + 1]) of (edge_tok, edge_next), the tokens ascending — every token that leads from n to a node other than
 * the root; any other token leads to the root, and so does every token >= opts->ids.eot (specials, timestamps). A node that ends a
 * phrase carries the root's edges (the walk restarts). A row's node at position p is next(node of its parent row at p - 1, token
 * fed at p), the root at the first generated position; the nodes are kept on the device per (cache row, position) and follow the
 * beam's re-ordering. A bonus given on a partial match is NOT taken back when the match breaks. A row whose raw distribution defines
 * no_speech_prob inside the search (the prompt ends on <|startoftranscript|>) is not biased at that step: no_speech_prob is the same
 * with and without a table.
 * The table, the states and the pinned staging of the upload live in buffers of the slot at fixed addresses (allocated at the first
 * call): captured step graphs stay valid across calls and across tables. The upload is asynchronous on the slot's stream.
 * WLX_ERR_ARG, the installed table (if any) untouched: n_nodes outside 1..WLX_BIAS_MAX_NODES, more than WLX_BIAS_MAX_EDGES edges,
 * n_tok outside 0..WLX_BIAS_MAX_TOKENS, offsets that do not start at 0 and ascend, edge tokens of a node that do not ascend, an
 * edge_next outside 1..n_nodes - 1, a token outside the vocabulary, a token named twice in tok_ids, a boost or value that is not finite.
 * wlx_bias_clear: the slot decodes without a table again (its step is the launch list it was before the first wlx_bias_set). */
#define WLX_BIAS_MAX_NODES 4096
#define WLX_BIAS_MAX_EDGES 16384
#define WLX_BIAS_MAX_TOKENS 1024
int32_t wlx_bias_set(wlx_engine* e, int32_t slot, int32_t n_nodes, const int32_t* edge_off, const int32_t* edge_tok,
                     const int32_t* edge_next, float boost, int32_t n_tok, const int32_t* tok_ids, const float* tok_vals);
int32_t wlx_bias_clear(wlx_engine* e, int32_t slot);

/* Keyword boosting per item — a set of tables on the slot, one selected per item of a decode group (wlx_bias_set_items, wlx_bias_select;
 * DESIGN.md §27) — is declared in wlx_bias_items.h, which this header includes at its end. So is grammar-constrained decoding — a closed
 * phrase list as a DFA on the slot, whose launch masks where these add (wlx_grammar_set, wlx_grammar_clear) — in wlx_grammar.h. */

/* One decoder step on [sot]; softmax restricted to `lang_ids`; probs_out[batch][n_lang]. */
int32_t wlx_detect_language(wlx_engine* e, int32_t slot, int32_t batch, int32_t sot,
                            const int32_t* lang_ids, int32_t n_lang, float* probs_out);

/* Device times of the slot's last log-mel / encode / generate (HIP events); waits for whichever of them is still running. */
int32_t wlx_timings_get(wlx_engine* e, int32_t slot, wlx_timings* out);
int32_t wlx_sync(wlx_engine* e, int32_t slot);

/* ---- word timestamps (PRODUCT entry point: transcribe(word_timestamps=True) calls it once per segment group) ---- */
/* Word alignment — replaces ctranslate2.models.Whisper.align(encoder_output, start_sequence, text_tokens, num_frames,
 * median_filter_width) (whisper_live/transcriber/transcriber_faster_whisper.py:1657-1663).
 * tokens = start_sequence (n_sot ids) + [no_timestamps] + text_tokens + [eot]  (n_tokens <= 448) of encoder item `item`;
 * heads = n_heads (layer, head) pairs (the model's alignment heads). Outputs: the DTW path as parallel arrays
 * text_indices / time_indices (n_path <= path_cap entries; time in encoder positions of 20 ms) and
 * text_token_probs[n_tokens - n_sot - 2] = softmax over ids < eot of each text token. */
int32_t wlx_align(wlx_engine* e, int32_t slot, int32_t item, const int32_t* tokens, int32_t n_tokens, int32_t n_sot,
                  int32_t num_frames, int32_t median_filter_width, const int32_t* heads, int32_t n_heads, int32_t eot,
                  int32_t* text_indices, int32_t* time_indices, int32_t path_cap, int32_t* n_path_out,
                  float* text_token_probs);

/* The same for a group of up to WLX_ALIGN_MAX_BATCH entries in ONE launch sequence with ONE wait at its end: entry i means what wlx_align
 * means for encoder item items[i] (NULL = identity; an item may repeat), the tokens at tokens[i * tokens_stride .. + n_tokens[i]) and
 * num_frames[i]. The teacher-forced pass runs entry by entry, 64 rows at a time, with the kernels of wlx_align (text_token_probs are
 * bit-identical to its); softmax / normalise / median / head mean and the DTW run ON THE DEVICE for all entries at once (csrc/align.hip),
 * in float32: the path of entry i is exactly the DTW of the float32 cost matrix the device computed for it. Outputs of entry i at
 * i * path_stride (text_indices, time_indices; n_path_out[i] steps) and i * probs_stride. n == 0 launches nothing.
 * WLX_ERR_ARG / WLX_ERR_STATE before any launch, nothing written: n outside 0..WLX_ALIGN_MAX_BATCH, a null pointer, an item that is
 * not encoded, n_tokens[i] outside n_sot + 3 .. 448, a bad head / token / eot (as wlx_align), median_filter_width even or outside
 * 1..WLX_ALIGN_MAX_MEDIAN, path_stride < n_tokens[i] - 1 - n_sot + frames of entry i (the longest path), probs_stride < n_tokens[i] - n_sot - 2.
 * WLX_ERR_NOMEM before any launch if the score scratch (n_heads * n_tokens[i] * 1536 floats per entry, grown on demand) cannot be had. */
#define WLX_ALIGN_MAX_BATCH 64
#define WLX_ALIGN_MAX_MEDIAN 15
int32_t wlx_align_batch(wlx_engine* e, int32_t slot, int32_t n, const int32_t* items,
                        const int32_t* tokens, const int32_t* n_tokens, int32_t tokens_stride, int32_t n_sot,
                        const int32_t* num_frames, int32_t median_filter_width,
                        const int32_t* heads, int32_t n_heads, int32_t eot,
                        int32_t* text_indices, int32_t* time_indices, int32_t path_stride, int32_t* n_path_out,
                        float* text_token_probs, int32_t probs_stride);

/* ---- voice-activity probabilities (Silero VAD, 16 kHz) — PRODUCT entry points: the VAD gate of every use_vad session ----
 * Replaces the model call inside faster_whisper.vad.get_speech_timestamps (onnxruntime, one CPU thread) that the
 * reference makes before every transcription when the client asks for VAD:
 * whisper_live/transcriber/transcriber_faster_whisper.py:830-838 and, per batch item, whisper_live/batch_inference.py:245-248;
 * I/O contract of the same network: whisper_live/vad.py:50-109 (512-sample windows, 64 samples of left context, zero
 * initial state, one probability per window). The hysteresis / padding / chunk bookkeeping that turns probabilities
 * into sample ranges stays on the host (whisperlive_amd/vad.py).
 * Weights: HOST pointers, float32 row-major, copied and repacked at creation:
 *   stft_basis [258,256]; enc_w[i] [Cout,Cin,3], enc_b[i] [Cout] with (Cin,Cout) = (129,128) (128,64) (64,64) (64,128);
 *   lstm_w_ih, lstm_w_hh [512,128] and lstm_b_ih, lstm_b_hh [512] in gate order i,f,g,o; out_w [128]; out_b [1]. */
typedef struct wlx_vad wlx_vad;
typedef struct {
    const float* stft_basis;
    const float* enc_w[4];
    const float* enc_b[4];
    const float* lstm_w_ih;
    const float* lstm_w_hh;
    const float* lstm_b_ih;
    const float* lstm_b_hh;
    const float* out_w;
    const float* out_b;
} wlx_vad_weights;
int32_t wlx_vad_create(const wlx_vad_weights* w, int32_t device, wlx_vad** out);
void    wlx_vad_destroy(wlx_vad* v);
/* `n` float32 samples (host pointer) -> ceil(n/512) probabilities (host buffer of `cap` floats); the last window is
 * zero-padded. Each call starts from a zero state, like get_speech_timestamps on a fresh chunk. Thread-safe (calls on
 * one object are serialised; it owns its HIP stream). device_ms_out (nullable): kernel time between HIP events.
 * The pass is that of wlx_vad_probs_batch (below) with one item; so are wlx_vad_probs_resident and wlx_vad_probs_pcm. */
int32_t wlx_vad_probs(wlx_vad* v, const float* pcm, int64_t n, float* probs_out, int32_t cap,
                      int32_t* n_windows_out, float* device_ms_out);

/* ---- device-resident PCM ring of ONE client stream (round 6; PRODUCT entry points of the streaming path) ----
 * The device-side mirror of the session buffer ServeClientBase keeps on the host (whisper_live/backend/base.py:173-234:
 * `frames_np`, the 45 s cap / 30 s trim of add_frames :191-198, the chunk taken by get_audio_chunk_for_processing :219-234).
 * Every packet a client sends crosses PCIe ONCE — wlx_ring_append — and everything that reads audio afterwards reads HBM:
 * the VAD gate (wlx_vad_probs_resident) and the log-mel front end, whose PCM -> LDS loads walk the list of speech ranges the
 * gate kept (wlx_logmel_ring: replaces faster_whisper.vad.collect_chunks + np.concatenate + a second upload,
 * transcriber_faster_whisper.py:836-838,862). A ring is independent of slots: the socket thread appends while the
 * transcription thread reads; calls on one ring are serialised by the library.
 * Sample positions are ABSOLUTE stream positions (sample 0 = the first sample ever appended): a trim moves `base`,
 * never the positions a caller already holds. A range that has been trimmed away fails with WLX_ERR_STATE. */
typedef struct wlx_ring wlx_ring;
int32_t wlx_ring_create(wlx_engine* e, int64_t capacity_samples /* 0: 64 s */, wlx_ring** out);
void    wlx_ring_destroy(wlx_ring* r);
/* add_frames (base.py:173-234): if more than `max_resident` samples are resident, the OLDEST `trim` samples are dropped
 * first (45 s / 30 s in the reference: pass 720000 / 480000; max_resident <= 0 disables the rule), then the `n` host
 * samples are appended. Outputs (nullable): samples dropped by this call, first resident position, resident count.
 * The copy is complete on return. */
int32_t wlx_ring_append(wlx_ring* r, const float* samples, int64_t n, int64_t max_resident, int64_t trim,
                        int64_t* dropped_out, int64_t* base_out, int64_t* resident_out);
int32_t wlx_ring_state(wlx_ring* r, int64_t* base_out, int64_t* resident_out);
/* ---- live sessions at any served sample rate (PRODUCT entry points of the streaming path) ----
 * A ring may be given a WIRE FORMAT once, before the first append: the client's packets then cross PCIe as they came off the socket
 * and are converted, down-mixed and resampled to 16 kHz on the device, packet by packet, by the kernel of wlx_pcm_put_frames.
 * sample_format: WLX_PCM_F32, WLX_PCM_S16, or one of the 8-bit formats below (code 2 is unassigned; the FILE entry points —
 * wlx_pcm_put_frames, wlx_pcm_put_frames_split, wlx_debug_resample* — keep taking F32 and S16 only). channels 1..WLX_PCM_MAX_CHANNELS,
 * down-mixed as the file path does (float32 mean, channels added in order, one division); sample_rate under the RATES rule of
 * wlx_pcm_put_frames. WLX_ERR_ARG: an unknown format, a bad channel count, an unserved rate. WLX_ERR_STATE: a ring that has a format
 * already or has been appended to. A refusal changes nothing. */
#define WLX_PCM_U8    3   /* (x - 128) / 128 */
#define WLX_PCM_MULAW 4   /* G.711 mu-law -> its 16-bit linear value / 32768 */
#define WLX_PCM_ALAW  5   /* G.711 A-law  -> its 16-bit linear value / 32768 */
int32_t wlx_ring_set_format(wlx_ring* r, int32_t sample_format, int32_t channels, int32_t sample_rate);
/* The streaming append of a ring with a format: `frames` = n_frames interleaved frames in the wire format (host). With J input frames
 * seen so far and M outputs in the stream, the call appends the outputs m in [M, M') at absolute positions m, J' = J + n_frames:
 *   flush == 0: every output whose newest input exists, floor((half_len + m * down) / up) <= J' - 1;
 *   flush != 0: M' = ceil(J' * up / down), the one-shot length, inputs past the end being zero; the stream is then CLOSED and
 *               further appends give WLX_ERR_STATE.
 * For ANY cutting of a stream into packets (empty ones, one-frame ones, ones shorter than the filter's reach) followed by a flush, the
 * concatenation of what the calls appended is BIT-IDENTICAL to wlx_pcm_put_frames / wlx_debug_resample of the concatenated frames:
 * same taps, same float32 accumulation order per output, zeros in front of the stream; no emitted sample is ever revised. At 16 kHz
 * in, the call converts and down-mixes only (M' = J').
 * The trim rule (max_resident, trim) is applied BEFORE the append exactly as in wlx_ring_append; dropped / base / resident are in
 * 16 kHz samples. new_out (nullable, `cap` floats): the call's M' - M new samples, copied to the host in the same wait (the session's
 * host mirror stays sample for sample with the ring); cap < M' - M is refused before any launch, nothing changed. *n_new_out = M' - M.
 * State of a stream: J, M, the last ceil(2 * half_len / up) + 2 input frames (device) and a staging buffer for [tail | packet], grown
 * on demand. The copy is complete on return; calls are serialised by the ring's mutex; the ring's own stream, never the null stream;
 * readers are waited for only where data moves under them. wlx_ring_append on a ring with a format is WLX_ERR_STATE; this call on a
 * ring without one is WLX_ERR_STATE. */
int32_t wlx_ring_append_frames(wlx_ring* r, const void* frames, int64_t n_frames, int32_t flush,
                               int64_t max_resident, int64_t trim,
                               float* new_out, int64_t cap, int64_t* n_new_out,
                               int64_t* dropped_out, int64_t* base_out, int64_t* resident_out);
/* Host only (no device work, like wlx_vad_segments): M' of the stream form as a function of J' = frames_seen alone. WLX_ERR_ARG for an
 * unserved rate or a negative count. */
int32_t wlx_resample_stream_count(int32_t sample_rate, int64_t frames_seen, int32_t flush, int64_t* n_out);
/* ---- live MULTICHANNEL sessions: one ring per channel, filled together (PRODUCT entry points of the streaming path) ----
 * A ring group holds `channels` LANES — one allocation [channels][capacity] — for a stream whose channels are kept apart (a telephony
 * bridge: agent on channel 0, customer on channel 1). A packet of interleaved frames crosses PCIe once and ONE launch of the
 * channel-split instantiation of the resampling kernel (blockIdx.y = channel: sample r * channels + c, no mean, no division) writes
 * every lane; the [tail | packet] staging and the device tail hold whole frames and are shared by the lanes.
 * wlx_ring_group_create: channels 1..WLX_PCM_MAX_CHANNELS, sample_format and sample_rate as wlx_ring_set_format, and its refusals
 * (WLX_ERR_ARG; nothing is created). capacity_samples is per lane (0: 64 s).
 * wlx_ring_group_lane: a BORROWED wlx_ring*, valid until wlx_ring_group_destroy. A lane is a full ring for every reader —
 * wlx_ring_state, wlx_vad_probs_resident, wlx_logmel_ring, wlx_spk_embed_ring_batch work on it unchanged — and a closed one for
 * writers: wlx_ring_append, wlx_ring_set_format and wlx_ring_append_frames on a lane are WLX_ERR_STATE, wlx_ring_destroy on a lane
 * does nothing. A lane index outside 0..channels - 1 is WLX_ERR_ARG.
 * wlx_ring_group_append_frames: the contract of wlx_ring_append_frames applied to all lanes in lockstep. ONE trim decision and ONE
 * growth serve all lanes, so every lane has the same base and resident at all times (dropped / base / resident are per lane, in
 * 16 kHz samples). Per call: one tail copy, one packet upload, one launch over [M, M') x channels, one new tail, one wait.
 * new_out (nullable): [channels][cap] floats, ONE copy back, lane c's M' - M new samples at new_out + c * cap; cap < M' - M is
 * refused before anything is enqueued, nothing changed. After a flush further appends are WLX_ERR_STATE.
 * For ANY cutting of a stream into packets followed by a flush, lane c is BIT-IDENTICAL to a mono ring given
 * wlx_ring_set_format(fmt, 1, rate) and fed channel c's frames with the same cutting, with equal dropped / base / resident at every
 * packet; hence to the one-shot resample of that channel, and for F32 / S16 to item c of wlx_pcm_put_frames_split.
 * Readers of a lane and the group's append are serialised as calls on one ring are (the append holds every lane's mutex); it waits
 * for pending readers only where data moves under them (a trim, a growth). The group's own stream, never the null stream. */
typedef struct wlx_ring_group wlx_ring_group;
int32_t wlx_ring_group_create(wlx_engine* e, int64_t capacity_samples /* per lane; 0: 64 s */, int32_t sample_format, int32_t channels,
                              int32_t sample_rate, wlx_ring_group** out);
void    wlx_ring_group_destroy(wlx_ring_group* g);
int32_t wlx_ring_group_lane(wlx_ring_group* g, int32_t channel, wlx_ring** out);
int32_t wlx_ring_group_append_frames(wlx_ring_group* g, const void* frames, int64_t n_frames, int32_t flush,
                                     int64_t max_resident, int64_t trim,
                                     float* new_out, int64_t cap, int64_t* n_new_out,
                                     int64_t* dropped_out, int64_t* base_out, int64_t* resident_out);
/* wlx_vad_probs on ring samples [start, start + n): no host-to-device copy. Same contract otherwise (zero initial
 * state, ceil(n / 512) windows, the last one zero-padded) plus `extra_zero_windows` all-zero windows behind them
 * (faster_whisper.vad pads n to the NEXT multiple of 512 — a whole window of zeros when n already is one — and the
 * host side asks for the same count, so the two paths segment identically). `v` and `r` must live on the same device. */
int32_t wlx_vad_probs_resident(wlx_vad* v, wlx_ring* r, int64_t start, int64_t n, int32_t extra_zero_windows,
                               float* probs_out, int32_t cap, int32_t* n_windows_out, float* device_ms_out);
/* wlx_vad_probs_resident with the resident PCM of a slot item (wlx_pcm_put / wlx_pcm_put_frames) in place of the ring: samples
 * [start, start + n) of item `item`, same contract, no host-to-device copy, and the VAD object's own PCM buffers (device
 * and pinned) do not grow with the file — only its per-window buffers do. The VAD object's stream is ordered behind the slot's stream
 * with an event (a wlx_pcm_put_frames resample may still be in flight), never through the null stream. The slot counts as busy for
 * the call (WLX_ERR_STATE on a busy slot). `v` and `e` on different devices: WLX_ERR_ARG; a span outside the resident samples:
 * WLX_ERR_STATE. */
int32_t wlx_vad_probs_pcm(wlx_vad* v, wlx_engine* e, int32_t slot, int32_t item, int64_t start, int64_t n, int32_t extra_zero_windows,
                          float* probs_out, int32_t cap, int32_t* n_windows_out, float* device_ms_out);
/* The gate of a BATCH (the batch worker's requests, whisper_live/batch_inference.py:245-248, where the reference calls the network once
 * per item): 1 <= n <= WLX_VAD_MAX_BATCH sequences of different lengths in ONE pass — one upload, one launch of each kernel, one
 * download, one wait. The recurrences are independent and run side by side, one workgroup (one CU) each.
 * wlx_vad_probs_batch: `pcm` holds the n segments back to back on the host, segment i of n_samples[i] samples.
 * T_i = ceil(n_samples[i] / 512) + extra_zero_windows[i] windows (0 <= extra <= 4, meaning as in wlx_vad_probs_resident; a null
 * `extra_zero_windows` is all 0). probs_out receives the rows packed in item order (sum T_i <= cap floats), n_windows_out[i] = T_i.
 * Row i does not depend on what else is in the batch, or in what order: every item starts from a zero state and no workgroup serves
 * two items. (wlx_vad_probs on segment i zero-padded to 512 * T_i samples is this pass with that one item, so it returns the same
 * bits.) An item with T_i == 0 takes no part (all empty: WLX_OK, nothing launched). WLX_ERR_ARG before any launch, nothing written:
 * n outside 1..WLX_VAD_MAX_BATCH, a null pointer, a negative count, an extra out of range, sum T_i > cap, more than 3600 s of
 * samples in all.
 * wlx_vad_probs_pcm_batch: the same on samples [0, n_samples[i]) of the resident PCM of slot items first_item + i (wlx_pcm_put /
 * wlx_pcm_put_frames): no host-to-device copy of audio, the VAD object's PCM buffers (device and pinned) are not touched, its stream is
 * ordered behind the slot's with ONE event, the slot counts as busy for the call. Errors as wlx_vad_probs_pcm: WLX_ERR_ARG for
 * different devices or items outside the slot, WLX_ERR_STATE for a busy slot or an item holding fewer than n_samples[i] samples.
 * device_ms_out (nullable): HIP-event time from the first to the last kernel. */
#define WLX_VAD_MAX_BATCH 64
int32_t wlx_vad_probs_batch(wlx_vad* v, const float* pcm, const int64_t* n_samples, const int32_t* extra_zero_windows, int32_t n,
                            float* probs_out, int64_t cap, int32_t* n_windows_out, float* device_ms_out);
int32_t wlx_vad_probs_pcm_batch(wlx_vad* v, wlx_engine* e, int32_t slot, int32_t first_item, const int64_t* n_samples,
                                const int32_t* extra_zero_windows, int32_t n, float* probs_out, int64_t cap,
                                int32_t* n_windows_out, float* device_ms_out);
/* Host only (no device work): the hysteresis segmentation of per-window speech probabilities into padded sample ranges —
 * faster_whisper.vad.get_speech_timestamps' loop (reference call site: transcriber_faster_whisper.py:825-852), statement for
 * statement whisperlive_amd/vad.py speech_segments_from_probs. It runs between the VAD launch and the log-mel launch, with the
 * GPU waiting. thr / neg: the thresholds rounded to float32; the durations in samples as the Python code computes them
 * (max_speech may be +inf). start_end_out: [cap][2]. */
int32_t wlx_vad_segments(const float* probs, int32_t n_windows, int64_t n_samples, double thr, double neg, double min_speech,
                         double pad, double max_speech, double min_silence, double min_silence_at_max,
                         int64_t* start_end_out, int32_t cap, int32_t* n_out);
/* log-mel of the CONCATENATION of `n_ranges` ring ranges [ranges[2 i], ranges[2 i + 1]) (absolute positions, ascending,
 * <= 256 of them) into item `item` of the slot: identical features to wlx_logmel on the concatenated samples. The launch
 * is issued at once (it reads the ring, which the socket thread may trim later). */
int32_t wlx_logmel_ring(wlx_engine* e, int32_t slot, int32_t item, wlx_ring* r, const int64_t* ranges, int32_t n_ranges,
                        int32_t* n_frames_out);

/* ---- text translation (M2M100 / small100) — PRODUCT entry points of the `enable_translation` side channel ----
 * Replaces the reference's per-client M2M100ForConditionalGeneration.generate() on torch.cuda
 * (whisper_live/backend/translation_backend.py:62-66,86-96; wired in whisper_live/server.py:203-229).
 * Weights: float32 tensors named with their Hugging Face M2M100 keys ("model.shared.weight",
 * "model.encoder.layers.{i}.self_attn.q_proj.weight", ...; the output projection is tied to model.shared), host or device
 * pointers as for wlx_engine_create. A slot owns a NON-BLOCKING stream (it takes none of the hardware queues of the ASR slots)
 * and every device buffer of a call for max_batch items of <= max_src source tokens and max_rows_per_item beams; calls on a
 * busy slot return WLX_ERR_STATE. */
typedef struct {
    int32_t d_model, n_heads, enc_layers, dec_layers, ffn, vocab;
    int32_t max_positions;       /* max_position_embeddings (1024): source length and max_length are bounded by it */
    int32_t pad_id, eos_id, decoder_start_id;
    int32_t scale_embedding;     /* embeddings scaled by sqrt(d_model) */
} wlx_mt_spec;
typedef struct wlx_mt wlx_mt;
/* Generation options = the beam-search settings of transformers' generate() (M2M100's generation_config.json). */
typedef struct {
    int32_t num_beams;             /* 1 = greedy search */
    int32_t max_length;            /* decoder tokens including the decoder start token, <= min(448, max_positions) */
    int32_t early_stopping;        /* 0 = False, 1 = True, 2 = "never" */
    float   length_penalty;
    int32_t no_repeat_ngram_size;  /* 0 = off */
    int32_t forced_eos_token_id;   /* -1 = none */
} wlx_mt_gen_opts;
int32_t wlx_mt_create(const wlx_mt_spec* spec, const wlx_tensor* weights, int32_t n_weights, int32_t device, wlx_mt** out);
void    wlx_mt_destroy(wlx_mt* mt);
int32_t wlx_mt_slot_create(wlx_mt* mt, int32_t max_batch, int32_t max_rows_per_item, int32_t max_src, int32_t* slot_out);
int32_t wlx_mt_slot_destroy(wlx_mt* mt, int32_t slot);
/* Translate `batch` sources (src_ids[i][0 .. src_lens[i]) with row stride src_stride: [tgt_lang_code] + pieces + [eos] for
 * small100). Outputs per item: the best hypothesis' generated tokens (decoder start and final EOS excluded, at most
 * tokens_stride), their count, and its score (beam search: Hugging Face's sequences_scores = sum of log-probabilities /
 * generated_length ** length_penalty; greedy: the sum of the log-probabilities). Returns when the results are final. */
int32_t wlx_mt_translate(wlx_mt* mt, int32_t slot, int32_t batch, const int32_t* src_ids, const int32_t* src_lens,
                         int32_t src_stride, const wlx_mt_gen_opts* opts, int32_t* tokens_out, int32_t tokens_stride,
                         int32_t* n_tokens_out, float* scores_out);
/* Translate a whole transcript as ONE job: `n` sources (1 <= n <= WLX_MT_MANY_MAX; n may exceed the slot's max_batch), arguments
 * and outputs as wlx_mt_translate. The call orders the sources by length (a stable order), cuts them into groups of at most
 * max_batch sources that fit the slot's source-token buffers, and runs each group as one encoder pass and one generate whose search
 * (beam search, greedy search, no_repeat_ngram bans) runs ON THE DEVICE: no table goes up and no candidate comes down per decode
 * step. The host enqueues decode steps in blocks and, after each block, waits for an event and reads a done word the search kernel
 * stored to pinned memory behind the results; steps enqueued past the end compute on scratch. Results are written in INPUT order.
 * Contract: entry i has the tokens, and the bit pattern of the score, that wlx_mt_translate gives for the sources of i's group in
 * the group's order; wherever a batched wlx_mt_translate equals its single calls (every case the tests run) that is also the
 * result of a single call on source i alone.
 * WLX_ERR_ARG, before any launch and with no output written: a null pointer, n outside 1..WLX_MT_MANY_MAX, a source of length 0
 * or longer than the slot's max_src (or src_stride), a token outside the vocabulary, options wlx_mt_translate refuses.
 * WLX_ERR_STATE, likewise: a busy slot. wlx_mt_translate itself is unchanged (host search): the live path keeps using it. */
#define WLX_MT_MANY_MAX 4096     /* sources of one wlx_mt_translate_many call: an hour of speech in segments */
int32_t wlx_mt_translate_many(wlx_mt* mt, int32_t slot, int32_t n, const int32_t* src_ids, const int32_t* src_lens,
                              int32_t src_stride, const wlx_mt_gen_opts* opts, int32_t* tokens_out, int32_t tokens_stride,
                              int32_t* n_tokens_out, float* scores_out);

/* ---- speaker embedding (WeSpeaker ResNet34) — PRODUCT entry points of the `enable_diarization` option ----
 * Replaces the pyannote.audio Inference(window="whole") call of the reference's SpeakerDiarizer._compute_embedding
 * (whisper_live/diarization.py:100-118): Kaldi filterbank (80 bins, 25 ms / 10 ms, per-bin mean over the frames removed) ->
 * ResNet (3 x 3 stem, four stages of BasicBlocks) -> statistics pooling -> Linear -> L2 normalisation, all on the device.
 * Weights: float32 tensors with BatchNorm ALREADY FOLDED into the convolutions and the values rounded to fp16
 * (whisperlive_amd/spk_weights.py fold()): "conv1.weight" [planes][1][3][3], "conv1.bias", "layer{1..4}.{b}.conv1.weight" /
 * ".conv1.bias" / ".conv2.weight" / ".conv2.bias", "layer{2..4}.0.shortcut.weight" [C][Cin][1][1] / ".shortcut.bias",
 * "seg_1.weight" [embed_dim][2 * 8 planes * n_mels / 8], "seg_1.bias". One engine per GPU: it owns a NON-BLOCKING stream and
 * every buffer of a call of up to max_seconds of audio; concurrent calls are serialised inside. */
typedef struct {
    int32_t n_mels;        /* 80; a multiple of 8 */
    int32_t planes;        /* channels of the stem and the first stage (32); stage L has planes << L */
    int32_t blocks[4];     /* BasicBlocks per stage: {3, 4, 6, 3} */
    int32_t embed_dim;     /* 256 */
    int32_t max_seconds;   /* longest segment of one call (45: the session buffer's cap) */
    float   pool_eps;      /* std = sqrt(var_unbiased + pool_eps); WeSpeaker's TSTP uses 1e-7 (UNPINNED: no checkpoint to compare) */
} wlx_spk_spec;
typedef struct wlx_spk wlx_spk;
int32_t wlx_spk_create(const wlx_spk_spec* spec, const wlx_tensor* weights, int32_t n_weights, int32_t device, wlx_spk** out);
void    wlx_spk_destroy(wlx_spk* spk);
/* L2-normalised embedding out[embed_dim] of 16 kHz mono PCM in [-1, 1]. WLX_ERR_TOO_SHORT under 4800 samples (0.3 s, where the
 * reference returns no embedding; `out` is not written), WLX_ERR_ARG over max_seconds. Returns when the result is final. The pass is
 * that of wlx_spk_embed_batch with one segment. */
int32_t wlx_spk_embed(wlx_spk* spk, const float* pcm_f32, int64_t n_samples, float* out);
/* 1 <= n <= WLX_SPK_MAX_BATCH segments in ONE pass over the network (one upload, one launch sequence, one wait):
 * pcm_f32 holds the segments back to back (host), n_samples[i] the length of each, out [n][embed_dim] one embedding per segment.
 * A row does not depend on what else is in the batch or where the segment stands in it (so it has the bits of wlx_spk_embed
 * on that segment, which is this pass with n = 1). status[i] = WLX_OK, or WLX_ERR_TOO_SHORT for a segment under 4800
 * samples: its row is zero and it takes no part in the pass (all too short: WLX_OK, nothing launched). The segments share
 * the engine's buffers: WLX_ERR_ARG, nothing launched and nothing written, when their lengths sum to more than max_seconds,
 * for n outside its range and for a null pointer. */
#define WLX_SPK_MAX_BATCH 64
int32_t wlx_spk_embed_batch(wlx_spk* spk, const float* pcm_f32, const int64_t* n_samples, int32_t n, float* out, int32_t* status);
/* wlx_spk_embed_batch on ranges of RESIDENT audio: entry i is samples [starts[i], starts[i] + n_samples[i]) of the resident PCM of
 * slot item `item` (wlx_pcm_put / wlx_pcm_put_frames). No host-to-device copy of audio; the engine's PCM buffer is not touched. The
 * ranges may touch, overlap and repeat: they are only read. out, status, WLX_ERR_TOO_SHORT and the bits of every row as above. The
 * engine's stream is ordered behind the slot's with ONE event (a wlx_pcm_put_frames resample may still be in flight); the slot counts
 * as busy for the call; one wait, at the end. Every refusal happens before any launch and writes nothing. WLX_ERR_ARG: a null
 * pointer, n outside 1..WLX_SPK_MAX_BATCH, a negative start or count, one range or the sum of all over max_seconds (the ranges share the
 * engine's activation buffers), `spk` and `e` on different devices, an item outside the slot. WLX_ERR_STATE: a busy slot, no PCM
 * resident in the item, a range ending past the resident count. */
int32_t wlx_spk_embed_pcm_batch(wlx_spk* spk, wlx_engine* e, int32_t slot, int32_t item, const int64_t* starts,
                                const int64_t* n_samples, int32_t n, float* out, int32_t* status);
/* the same on ABSOLUTE stream positions of a device PCM ring (wlx_ring_*, below). The ring's mutex is held for the call, as in
 * wlx_vad_probs_resident: an append or a trim from the socket thread waits its turn. WLX_ERR_STATE for a range that starts below the
 * ring's base (trimmed away) or ends past base + resident. */
int32_t wlx_spk_embed_ring_batch(wlx_spk* spk, wlx_ring* r, const int64_t* starts, const int64_t* n_samples, int32_t n,
                                 float* out, int32_t* status);

/* ---- offline speaker clustering: all embeddings of a file at once (the online rule of the live sessions is host code) ----
 * Average-linkage (UPGMA) agglomerative clustering of the cosine DISTANCES 1 - dot(x_i, x_j) of n unit embeddings, float32 throughout,
 * in one launch of one workgroup. The rules are exact (whisperlive_amd/file_diarization.py cluster_host restates them in NumPy float32
 * and the tests ask for equality): clusters are named by their lowest member; each round merges the pair (i, j), i < j, of live
 * clusters with the smallest (distance, i, j) in lexicographic order, j into i, and every other live k gets
 * d(k, i) = (n_i d(k, i) + n_j d(k, j)) / (n_i + n_j), each operation rounded on its own; it stops at one cluster, or when the smallest
 * distance is > threshold and (max_clusters == 0 or live clusters <= max_clusters): max_clusters forces merges past the threshold.
 * labels number the clusters 0 .. K-1 by lowest member: with windows in time order, by first appearance. */
#define WLX_SPK_CLUSTER_MAX 2048
typedef struct {
    float   threshold;     /* cosine DISTANCE at which merging stops (1 - similarity), in [0, 2] */
    int32_t max_clusters;  /* 0 = no cap */
} wlx_spk_cluster_opts;
/* host embeddings emb [n][dim] (unit rows, dim = the engine's embed_dim, 1 <= n <= WLX_SPK_CLUSTER_MAX) -> labels [n], *n_clusters = K,
 * and, when `centroids` is not null, its first K rows [dim]: the normalised mean of each cluster's members (the buffer holds up to n
 * rows; rows from K on are not written). n = 1: label 0, nothing launched. One upload, one wait. WLX_ERR_ARG, before any launch and
 * with nothing written: a null pointer, n or dim out of range, a threshold that is NaN or outside [0, 2], max_clusters < 0.
 * The first call of an engine that clusters (this one, wlx_spk_diarize_pcm or wlx_spk_diarize_many) makes the buffers all three share,
 * sized for a wave: WLX_SPK_MANY_MAX_CELLS floats of matrices and tables of WLX_SPK_MANY_MAX_ROWS rows (64 MiB + 16 MiB of HBM and
 * 16 MiB pinned at embed_dim 256). An engine that only embeds never pays for them. */
int32_t wlx_spk_cluster(wlx_spk* spk, const float* emb, int32_t n, int32_t dim, const wlx_spk_cluster_opts* opts,
                        int32_t* labels, float* centroids, int32_t* n_clusters);
/* A whole file: windows [starts[i], starts[i] + n_samples[i]) of the resident PCM of a slot item, 1 <= n <= WLX_SPK_CLUSTER_MAX. ALL of
 * them are embedded — n may exceed WLX_SPK_MAX_BATCH and their sum max_seconds: the call groups the windows that take part itself,
 * greedily in order, into ragged passes of at most WLX_SPK_MAX_BATCH windows and max_seconds of samples (a window under 4800 samples
 * counts toward neither), and enqueues the passes back to back, each writing its rows into one device table — then clustered as above,
 * with ONE wait at the end. It is wlx_spk_diarize_many of one file behind refusals of its own, plus dist_out.
 * A window under 4800 samples: status[i] = WLX_ERR_TOO_SHORT, labels[i] = -1, a zero row of emb_out; it takes no part. The m others
 * get status WLX_OK and their cluster in labels. Nullable outputs: emb_out [n][embed_dim], row i with the bits wlx_spk_embed_pcm_batch
 * gives for that range; dist_out [m][m], the matrix the device clustered, over the windows that took part in their order;
 * centroids, K rows as above (room for m). m = 1: label 0, no clustering launch; m = 0: *n_clusters = 0, nothing launched.
 * Ordering behind the slot's stream, the busy rule, the device check and WLX_ERR_STATE as in wlx_spk_embed_pcm_batch. WLX_ERR_ARG,
 * before any launch and with nothing written: a null pointer, n out of range, the options as above, a negative start or count, a
 * single window over max_seconds. */
int32_t wlx_spk_diarize_pcm(wlx_spk* spk, wlx_engine* e, int32_t slot, int32_t item, const int64_t* starts, const int64_t* n_samples,
                            int32_t n, const wlx_spk_cluster_opts* opts, int32_t* labels, int32_t* status, float* emb_out,
                            float* dist_out, float* centroids, int32_t* n_clusters);
/* A wave of files: wlx_spk_diarize_pcm of 1 <= n_files <= WLX_SPK_MANY_MAX_FILES DIFFERENT items of one slot behind ONE wait. File f is
 * item items[f] with n_windows[f] windows (0..WLX_SPK_CLUSTER_MAX) and options opts[f]; starts / n_samples / labels / status / emb_out /
 * centroids are packed file by file, file f at window w0_f = n_windows[0] + .. + n_windows[f-1] (centroids: K_f rows from row w0_f).
 * The windows that take part, of all files in file order, are grouped greedily into ragged passes of at most WLX_SPK_MAX_BATCH windows
 * and max_seconds of samples — a pass may span files — and enqueued back to back into one table; then ONE distance-matrix launch, ONE
 * clustering launch (a workgroup per file, the files side by side on as many CUs) and ONE centroid launch over the files with two or
 * more such windows, and the downloads. For every file labels, status, n_clusters[f], its rows of emb_out and its centroids are, bit
 * for bit, what wlx_spk_diarize_pcm returns for that item, those windows and those options (short windows, m = 1 and m = 0 included).
 * file_status[f] = WLX_OK, or WLX_ERR_STATE for an item without resident PCM or with a window past its resident count: that file's
 * labels are -1, its window status WLX_ERR_STATE, its rows zero, n_clusters[f] = 0, and the other files go on. The call returns
 * WLX_ERR_STATE for a busy slot, and WLX_ERR_ARG — before any launch and with nothing written — for: a null required pointer (emb_out
 * and centroids may be null), n_files out of range, a file with a negative count or more than WLX_SPK_CLUSTER_MAX windows, more than
 * WLX_SPK_MANY_MAX_ROWS windows in all, matrices (the sum of m_f^2 over the windows that take part) over WLX_SPK_MANY_MAX_CELLS
 * floats, options as above, a negative start or count, a window over max_seconds, different devices, an item outside the slot or named
 * twice. One file is the same path: wlx_spk_diarize_pcm and wlx_spk_cluster run it on a wave of one, in the same buffers. */
#define WLX_SPK_MANY_MAX_FILES 64
#define WLX_SPK_MANY_MAX_ROWS  8192          /* windows of all files together */
#define WLX_SPK_MANY_MAX_CELLS (4u * WLX_SPK_CLUSTER_MAX * WLX_SPK_CLUSTER_MAX)   /* floats of all distance matrices together */
int32_t wlx_spk_diarize_many(wlx_spk* spk, wlx_engine* e, int32_t slot, int32_t n_files, const int32_t* items,
                             const int32_t* n_windows /*[n_files]*/, const int64_t* starts, const int64_t* n_samples /* packed, file by file */,
                             const wlx_spk_cluster_opts* opts /*[n_files]*/, int32_t* labels, int32_t* status /* per window */,
                             int32_t* file_status, int32_t* n_clusters /*[n_files]*/,
                             float* emb_out, float* centroids /* nullable; packed [sum n][E] */);

/* ==== everything below: TEST / PROFILING hooks (used only by tests/, scripts/ and bench.py's roofline leg; not part of
 * the drop-in boundary; the product entry points end here) ================================================================= */
/* next-token logits [rows, vocab] of the last decoder step executed on the slot */
int32_t wlx_debug_logits_get(wlx_engine* e, int32_t slot, float* out, int32_t rows, int64_t cap_floats);
/* teacher-forced decoder pass: feed `n` tokens of one sequence (item 0), return logits [n, vocab] */
int32_t wlx_debug_decode_logits(wlx_engine* e, int32_t slot, const int32_t* tokens, int32_t n, float* out);
/* run the search kernels on caller-supplied logits (float32 [steps][rows][vocab], host):
 * exercises logits processors + beam/sampling bookkeeping without the network */
int32_t wlx_debug_search(wlx_engine* e, int32_t slot, const float* logits, int32_t steps,
                         const int32_t* prompt, int32_t prompt_len, const wlx_gen_opts* opts,
                         int32_t* tokens_out, int32_t tokens_stride, int32_t* n_tokens_out, float* scores_out);
/* the same for `batch` items in one call (wlx_debug_search is its batch of one): logits float32 [steps][batch * R][vocab], host,
 * R = beam_size in beam mode, num_hypotheses when sampling; item b's rows are [b * R, (b + 1) * R). prompts [batch][prompt_stride] as
 * wlx_generate; outputs tokens_out [batch][NH][tokens_stride], n_tokens_out / scores_out [batch][NH], NH = max(1, num_hypotheses).
 * WLX_ERR_ARG, with nothing launched and no output written: a null argument, batch < 1 or above the slot's items, steps < 1, and
 * whatever wlx_generate refuses (rows, prompt length against max_length, tokens outside the vocabulary, options). */
int32_t wlx_debug_search_batch(wlx_engine* e, int32_t slot, const float* logits, int32_t steps, int32_t batch,
                               const int32_t* prompts, const int32_t* prompt_lens, int32_t prompt_stride, const wlx_gen_opts* opts,
                               int32_t* tokens_out, int32_t tokens_stride, int32_t* n_tokens_out, float* scores_out);
/* time `iters` replays of one full decode step (rows x vocab GEMV chain) with HIP events; returns avg ms */
int32_t wlx_debug_time_decode_step(wlx_engine* e, int32_t slot, int32_t rows, int32_t t, int32_t iters,
                                   float* avg_ms_out);

/* per-kernel HIP-event profile of one decode step (eager launches bracketed by event pairs on the slot
 * stream), aggregated by kernel name; bytes_per_launch = algorithmic bytes (weights / K,V streamed once). */
typedef struct {
    char name[64];
    float launches_per_step, avg_us, total_us_per_step;
    double bytes_per_launch;
} wlx_kernel_stat;
/* In-kernel timeline of one decode step. Only libwlx_trace.so (the same sources built with -DWLX_TRACE) records;
 * the production library returns WLX_ERR_STATE. out: [n_launches][(2048 + 1) * 8] u64 (n_launches <= 320), names: [n_launches][48]. */
int32_t wlx_debug_trace_step(wlx_engine* e, int32_t slot, int32_t rows, int32_t t, int32_t with_search,
                             uint64_t* out, int64_t cap_u64, char* names, int32_t* n_launches_out);

int32_t wlx_debug_profile_step(wlx_engine* e, int32_t slot, int32_t rows, int32_t t, int32_t iters,
                               wlx_kernel_stat* out, int32_t cap, int32_t* n_out);

/* translation engine: float32 final encoder output of `batch` sources, packed item after item ([sum src_lens][d_model]) */
int32_t wlx_mt_debug_encode(wlx_mt* mt, int32_t slot, int32_t batch, const int32_t* src_ids, const int32_t* src_lens,
                            int32_t src_stride, float* out, int64_t cap_floats);
/* translation engine: teacher-forced decoder logits [n][vocab] of one source and decoder tokens dec_tokens[0 .. n) */
int32_t wlx_mt_debug_decode_logits(wlx_mt* mt, int32_t slot, const int32_t* src_ids, int32_t src_len, const int32_t* dec_tokens,
                                   int32_t n, float* out);
/* translation engine: device times (HIP events) of the slot's last wlx_mt_translate (or of the last group of its last
 * wlx_mt_translate_many): encoder pass, decode loop; decode steps (of all groups). After wlx_mt_translate_many the decode time ends
 * behind everything the host had enqueued when it saw the done word: with a block length above 1 (libwlx_ab.so, the hook) that
 * includes the group's decode steps past its end, which `steps` does not count. */
int32_t wlx_mt_debug_timings(wlx_mt* mt, int32_t slot, float* encode_ms, float* decode_ms, int32_t* steps);
/* translation engine: the search alone on caller-supplied logits (float32 [steps][batch * num_beams][vocab], host; any vocab in
 * 2..262144), no network pass: step i's logits go to the production top-k launches, then either the host bookkeeping of
 * wlx_mt_translate (use_device = 0) or the device search of wlx_mt_translate_many (use_device = 1, decode steps enqueued in blocks of
 * step_block, 0 = the library's) runs. ban_ld: the row length of the no_repeat_ngram ban table (the slots use 448). Outputs as
 * wlx_mt_translate, plus the decode steps taken. WLX_ERR_ARG before any launch: a null pointer, batch outside 1..64, ids outside
 * the vocabulary, options wlx_mt_translate refuses (num_beams <= 16), fewer steps of logits than max_length can take. */
int32_t wlx_mt_debug_search(int32_t device, const float* logits, int32_t steps, int32_t batch, const wlx_mt_gen_opts* opts,
                            int32_t vocab, int32_t pad_id, int32_t eos_id, int32_t start_id, int32_t ban_ld, int32_t step_block,
                            int32_t use_device, int32_t* tokens_out, int32_t tokens_stride, int32_t* n_tokens_out,
                            float* scores_out, int32_t* steps_run_out);
/* translation engine kernels, one launch each on host arrays (fp16 as uint16 bits), on a private stream of `device`; every
 * shape the launcher cannot serve fails with WLX_ERR_ARG before any launch.
 * Attention: groups [n_groups][4] = (q0, nq, k0, nk), head h at columns 64 h of Q / K / V / O (strides ldq / ldk / ldv / ldo);
 * 1 <= nq <= max_nq <= 16. With `anc` (rows (max q0 + 1) x ld_anc, nk <= min(ld_anc, tmax)) key j of a group is row
 * anc[q0 * ld_anc + j] * tmax + j of K / V, else row k0 + j. O is copied in and out: rows no group owns come back unchanged. */
int32_t wlx_mt_debug_attn(int32_t device, const uint16_t* q, int64_t ldq, int64_t q_rows, const uint16_t* k, int64_t ldk,
                          const uint16_t* v, int64_t ldv, int64_t kv_rows, const int32_t* groups, int32_t n_groups, int32_t max_nq,
                          int32_t heads, const int32_t* anc, int32_t ld_anc, int32_t tmax, uint16_t* o, int64_t ldo, int64_t o_rows);
/* log-softmax + top-k over float32 logits [rows][vocab] (vocab a multiple of 16, <= 262144; 1 <= k <= 32), optional bans
 * ban[r][0 .. nban[r]) (row stride ban_ld; nban may be null): out_val / out_idx [rows][k], -inf / -1 past the eligible tokens */
int32_t wlx_mt_debug_topk(int32_t device, const float* logits, int32_t rows, int32_t vocab, const int32_t* ban, const int32_t* nban,
                          int32_t ban_ld, int32_t k, float* out_val, int32_t* out_idx);
/* token embedding: E float32 [vocab][d] (d a multiple of 32) packed as the engine packs it, x[r] = scale * E[tok[r]] +
 * sinpos[pos[r]] with sinpos float32 [n_pos][d]; x float32 [rows][d] */
int32_t wlx_mt_debug_embed(int32_t device, const float* E, int32_t vocab, int32_t d, const int32_t* tok, const int32_t* pos,
                           int32_t rows, float scale, const float* sinpos, int32_t n_pos, float* x);
/* KV-cache append of a decode step: qkv fp16 [rows][ldqkv] (q | k | v thirds of d columns, d and ldqkv multiples of 8, ldqkv >= 3 d);
 * the k / v third of row r goes to slot t (0 <= t < tmax) of row r of Kc / Vc fp16 [cache_rows][tmax][d], rows <= cache_rows.
 * Kc / Vc are copied in and out: every other element comes back unchanged. */
int32_t wlx_mt_debug_kv_append(int32_t device, const uint16_t* qkv, int64_t ldqkv, int32_t rows, int32_t d, uint16_t* Kc, uint16_t* Vc,
                               int32_t cache_rows, int32_t tmax, int32_t t);
/* The in-place ReLU of the MLP: y fp16 [M][ld], columns 0 .. N of every row (N and ld multiples of 8, ld >= N); y is copied in and
 * out, the columns N .. ld come back unchanged. */
int32_t wlx_mt_debug_relu(int32_t device, uint16_t* y, int64_t ld, int32_t M, int32_t N);

/* speaker engine: device times (HIP events) of the last wlx_spk_embed, wlx_spk_embed_batch, wlx_spk_embed_pcm_batch or
 * wlx_spk_embed_ring_batch that launched: filterbank, then network + pooling + head */
int32_t wlx_spk_debug_timings(wlx_spk* spk, float* fbank_ms, float* net_ms);
/* speaker engine kernels, one launch each on host arrays, same conventions as the hooks above.
 * Filterbank of n_samples >= 400 samples: frames_out float32 [T][n_mels] (log-mel, per-bin mean removed) and image_out, its fp16
 * rounding transposed to [n_mels][T] (what the stem reads), T = 1 + (n_samples - 400) / 160 <= cap_frames. */
int32_t wlx_spk_debug_fbank(int32_t device, const float* pcm, int64_t n_samples, int32_t n_mels, float* frames_out, uint16_t* image_out,
                            int32_t cap_frames, int32_t* n_frames_out);
/* One convolution: in fp16 [H][W][Cin], w float32 [Cout][Cin][ksize][ksize] (rounded to fp16 and packed by the hook as the engine
 * does), bias float32 [Cout] or null, resid fp16 [OH][OW][Cout] or null, out fp16 [OH][OW][Cout], OH = (H - 1) / stride + 1.
 * ksize 3 (padding 1) or 1 (padding 0), stride 1 or 2. Cin = 1 runs the stem's vector-ALU kernel (ksize 3, w kept float32, Cout a
 * multiple of 4); otherwise Cin and Cout are multiples of 32 and the MFMA kernel runs. */
int32_t wlx_spk_debug_conv(int32_t device, const uint16_t* in, int32_t H, int32_t W, int32_t Cin, const float* w, const float* bias,
                           const uint16_t* resid, int32_t Cout, int32_t stride, int32_t ksize, int32_t relu, uint16_t* out);
/* Statistics pooling of x fp16 [F][T][C] over T >= 2 (C a multiple of 64): out float32 [2][C][F], mean then sqrt(var_unbiased + eps) */
int32_t wlx_spk_debug_pool(int32_t device, const uint16_t* x, int32_t F, int32_t T, int32_t C, float eps, float* out);
/* The ragged forms, one launch over n <= WLX_SPK_MAX_BATCH items packed back to back without padding. Convolution: item i is its own
 * [H][widths[i]][Cin] image in `in` and its own [OH][(widths[i] - 1) / stride + 1][Cout] image in `resid` / `out`; the rest as
 * wlx_spk_debug_conv, Cin = 1 included. Pooling: item i is [F][frames[i]][C] (frames[i] >= 2), out float32 [n][2][C][F].
 * wlx_spk_debug_conv and _pool go through the same launchers with n = 1 (for Cin >= 32 the launcher then picks a kernel without the
 * item table around the same tile code, as it does for wlx_spk_embed). */
int32_t wlx_spk_debug_conv_batch(int32_t device, const uint16_t* in, int32_t H, int32_t n, const int32_t* widths, int32_t Cin,
                                 const float* w, const float* bias, const uint16_t* resid, int32_t Cout, int32_t stride, int32_t ksize,
                                 int32_t relu, uint16_t* out);
int32_t wlx_spk_debug_pool_batch(int32_t device, const uint16_t* x, int32_t F, int32_t n, const int32_t* frames, int32_t C, float eps,
                                 float* out);
/* The ragged filterbank and mean removal, one launch each over 1 <= n <= WLX_SPK_MAX_BATCH windows of ONE buffer of n_samples samples:
 * item i is the frames[i] >= 1 frames from sample offsets[i] >= 0 on (any offset; windows may overlap and come in any order; the last
 * frame ends inside the buffer: offsets[i] + 400 + 160 (frames[i] - 1) <= n_samples). Outputs packed back to back in item order, as the
 * engine packs them: frames_out float32 [sum T][n_mels], image_out fp16 item by item [n_mels][frames[i]]. Every item has the bits of
 * wlx_spk_debug_fbank on its samples alone. */
int32_t wlx_spk_debug_fbank_batch(int32_t device, const float* pcm, int64_t n_samples, int32_t n, const int64_t* offsets,
                                  const int32_t* frames, int32_t n_mels, float* frames_out, uint16_t* image_out);
/* The embedding head: pooled float32 [n][D], W float32 [E][D] (rounded to fp16 by the hook as the engine does), b float32 [E] ->
 * emb float32 [n][E] = W pooled + b (normalize = 0) or that divided by its norm, an all-zero row staying zero (normalize = 1).
 * D a multiple of 8 (the kernel's 8-wide loads), D and E up to 2^16, n up to 65535. */
int32_t wlx_spk_debug_head(int32_t device, const float* pooled, const float* W, const float* b, int32_t n, int32_t D, int32_t E,
                           int32_t normalize, float* emb);
/* The clustering kernels, one launch each. Affinity: X float32 [n][dim] (1 <= n <= WLX_SPK_CLUSTER_MAX, 1 <= dim <= 1024) ->
 * dist_out [n][n] = 1 - X X^T, exactly symmetric, diagonal exactly 0. */
int32_t wlx_spk_debug_affinity(int32_t device, const float* X, int32_t n, int32_t dim, float* dist_out);
/* Clustering of a given symmetric matrix dist [n][n] (not written): labels [n], merges [n - 1][2] as (i, j), heights [n - 1],
 * *n_merges, *n_clusters; rows of merges / heights from *n_merges on come back unchanged. */
int32_t wlx_spk_debug_ahc(int32_t device, const float* dist, int32_t n, const wlx_spk_cluster_opts* opts, int32_t* labels,
                          int32_t* merges, float* heights, int32_t* n_merges, int32_t* n_clusters);
/* The many-forms of the two, one launch each over 1 <= n_files <= WLX_SPK_MANY_MAX_FILES files packed back to back: file f has ns[f]
 * rows (1..WLX_SPK_CLUSTER_MAX; all together at most WLX_SPK_MANY_MAX_ROWS, their matrices at most WLX_SPK_MANY_MAX_CELLS floats) at
 * row0_f = ns[0] + .. + ns[f-1] of X / labels / heights, its matrix [ns[f]][ns[f]] at ns[0]^2 + .. + ns[f-1]^2 of dist, its merges at
 * 2 * row0_f of merges (room for ns[f] pairs, ns[f] - 1 at the most written). opts, n_merges, n_clusters: one entry per file. Every
 * file's results have the bits of wlx_spk_debug_affinity / wlx_spk_debug_ahc on that file alone: those two are these launches over
 * one file. */
int32_t wlx_spk_debug_affinity_many(int32_t device, const float* X, int32_t n_files, const int32_t* ns, int32_t dim, float* dist_out);
int32_t wlx_spk_debug_ahc_many(int32_t device, const float* dist, int32_t n_files, const int32_t* ns, const wlx_spk_cluster_opts* opts,
                               int32_t* labels, int32_t* merges, float* heights, int32_t* n_merges, int32_t* n_clusters);
/* device times (HIP events) of the last wlx_spk_cluster, wlx_spk_diarize_pcm or wlx_spk_diarize_many that clustered: the distance
 * matrix launch, the clustering launch (of a many-call: its ONE launch of each, over all its files) */
int32_t wlx_spk_debug_cluster_timings(wlx_spk* spk, float* affinity_ms, float* ahc_ms);

/* Whisper kernels, one launch each (csrc/kernel_hooks.hip), same conventions: host arrays (fp16 as uint16 bits), a private stream
 * of `device`, outputs copied in AND out (bytes no thread owns come back unchanged), WLX_ERR_ARG before any launch for every
 * shape the launcher cannot serve.
 * LayerNorm of x float32 [M][ldx] over d columns (a multiple of 4, <= 2048; strides multiples of 4): out16 fp16 [M][ldo] and,
 * when out32 is not null, the float32 copy [M][ldo] (launch_layernorm_f16_f32, else launch_layernorm_f16). */
int32_t wlx_debug_layernorm(int32_t device, const float* x, int64_t ldx, const float* gamma, const float* beta, int32_t M, int32_t d,
                            uint16_t* out16, float* out32, int64_t ldo);
/* encoder self-attention (launch_attn_encoder): per item Q [T][ldq], K [T][ldk] (q pre-scaled), V^T [H * 64][ldvt] with
 * ldvt >= T rounded up to 32, O [T][ldo]; item strides isq / isk / isv / iso in halfs. 65 <= T (three 32-key tiles in flight);
 * Q / K / V^T strides multiples of 8. items * T >= 4000 runs the eight-wave kernel, else the four-wave one. */
int32_t wlx_debug_attn_encoder(int32_t device, const uint16_t* q, int64_t ldq, int64_t isq, const uint16_t* k, int64_t ldk, int64_t isk,
                               const uint16_t* vt, int64_t ldvt, int64_t isv, uint16_t* o, int64_t ldo, int64_t iso, int32_t T,
                               int32_t H, int32_t items);
/* One encoder GEMM launch (gemm.hip): A fp16 [zbatch][M][lda] (free lda / strideA: the conv-as-GEMM rows overlap), W float32 [N][K]
 * (conv3_cin != 0: a conv weight [N][Cin][3], K = 3 Cin) packed by the hook with the production pack kernels into KT k-tiles (even,
 * KT * 32 >= K), bias [N] (nullable), pos [M][N] (mode 2). mode = GemmMode 0..5 (store fp16, GELU fp16, GELU + pos fp32, residual fp32,
 * QKV, tile-packed cross K / V). force_form -1: launch_gemm's own pick; 0 / 1 / 2: the second form's 64 x 96, 96 x 96, 128 x 128 tile;
 * 3: the large-M form. *_len: halfs / floats of the caller's arrays, all copied in and out. ran_out[4] = form, LDS-transposed
 * epilogue (0 / 1), XCD remap a, b (0, 0 = off). */
typedef struct {
    int32_t zbatch, M, N, K, KT, conv3_cin, mode, force_form;
    int32_t d, rows_per_item;
    float qscale;
    int32_t reserved;
    int64_t lda, strideA, a_len;
    int64_t ldc, strideC, c_len;
    int64_t ldx, strideX, x_len;
    int64_t ldk, kv_item_stride_k, kv_layer_stride_k, k_len;
    int64_t ldvt, kv_item_stride_v, kv_layer_stride_v, v_len;
} wlx_debug_gemm_args;
int32_t wlx_debug_gemm(int32_t device, const wlx_debug_gemm_args* a, const uint16_t* A, const float* W, const float* bias,
                       const float* pos, uint16_t* C, float* X, uint16_t* kout, uint16_t* vt, int32_t* ran_out);
/* decode cross-attention: launch_dec_cross_attn then launch_dec_xattn_combine. q [rows][ldq]; kp / vp: tile-packed cross K / V of
 * ONE layer ([n_items][item_stride], the layout of the GEMM_CROSS_KV epilogue: 1536 padded keys); groups of R <= 16 rows, group g
 * attends to item group_item[g]; (groups - 1) * R < rows <= groups * R. Returns the split partials part_o fp16
 * [groups][H][8][16][64], part_ml float32 [groups][H][16][8][2] and the combined rows out fp16 [rows][ldo]. With align_out (float32
 * [rows][1536]) also launch_dec_align_scores of head align_head on item align_item's packed K. */
int32_t wlx_debug_dec_cross_attn(int32_t device, const uint16_t* q, int64_t ldq, const uint16_t* kp, const uint16_t* vp,
                                 int64_t item_stride, int32_t n_items, int32_t H, int32_t R, int32_t groups, int32_t rows,
                                 const int32_t* group_item, uint16_t* part_o, float* part_ml, uint16_t* out, int64_t ldo,
                                 int32_t align_item, int32_t align_head, float* align_out);
/* One launch_dec_gemv (csrc/dec_gemv.hip, dec_vocab.hip) on a GemvParams built as engine_decode.hip decoder_pass builds it, done = null.
 * in_mode / out_mode / xsrc: GemvIn / GemvOut / GemvXsrc of csrc/decoder.h. W float32 [N][K], packed by the hook into KT = K / 32
 * k-tiles; bias [N] or null (null: fp32 rows out only — the vocabulary projection). Inputs by mode: X float32 [M][ldx] (LayerNorm
 * prologue, with gamma / beta [K]); Xh fp16 [M][ldxh]; part_o fp16 [ceil(M / R)][H][8][16][64] and part_ml float32
 * [ceil(M / R)][H][16][8][2] (split combine, K = 64 H); slab float32 [2][rows][ld] at slab_stride floats, ld = ldx under a LayerNorm
 * prologue and ldxres otherwise (read with xsrc = SLABS, written by GEMV_OUT_SLAB, KTS = KT / 2 k-tiles per slice); tok_emb fp16
 * [tokens][K], pos_emb float32 [positions][K], emb_token / row_pos / row_cache int32 [M] (xsrc = EMBED and GEMV_OUT_QKV).
 * Outputs, copied in AND out: Yh fp16 [M][ldyh] (N columns, d for QKV); Y float32 [M][ldy]; Xres float32 [M][ldxres] (read and
 * written); Kc / Vc fp16 [cache rows][cache_row_stride], row r at row_cache[r], position row_pos[r] * d; slab; X and intok int32
 * [cache rows][448] (xsrc = EMBED: the gathered rows and the fed tokens). *_len: elements of the caller's arrays. name_out: the
 * kernel launch_dec_gemv runs for these parameters (dec_gemv_kernel_name).
 * WLX_ERR_ARG before any launch: M outside 1..320; K != 32 KT; a LayerNorm prologue with K > 1536; ldx / ldy / ldxres /
 * slab_stride / cache_row_stride / ldyh not multiples of 4 or ldxh not a multiple of 8 (the kernels' 16- and 8-byte pieces); a stride
 * below its row; a length that does not hold what is addressed; a bias missing or N not a multiple of 16 where the epilogue is not
 * fp32 rows out; fp32 rows out WITH a bias and N > 8192; QKV with N != 3 d; a position outside 0..447 or a cache row outside
 * 0..32767; R outside 1..16 or K != 64 H in the split combine; xsrc != PLAIN or GEMV_OUT_SLAB where no lean kernel serves the
 * parameters (dec_gemv_is_lean: the first-generation kernel knows neither). */
typedef struct {
    int32_t in_mode, out_mode, xsrc, M, K, KT, N, busy_device, KTS, H, R, d;
    float qscale;
    int32_t reserved;
    int64_t ldx, ldxh, ldyh, ldy, ldxres, cache_row_stride, slab_stride;
    int64_t x_len, xh_len, part_o_len, part_ml_len, slab_len, tok_emb_len, pos_emb_len, yh_len, y_len, xres_len, kc_len, vc_len, intok_len;
} wlx_debug_dec_gemv_args;
int32_t wlx_debug_dec_gemv(int32_t device, const wlx_debug_dec_gemv_args* a, const float* W, const float* bias, const float* gamma,
                           const float* beta, float* X, const uint16_t* Xh, const uint16_t* part_o, const float* part_ml, float* slab,
                           const uint16_t* tok_emb, const float* pos_emb, const int32_t* emb_token, const int32_t* row_pos,
                           const int32_t* row_cache, uint16_t* Yh, float* Y, float* Xres, uint16_t* Kc, uint16_t* Vc, int32_t* intok,
                           char* name_out, int32_t name_cap);
/* One launch_dec_cq_cross_attn (csrc/decoder.hip): LayerNorm of x float32 [rows][ldx] + query projection (Wq float32 [d][d], packed by
 * the hook; bias [d]; scaled by qscale) + the split partials of the cross attention; kp / vp / item_stride / group_item / part_o /
 * part_ml as wlx_debug_dec_cross_attn (query lanes past a group's live rows compute the group's LAST live row again).
 * WLX_ERR_ARG unless dec_cq_cross_attn_eligible(d, H, R) (d = 768, H = 12, R in 1..16), (groups - 1) * R < rows <= groups * R, ldx a
 * multiple of 4 covering d, item_stride a multiple of 8 covering the packed image, every group_item inside 0..n_items - 1. */
int32_t wlx_debug_dec_cq_cross_attn(int32_t device, const float* x, int64_t ldx, const float* gamma, const float* beta, const float* Wq,
                                    const float* bias, float qscale, int32_t d, const uint16_t* kp, const uint16_t* vp,
                                    int64_t item_stride, int32_t n_items, int32_t H, int32_t R, int32_t groups, int32_t rows,
                                    const int32_t* group_item, uint16_t* part_o, float* part_ml);
/* decode self-attention over the KV cache (launch_dec_self_attn): q [rows][ldq], kc / vc [cache_rows][cache_row_stride] with
 * position p of a cache row at p * d (cache_row_stride covers at least the positions in use), row r attends to positions 0..pos[r], position p read from cache row
 * anc[ancrow[r]][p] (anc int16 [cache_rows][448]). ident_ancestry = 1 requires ancrow[r] == r (rows <= 16: the eight-wave
 * kernel, else four waves); 0 runs the table-lookup form. out fp16 [rows][ldo]. */
int32_t wlx_debug_dec_self_attn(int32_t device, const uint16_t* q, int64_t ldq, const uint16_t* kc, const uint16_t* vc,
                                int64_t cache_row_stride, int32_t cache_rows, int32_t d, int32_t H, int32_t rows, const int32_t* pos,
                                const int32_t* ancrow, const int16_t* anc, int32_t ident_ancestry, uint16_t* out, int64_t ldo);

/* The audio front end's kernel (csrc/resample.hip), same conventions: host arrays, a private stream of `device`, `out` (cap floats)
 * copied in AND out so floats past *n_out come back unchanged. ONE copy and ONE launch per block of block_frames input frames
 * (0: the product default, 8 MB of file bytes); a block's outputs read its own frames only, so block_frames moves the seams.
 * WLX_ERR_ARG before any launch: channels outside 1..WLX_PCM_MAX_CHANNELS, sample_rate <= 0, n_frames < 0, an unknown format, a
 * ratio the kernel does not serve (wlx_pcm_put_frames RATES), n_frames > 2^50, block_frames below the filter's reach of ceil(2 * half_len / up) + 2 frames,
 * cap < ceil(n_frames * up / down). */
int32_t wlx_debug_resample(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                           int32_t sample_rate, int64_t block_frames, float* out, int64_t cap, int64_t* n_out);
/* The channel-split instantiation (wlx_pcm_put_frames_split): same arguments and refusals, `out` is [channels][cap] floats, copied in
 * AND out like the above, and channel c lands in row c (*n_out floats of it; every other float comes back unchanged). */
int32_t wlx_debug_resample_split(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                                 int32_t sample_rate, int64_t block_frames, float* out, int64_t cap, int64_t* n_out);
/* The same, and the summed HIP-event time of the block launches (scripts/resample_time.py). */
int32_t wlx_debug_resample_timed(int32_t device, const void* frames, int64_t n_frames, int32_t channels, int32_t sample_format,
                                 int32_t sample_rate, int64_t block_frames, float* out, int64_t cap, int64_t* n_out,
                                 float* kernel_ms_out);

/* The stream form of the same kernel (wlx_ring_append_frames) without an engine: a fresh stream state is fed the packets [0, cuts[0]),
 * [cuts[0], cuts[1]), ... [cuts[n_cuts - 1], n_frames) — n_cuts + 1 calls; cuts ascending, repeated values give empty packets — each
 * call waited for as the product call is. flush = 0: no flush; 1: one more call, an empty flushing packet; 2: the LAST packet carries the
 * flush (data and flush in the same call). All five sample formats. `out` (cap floats) is copied in AND out; *n_out = outputs emitted;
 * per_call_counts (nullable): n_cuts + 1 entries, one more when flush == 1. WLX_ERR_ARG before any launch: what wlx_ring_set_format
 * refuses, cuts out of order or past n_frames, cap below the total the planner gives. */
int32_t wlx_debug_resample_stream(int32_t device, const void* frames, int64_t n_frames, int32_t channels,
                                  int32_t sample_format, int32_t sample_rate,
                                  const int64_t* cuts, int32_t n_cuts, int32_t flush,
                                  float* out, int64_t cap, int64_t* n_out, int64_t* per_call_counts);

/* The FLAC frame decoder and the finish kernel (csrc/flac.hip, csrc/flac_core.h) without the resampler, on a private stream of `device`:
 * the stream's decoded INTEGER samples, interleaved [n][channels], nothing scaled or resampled; *n_frames_out = n (samples per
 * channel), cap_samples = the int32 values samples_out holds (>= n * channels). Any rate; <= 24 bits, <= 8 channels. The index runs
 * first: WLX_ERR_DATA / WLX_ERR_ARG as wlx_flac_probe before any launch; WLX_ERR_DATA after the one wait for a frame that does not decode. */
int32_t wlx_debug_flac_decode(int32_t device, const void* bytes, int64_t n_bytes, int32_t* samples_out, int64_t cap_samples,
                              int64_t* n_frames_out, int32_t* channels_out);
/* The ragged kernels of wlx_pcm_put_many (csrc/put_many.hip), ONE launch each on a private stream of `device`, n <= WLX_PUT_MANY_MAX entries.
 * wlx_debug_resample_many: resample_many_kernel over n entries of their own shapes (frames[k]: [n_frames[k]][channels[k]] in
 * sample_formats[k], any of the five WLX_PCM_* codes, at sample_rates[k]); entry k's outputs land at out[out_off[k] ..), n_out[k] of
 * them; `out` (cap floats) is copied in AND out. Entry k is BIT-IDENTICAL to wlx_debug_resample / wlx_debug_resample_stream of that entry
 * alone. WLX_ERR_ARG before any launch: what wlx_ring_set_format refuses, n_frames outside 0..2^31, an output outside the buffer.
 * wlx_debug_flac_decode_many: flac_frames_many_kernel + flac_finish_many_kernel over the concatenated frame tables of n FLAC files; entry
 * k's decoded INTEGER samples land at samples_out[out_off[k] ..) as wlx_debug_flac_decode leaves them, status_out[k] = WLX_OK, or
 * WLX_ERR_DATA for an entry with a frame that does not decode (its frame's samples are zeros). The index of every entry runs first:
 * WLX_ERR_DATA / WLX_ERR_ARG as wlx_debug_flac_decode, for the call, before any launch.
 * wlx_debug_put_many_budget: the scratch budget of wlx_pcm_put_many in this process from now on (bytes >= 64 KB; 0: unchanged; < 0: the
 * default); *previous (nullable) = the budget before, *last_sub_batches (nullable) = the sub-batches the last call ran as. */
int32_t wlx_debug_resample_many(int32_t device, int32_t n, const void* const* frames, const int64_t* n_frames, const int32_t* channels,
                                const int32_t* sample_formats, const int32_t* sample_rates, float* out, const int64_t* out_off,
                                int64_t cap, int64_t* n_out);
int32_t wlx_debug_flac_decode_many(int32_t device, int32_t n, const void* const* bytes, const int64_t* n_bytes, int32_t* samples_out,
                                   const int64_t* out_off, int64_t cap_samples, int64_t* n_frames_out, int32_t* channels_out,
                                   int32_t* status_out);
int32_t wlx_debug_put_many_budget(int64_t bytes, int64_t* previous, int32_t* last_sub_batches);
/* The ADPCM block decoder (csrc/adpcm.hip adpcm_decode_kernel, csrc/adpcm_core.h) without the resampler, on a private stream of `device`:
 * the bytes of an IMA or MS ADPCM WAV file -> samples_out[n][channels], the decoded int16 values, one upload, one launch, one wait; any
 * sample rate. WLX_ERR_DATA as wlx_wav_probe; WLX_ERR_ARG for another tag, a layout the decoder does not take, or cap_samples < n * channels. */
int32_t wlx_debug_adpcm_decode(int32_t device, const void* bytes, int64_t n_bytes, int16_t* samples_out, int64_t cap_samples,
                               int64_t* n_frames_out, int32_t* channels_out);
/* The last completed wlx_pcm_put_flac of the slot (scripts/flac_time.py): ms_out[5] = host index + CRC time (wall), then the HIP-event
 * times of the upload (the host's copies into the pinned blocks included), flac_frames_kernel, flac_finish_kernel and the resample launch. */
int32_t wlx_debug_flac_timings(wlx_engine* e, int32_t slot, float* ms_out);

/* Word alignment's post-processing kernels (csrc/align.hip), same conventions; n <= WLX_ALIGN_MAX_BATCH entries packed back to back, outputs
 * copied in AND out. wlx_debug_dtw: the DTW kernel alone on caller matrices x [N[e]][M[e]] float32 (1 <= N <= 448, 1 <= M <= 1500,
 * path_stride >= N + M); path rows at e * path_stride, n_path[e] steps. wlx_debug_align_post: the whole sequence on caller scores
 * [n_heads][n_tok[e]][1536] per entry (the layout of dec_align_scores_kernel; frames past nf[e] are not read): cost_out is the DTW cost
 * matrix packed [n_tok[e] - 1 - n_sot][nf[e]], the path is the DTW of exactly that matrix. WLX_ERR_ARG before any launch: n outside
 * 0..64, a width that is even or outside 1..15, nf outside 1..1500, n_tok outside n_sot + 3 .. 448, path_stride below N + nf. */
int32_t wlx_debug_dtw(int32_t device, const float* x, int32_t n, const int32_t* N, const int32_t* M, int32_t* text_indices,
                      int32_t* time_indices, int32_t path_stride, int32_t* n_path);
int32_t wlx_debug_align_post(int32_t device, const float* scores, int32_t n, int32_t n_heads, const int32_t* n_tok, int32_t n_sot,
                             const int32_t* nf, int32_t median_filter_width, float* cost_out, int32_t* text_indices,
                             int32_t* time_indices, int32_t path_stride, int32_t* n_path);
/* HIP-event times of the slot's last wlx_align_batch: the decoder passes with their score capture, and everything behind them. */
int32_t wlx_debug_align_timings(wlx_engine* e, int32_t slot, float* pass_ms, float* post_ms);

/* ONE launch of the keyword-boosting kernel (csrc/dec_bias.hip dec_bias_kernel), same conventions, no engine: a table as wlx_bias_set
 * takes it (checked the same way against `vocab`), `rows` decoder rows of ONE item in beam mode (1..320), logits [rows][ldl] float32
 * copied in AND out (ldl >= vocab). Row r is fed tokens[r] at position pos[r] (0..447) of a prompt of plen tokens (1..448); the row
 * that held its hypothesis at pos[r] - 1 is parent[r], whose node there is prev_state[r] (rows that name the same parent at the same
 * position must agree; not read where pos[r] < plen; a row whose parent sits at pos[r] - 1 in this very launch is refused). nsp_row[r] = 1: the row is left as it is. state_out[r]: the row's node. */
int32_t wlx_debug_bias_apply(int32_t device, int32_t vocab, int32_t eot, int32_t n_nodes, const int32_t* edge_off, const int32_t* edge_tok,
                             const int32_t* edge_next, float boost, int32_t n_tok, const int32_t* tok_ids, const float* tok_vals,
                             float* logits, int32_t rows, int64_t ldl, const int32_t* tokens, const int32_t* pos, const int32_t* parent,
                             int32_t plen, const int32_t* nsp_row, const int16_t* prev_state, int16_t* state_out);

/* The probability kernels of search.hip and the data-movement kernels of the decoder pass, ONE launch each of the launcher the engine
 * calls, same conventions (host arrays, a private stream of `device`, outputs copied in AND out, WLX_ERR_ARG before any launch with
 * the outputs untouched: a null pointer and every limit named below).
 * No call may ask for more than 2^28 elements in any one array: rows * ldl for the logits; vocab * d and rows * d; feats_len, ld, item_stride
 * and items * featT_stride; cap. The outputs `out` and `probs` hold WLX_DEBUG_GUARD words MORE than the kernel owns (rows + 64, rows * n + 64),
 * copied in and out with the rest: a store past the last row shows in them.
 * All three softmax forms compute exp(l_t - max) / sum exp(l_i - max) in float32 over the admitted ids of row r of
 * logits [rows][ldl] (ldl >= the columns read; columns past them are never read). A logit of -inf contributes exactly 0 and a
 * target at -inf gives exactly 0. A row whose EVERY admitted logit is -inf is outside the contract (max = -inf, 0 / 0): the engine
 * never produces one (the raw logits of the vocabulary projection are finite) and the hooks do not look for it.
 * wlx_debug_token_prob (token_prob_kernel, no_speech_prob of a prefill): out[r] = softmax over ids [0, V) at id tok, the same id for
 *   every row. 1 <= rows <= 65535, 1 <= V <= 2^20, ldl >= V, 0 <= tok < V.
 * wlx_debug_token_prob_rows (token_prob_rows_kernel, text_token_probs of wlx_align / wlx_align_batch): out[r] = softmax over ids
 *   [0, vlim) at id toks[r]; a target outside [0, vlim) gives exactly 0 (ids from vlim on — end-of-text and above — are no text).
 *   1 <= rows <= 65535, 1 <= vlim <= 2^20, ldl >= vlim; toks[r] is any int32.
 * wlx_debug_lang_probs (lang_probs_kernel, wlx_detect_language): probs[r][i] = softmax over the n ids `ids` at ids[i], probs
 *   [rows][n]. 1 <= rows <= 65535, 1 <= n <= WLX_LANG_MAX (the slot's id table; wlx_detect_language has the same limit),
 *   0 <= ids[i] < ldl. Ids may repeat and come in any order; a repeated id counts once per mention in the denominator. */
#define WLX_LANG_MAX 256
#define WLX_DEBUG_GUARD 64
int32_t wlx_debug_token_prob(int32_t device, const float* logits, int64_t ldl, int32_t V, int32_t rows, int32_t tok, float* out);
int32_t wlx_debug_token_prob_rows(int32_t device, const float* logits, int64_t ldl, int32_t vlim, int32_t rows, const int32_t* toks,
                                  float* out);
int32_t wlx_debug_lang_probs(int32_t device, const float* logits, int64_t ldl, int32_t rows, const int32_t* ids, int32_t n,
                             float* probs);
/* launch_dec_embed (dec_embed_kernel): x[r][0 .. d) = float(tok_emb[tokens[r]][.]) + pos_emb[pos[r]][.] in float32 (one rounding), with
 * tok_emb fp16 [vocab][d] and pos_emb float32 [n_pos][d]; the kernel also notes the token a cache row is fed: the hook gives row r the
 * cache row r, intok [rows][448] int32 (copied in AND out) gets intok[r][pos[r]] = tokens[r] and nothing else. d a multiple of 4 in
 * 4..8192 (8-byte loads of the fp16 row), 1 <= vocab <= 2^20, 1 <= n_pos <= 448, 1 <= rows <= 65535, 0 <= tokens[r] < vocab,
 * 0 <= pos[r] < n_pos. Tokens may repeat. */
int32_t wlx_debug_dec_embed(int32_t device, const uint16_t* tok_emb, int32_t vocab, const float* pos_emb, int32_t n_pos, int32_t d,
                            const int32_t* tokens, const int32_t* pos, int32_t rows, float* x, int32_t* intok);
/* launch_prep_windows (prep_window_kernel): item i reads feats + i * item_stride as [n_mels][ld] float32 and writes its window
 * featT + i * featT_stride as fp16 rows of n_mels: row 1 + t = frame seek[i] + t for t < seg[i], zeros for seg[i] <= t < 3000; rows 0
 * and 3001 (the convolution's padding) and everything behind row 3001 are not written. 1 <= n_mels <= 128 (the kernel's LDS tile),
 * 1 <= items <= 64 (the by-value window table), seek[i] >= 0, 0 <= seg[i] <= 3000, seek[i] + seg[i] <= ld, item_stride >= 0 with
 * feats_len >= (items - 1) * item_stride + (n_mels - 1) * ld + max(seek + seg), featT_stride >= 3002 * n_mels;
 * featT holds items * featT_stride halfs. */
int32_t wlx_debug_prep_windows(int32_t device, const float* feats, int64_t feats_len, int64_t ld, int32_t n_mels, int64_t item_stride,
                               int32_t items, const int32_t* seek, const int32_t* seg, uint16_t* featT, int64_t featT_stride);
/* launch_f32_to_f16 (f32_to_f16_kernel, the token embedding's table at engine creation): dst[i] = fp16(src[i]), round to nearest
 * even, values past the fp16 range to +-inf, NaN to NaN. dst holds cap >= n halfs (copied in AND out). 1 <= n <= cap <= 2^28. */
int32_t wlx_debug_f32_to_f16(int32_t device, const float* src, int64_t n, uint16_t* dst, int64_t cap);

/* The three kernels of the Silero VAD pass (vad.hip), ONE launch each of the launch function the pass itself calls, on the object's
 * stream under its mutex and with the weights as wlx_vad_create repacked them. Host arrays; the output holds cap_windows rows and
 * WLX_DEBUG_GUARD words behind them, copied in AND out: words no thread owns come back unchanged. The packed-window geometry is that of
 * wlx_vad_probs_batch (item i owns windows [sum T_0..i-1, + T_i), items without a window take none). WLX_ERR_ARG before any launch, with
 * the output untouched: a null pointer (extra_zero_windows may be null: no extras), n outside 1..WLX_VAD_MAX_BATCH, a negative count,
 * an extra outside 0..4, cap_windows outside 1..2^19, sum T_i > cap_windows. A call whose items have no window launches nothing.
 * wlx_vad_debug_frontend (vad_frontend_batch_kernel): pcm as wlx_vad_probs_batch takes it -> gx [cap_windows][512], row w the input half
 *   of the LSTM gates of window w: W_ih f + b_ih + b_hh, gate order i, f, g, o.
 * wlx_vad_debug_lstm (vad_lstm_batch_kernel): gx [sum T_i][512] as above, item i of T[i] windows from zero state -> hs [cap_windows][512],
 *   row w = [unit j][4 identical copies of h_j].
 * wlx_vad_debug_out (vad_out_kernel): hs [T][512] -> probs [cap_windows]: sigmoid(out_w . relu(copy 0 of every unit) + out_b). */
int32_t wlx_vad_debug_frontend(wlx_vad* v, const float* pcm, const int64_t* n_samples, const int32_t* extra_zero_windows, int32_t n,
                               float* gx, int64_t cap_windows);
int32_t wlx_vad_debug_lstm(wlx_vad* v, const float* gx, const int32_t* T, int32_t n, float* hs, int64_t cap_windows);
int32_t wlx_vad_debug_out(wlx_vad* v, const float* hs, int32_t T, float* probs, int64_t cap_windows);

#include "wlx_bias_items.h"
#include "wlx_grammar.h"

#ifdef __cplusplus
}
#endif
#endif /* WLX_H */
