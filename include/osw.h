/*
 * osw.h — C ABI of libosw_hip.so, the MI355X (gfx950) Whisper transcription engine.
 *
 * This library is the drop-in for the arithmetic the reference delegates to
 * faster-whisper 1.2.1 / CTranslate2.  Each entry point names the reference
 * interface it replaces (paths under the reference repository):
 *
 *   osw_create / osw_set_weight / osw_set_weight_quant / osw_init_weight_uniform / osw_finalize
 *       replace   WhisperModel(model_id, device, compute_type, download_root)
 *                 called at src/backends/faster_whisper.py:40-45 (load_model :29-50)
 *   osw_destroy
 *       replaces  del self._models[model_id]; gc; empty_cache   (unload_model :52-65)
 *   osw_transcribe_batch
 *       replaces  WhisperModel.transcribe(path, task, beam_size, temperature,
 *                 language, initial_prompt) + list(segments)     (:235-246),
 *                 for the first 30 s window of every clip; greedy, beam search
 *                 (beam_size > 1, the reference's default 5) or sampling
 *                 (temperature > 0, best_of rows), chosen per call by osw_decode_opts
 *   osw_log_mel / osw_encode_windows / osw_decode_windows
 *       the same work split by stage, as faster-whisper's generate_segments seek
 *       loop needs it (FeatureExtractor -> encode -> generate per 30 s window)
 *   osw_get_mel / osw_get_encoder_output / osw_encoder_layer_debug
 *       stage-level read-back used only by the parity tests
 *   osw_ingest_mean_square + osw_ingest_apply_gain
 *       replace   preprocess_stt_audio / normalize_gain (src/audio/preprocessing.py:35-63),
 *                 called at src/main.py:296-300; bit-identical output bytes
 *   osw_ingest_resample
 *       replaces  resample_pcm16 (src/streaming.py:55-91; scipy resample_poly,
 *                 padtype "line"), called at src/streaming.py:293-294; bit-identical
 *
 *   osw_set_alignment_heads / osw_align_windows
 *       replace   WhisperModel.transcribe(..., word_timestamps=True)'s alignment step:
 *                 faster-whisper's find_alignment -> ctranslate2 Whisper.align(encoder_output,
 *                 sot_sequence, text_tokens, num_frames, median_filter_width=7) [upstream],
 *                 i.e. openai-whisper timing.find_alignment; the reference itself calls
 *                 transcribe without it (src/backends/faster_whisper.py:235-246)
 *   osw_get_alignment_matrix / osw_debug_dtw
 *       stage-level read-back and the DTW kernel alone, used only by the parity tests
 *   osw_debug_align_post / osw_debug_align_tail / osw_debug_align_self_attn / osw_debug_align_scores
 *       one launch of the alignment pass's other kernels on host data, used only by the parity tests
 *   osw_debug_enc_attn / osw_debug_dec_xattn / osw_debug_dec_self_attn
 *       one attention launch on host data, used only by the parity tests
 *   osw_debug_dec_gemm / osw_debug_dec_gemm_quant / osw_debug_dec_resln / osw_debug_dec_gelu
 *       one launch of the decoder's hi/lo GEMMs, residual+LayerNorm and GELU reduce on host
 *       data, used only by the parity tests
 *   osw_debug_enc_gemm / osw_debug_enc_layernorm
 *       one launch of the encoder's tiled GEMM (any epilogue, grouped rows, head-major scatter)
 *       and of its LayerNorm on host data, used only by the parity tests
 *   osw_debug_get_logmel / osw_debug_mel_windows
 *       the front end's raw log10 mel with its clip maximum, and the window-packing kernel
 *       alone (the conv stem's fp16 operand), used only by the parity tests
 *   osw_decode_opts::repetition_penalty / no_repeat_ngram_size (+ osw_debug_history_rules)
 *       replace   WhisperModel.transcribe(..., repetition_penalty=, no_repeat_ngram_size=):
 *                 ctranslate2's RepetitionPenalty / NoRepeatNgram logits processors [upstream],
 *                 run per decoder row and step on the GPU; the reference itself passes neither
 *                 (src/backends/faster_whisper.py:235-246)
 *   osw_set_confidences / osw_get_token_logprobs / osw_get_language_probs / osw_detect_language
 *       replace   the per-token log-probabilities a CTranslate2 WhisperGenerationResult can
 *                 return (return_scores / return_logits_vocab) [upstream], TranscriptionInfo's
 *                 language_probability / all_language_probs and WhisperModel.detect_language()
 *                 -> ctranslate2 Whisper.detect_language(encoder_output) [upstream]; the reference
 *                 reads none of them and hard-codes its confidences (src/streaming.py:407,419)
 *   osw_decode_window_list (+ osw_debug_dec_xattn_windows)
 *       replaces  the re-decode inside faster-whisper's generate_with_fallback [upstream]: a
 *                 window that failed its compression-ratio or log-probability test is generated
 *                 again at the next temperature from the encoder output it already has; the
 *                 reference passes one scalar temperature (src/backends/faster_whisper.py:238)
 *   osw_decode_opts::task_token < 0, osw_align_window::language < 0 && task < 0
 *       replace   WhisperModel(model_id) for the English-only checkpoints of the reference's
 *                 registry (src/model_registry.py:7-21: tiny.en, base.en, small.en, medium.en,
 *                 faster-distil-whisper-small.en / -medium.en, n_vocab 51864): faster-whisper's
 *                 Tokenizer(multilingual=False) [upstream], whose sot_sequence is
 *                 (<|startoftranscript|>,) with no language and no task token, in generate,
 *                 detect_language (answered "en" by the caller) and find_alignment
 *
 * Conventions: every call returns 0 (OSW_OK) or a negative code; the message of
 * the last failure on the calling thread is osw_last_error().  Host buffers are
 * caller-owned and only read/written during the call (the library copies them).
 * A context serialises its own calls (internal mutex); one context per device.
 * No torch types cross this boundary.
 *
 * Concurrency contract (the reference calls transcribe from several executor pools at
 * once, src/main.py:305, src/streaming.py:50-52, src/realtime/server.py:33-35, and loads
 * models on demand while serving, src/backends/faster_whisper.py:210-215):
 *   - any entry point may be called from any thread, on any context, at any time: calls
 *     on one context run one at a time; calls on different contexts (sibling lanes of
 *     one GPU, other GPUs, other models) run concurrently;
 *   - a context's decode steps are captured into hipGraphs on first use.  No entry point
 *     touches the legacy (null) stream: copies and memsets run on the context's own
 *     non-blocking stream.  Entry points that allocate, free, create or destroy streams
 *     (osw_create, osw_create_sibling, osw_destroy, osw_set_weight, osw_get_mel,
 *     osw_debug_gemm, a call whose input outgrows the resident buffers, the first ingest
 *     call on a device) wait for a capture in progress to end (one process-wide capture
 *     gate), so none of them can invalidate another context's capture;
 *   - the caller's own HIP / torch work in the same process must stay off the legacy
 *     stream while contexts are serving (e.g. run torch on a torch.cuda.Stream, which is
 *     non-blocking): HIP refuses legacy-stream work while any stream of the process
 *     captures, and the library cannot see it;
 *   - OSW_ECAPTURE reports a refused or invalidated stream capture: the context and the
 *     device remain usable, the call may be retried (it is not a device fault).
 */
#ifndef OSW_H
#define OSW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSW_OK 0
#define OSW_EINVAL (-22)
#define OSW_ENOMEM (-12)
#define OSW_EHIP (-100)
#define OSW_ESTATE (-101)
#define OSW_ECAPTURE (-102)

typedef struct osw_ctx osw_ctx;

/* n_audio_ctx is the encoder window: T = 50 * chunk_length positions for faster-whisper's
 * transcribe(chunk_length = 1..30 whole seconds), i.e. one of 50, 100, ..., 1500 (1500 = Whisper's own
 * 30 s window, the default everywhere).  osw_create returns OSW_EINVAL for any other value before it
 * allocates.  A context's window is fixed: every buffer is sized for it (X1 [w][2T + 2][C1], H1
 * [w][2T + 1][D], the residual / QKV / FC1 rows w * T, cross-K/V [L * 2][w][H][T][64]), "enc.pos" is a
 * [T][D] tensor (the first T rows of a checkpoint's table), a window holds at most 2T mel frames, and
 * sibling contexts share it.  The semantics (segment_size = min(100 * chunk_length, content_frames -
 * seek), zero padding to 100 * chunk_length frames, timestamp rules and the 448-position decoder
 * unchanged) restate upstream faster-whisper and are not pinned against it. */
typedef struct osw_dims {
    int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} osw_dims;

/* One decoding window (30 s unless the context was created with a shorter n_audio_ctx): frames
 * [seek, seek + segment_size) of clip `clip`'s log-mel, zero padded to 2 * n_audio_ctx frames (3000;
 * faster-whisper pad_or_trim); a larger segment_size is trimmed to that. */
typedef struct osw_window {
    int32_t clip;
    int32_t seek;
    int32_t segment_size;
} osw_window;

typedef struct osw_decode_opts {
    /* <|transcribe|> or <|translate|>.  < 0: an English-only model, whose start sequence is
     * <|startoftranscript|> alone: every prompt is [prefix..., sot(, no_timestamps)];
     * language_token, language_tokens, first_lang, n_langs and osw_session_window::language_token
     * are ignored, osw_window_result::language comes back -1, osw_detect_language returns
     * OSW_EINVAL and osw_get_language_probs OSW_ESTATE.  With timestamps <|startoftranscript|>
     * is the last prompt position, so that one decoder step gives both no_speech_prob (softmax
     * of its raw logits) and the first sampled token (the same logits under the rules). */
    int32_t task_token;
    int32_t language_token;      /* -1: detect from the <|startoftranscript|> logits */
    int32_t suppress_blank;      /* suppress " " and <|endoftext|> at the first sampled step */
    int32_t without_timestamps;  /* 0: timestamp rules on (faster-whisper default) */
    int32_t max_initial_timestamp_index; /* 50 = 1.0 s; -1 disables */
    int32_t max_length;          /* total positions (prompt + sampled), <= n_text_ctx */
    const int32_t* suppress_tokens; int32_t n_suppress;
    /* special token ids */
    int32_t eot, sot, sot_prev, no_speech, no_timestamps, timestamp_begin, blank;
    int32_t first_lang, n_langs;
    /* tokens placed BEFORE <|startoftranscript|> (e.g. <|startofprev|> + previous
     * text), n_windows * n_prefix ints, same length for every window of the call */
    const int32_t* prefix_tokens; int32_t n_prefix;
    /* optional per-window language tokens (n_windows ints; -1 = detect); NULL: use
     * language_token for every window */
    const int32_t* language_tokens;
    /* beam search (CTranslate2 BeamSearch semantics, as faster-whisper calls it):
     * beam_size <= 1 is greedy; windows * beam_size <= 5 * max_batch.  A caller
     * that sets beam_size > 1 must set length_penalty (0 = no length normalisation). */
    int32_t beam_size;           /* reference default 5 (src/backends/faster_whisper.py:237) */
    float patience;              /* <= 0 -> 1; stop once round(beam*patience) hypotheses finished */
    float length_penalty;        /* score / len**length_penalty ranks finished hypotheses */
    int32_t num_hypotheses;      /* <= 0 -> 1 */
    /* sampling = faster-whisper's temperature > 0 branch (beam 1, num_hypotheses = best_of,
     * sampling_topk 0): best_of decoder rows per window each draw every token from
     * softmax(logits / temperature) after the logits rules; the row with the best
     * sum_logprob / n_tokens**length_penalty is returned.  temperature <= 0: greedy or beam
     * search as above.  Replaces generate_with_fallback's sampling kwargs [upstream]. */
    float temperature;
    int32_t best_of;             /* <= 0 -> 1; windows * best_of <= 5 * max_batch */
    uint64_t seed;               /* draw seed (counter-hash Gumbel-max, reproducible) */
    /* length control (benches of realistic output lengths with random weights, which
     * never emit <|endoftext|> on their own): n_windows ints; greedy / sampling rows
     * emit <|endoftext|> once they have sampled token_budget[i] tokens, beam search
     * treats that step as the last one (<= 0: no limit).  NULL: off.  Not a reference
     * option. */
    const int32_t* token_budget;
    /* history rules = faster-whisper's transcribe(repetition_penalty=, no_repeat_ngram_size=),
     * i.e. CTranslate2's RepetitionPenalty and NoRepeatNgram logits processors [upstream; the
     * reference calls transcribe with neither, src/backends/faster_whisper.py:235-246].  A
     * decoder row's history is what it sampled so far in this window (timestamps included,
     * the prompt and the previous-text prefix excluded; a beam row: its own hypothesis).  On
     * every sampled step, on the raw fp32 logits and before every other rule:
     *   repetition_penalty p: x[t] = x[t] < 0 ? x[t] * p : x[t] / p for every distinct id t of
     *     the history (<= 0 or == 1: off, so a zeroed struct is off);
     *   no_repeat_ngram_size m: an id that would complete an m-gram the history already holds
     *     gets -inf (<= 0: off; 1 bans every id sampled so far).
     * sum_logprob and the beam scores come from the penalised distribution, as CTranslate2's
     * do; language detection and no_speech_prob stay on the raw logits. */
    float repetition_penalty;
    int32_t no_repeat_ngram_size;
} osw_decode_opts;

/* Caller-allocated outputs for n windows. */
typedef struct osw_window_result {
    int32_t* tokens;          /* [n][max_tokens]: sampled tokens (no prompt, no EOT) */
    int32_t max_tokens;
    int32_t* n_tokens;        /* [n] */
    float* sum_logprob;       /* [n]  includes the EOT step, as CTranslate2 scores do */
    float* no_speech_prob;    /* [n]  softmax(raw SOT logits)[no_speech] */
    int32_t* language;        /* [n]  language token used */
    float* logits_dump;       /* optional [n][dump_steps][n_vocab] raw logits of the first sampled steps */
    int32_t dump_steps;
} osw_window_result;

typedef struct osw_profile {
    double mel_ms, encoder_ms, crosskv_ms, decoder_ms, total_ms;
    int64_t decode_steps;           /* decoder steps launched in the last decode call */
    /* dominant-kernel accounting (HIP events around every launch of the class) */
    double enc_gemm_ms; int64_t enc_gemm_launches; double enc_gemm_flops;
    double enc_attn_ms; int64_t enc_attn_launches; double enc_attn_flops;
    double mel_kernel_ms; int64_t mel_kernel_launches; double mel_kernel_bytes;
    double xattn_ms; int64_t xattn_launches; double xattn_bytes;
} osw_profile;

const char* osw_version(void);
const char* osw_last_error(void);
int osw_device_count(int32_t* out);

/* Model widths served: n_audio_state == n_text_state in {128, 256, 384, 512, 768, 1024, 1280}
 * with 64-wide heads (512 / 768 / 1024 / 1280 are Whisper base / small / medium / large).  Any
 * other width, the multiples of 128 in between (640, 896, 1152) included, has no LayerNorm
 * kernel and returns OSW_EINVAL. */
int osw_create(const osw_dims* dims, int32_t device, int32_t max_batch, osw_ctx** out);
int osw_destroy(osw_ctx* ctx);
/* A second context on the parent's device that SHARES the parent's (finalized)
 * weights but owns its stream, workspaces and decode state.  Two contexts per GPU
 * driven from two host threads overlap one batch's MFMA-bound encoder with the
 * other's HBM/latency-bound decoder (the faster-whisper reference runs one
 * WhisperModel per process, src/backends/faster_whisper.py:40-45; this is the
 * batcher's per-GPU lane, not a reference entry point).  The weights stay alive
 * until the last context sharing them is destroyed; weight setters on a sibling
 * return OSW_EINVAL. */
int osw_create_sibling(osw_ctx* parent, int32_t max_batch, osw_ctx** out);

/* Sibling contexts serialise their encoders on the GPU (the encoder baton: one lane
 * encodes while the others decode); an encoder of fewer than `min_windows` windows skips
 * it, so small streaming encoders of sibling lanes run side by side.  Default 9
 * (OSW_BATON_MIN_WINDOWS); 0 = every encoder takes the baton.  Per context. */
int osw_set_encoder_baton_min(osw_ctx* ctx, int32_t min_windows);

/* Upload one canonical tensor (names and dtypes: open-speech_amd/weights.py). */
int osw_set_weight(osw_ctx* ctx, const char* name, const void* host, int64_t nbytes);
/* Read one tensor back as stored on the device (enc.conv1.w: the padded [De][3][C1]
 * layout).  For tests and checkpoint round trips. */
int osw_get_weight(osw_ctx* ctx, const char* name, void* host, int64_t nbytes);
/* Int8 decoder weights (weight-only quantisation, STT_COMPUTE_TYPE=int8_float16): matrix `name`
 * becomes W[n][k] ~ q[n][k] * mult[n], q int8 [N][K] row-major (n_q = N * K elements), mult fp32
 * [N] (n_mult = N, every entry finite).  Accepted for the seven matrix kinds the skinny decoder
 * GEMM streams: dec.tok and dec.lN.{qkv,o,xq,xo,fc1,fc2}.w; any other name, a wrong count or a K
 * that is no multiple of 64 returns OSW_EINVAL.  The device then holds fp16(q) in the tensor
 * itself (exact; what osw_get_weight returns for it), mult in "<name>.scale" and the int8
 * fragment copy the skinny kernel streams in "<name>.frag".  The activations stay the hi/lo fp16
 * pairs: the kernels run the float16 MFMA chain on fp16(q) and multiply each fp32 accumulator once
 * by mult[n] before it leaves (a C or split-K slab element is fp32(acc * mult[n]); the bias is
 * added after).  The state is per matrix and shared with sibling contexts, like the weights;
 * osw_set_weight / osw_init_weight_uniform make the matrix float16 again.  Locking, capture gate
 * and sibling rules are osw_set_weight's.  A change of kind (float16 <-> int8) is REFUSED
 * (OSW_EINVAL) once this context holds decode graphs or sibling contexts exist: their graphs
 * have the kernels of the old kind baked in (a destroyed sibling no longer counts).  An int8 dec.tok
 * needs an int8 dec.l0.qkv.w (the embedding is that GEMM's prologue in the one-row step): the mix is
 * refused by osw_finalize and by every decode call, at every batch size.  The opt-in OSW_GELU_TAIL / OSW_B1_ATTN_TAIL forms
 * have no int8 kernels: a decode that would reach them with an int8 matrix returns an error. */
/* (The three int8 entry points carry no digit in their names: the binding check matches [a-z_].) */
int osw_set_weight_quant(osw_ctx* ctx, const char* name, const int8_t* q, const float* mult, int64_t n_q,
                      int64_t n_mult);
/* *out = 1 when matrix `name` holds int8 weights, else 0; a name that is not one of the seven
 * matrix kinds above returns OSW_EINVAL. */
int osw_weight_is_quant(osw_ctx* ctx, const char* name, int32_t* out);
/* Device-side counter-hash init: x[i] = (2u-1)*scale + offset, u from splitmix64. */
int osw_init_weight_uniform(osw_ctx* ctx, const char* name, uint64_t seed, int64_t stream,
                            float scale, float offset, int64_t zero_lo, int64_t zero_hi);
int osw_finalize(osw_ctx* ctx);   /* all tensors present? derive internal layouts */

/* PCM int16 of n_clips clips, clip i = pcm[offsets[i], offsets[i+1]).  When
 * pcm_on_device != 0, `pcm` is a device pointer on the context's device.
 * Computes the faster-whisper log-mel (padding 160, per-clip max clamp) and keeps it
 * resident; n_frames[i] receives the frame count of clip i. */
int osw_log_mel(osw_ctx* ctx, const int16_t* pcm, const int64_t* offsets, int32_t n_clips,
                int32_t pcm_on_device, int32_t* n_frames);
int osw_get_mel(osw_ctx* ctx, int32_t clip, float* out, int64_t out_floats);  /* [n_mels][n_frames] */

/* Encoder + cross-attention K/V for n windows of the resident log-mel. */
int osw_encode_windows(osw_ctx* ctx, const osw_window* windows, int32_t n);
int osw_get_encoder_output(osw_ctx* ctx, int32_t window, float* out, int64_t out_floats); /* [n_audio_ctx][D] */

/* Decode of the n windows last encoded, per `opts`: greedy (beam_size <= 1,
 * temperature <= 0), CTranslate2-style beam search (beam_size > 1; the reference calls
 * beam_size = 5, src/backends/faster_whisper.py:237) or sampling (temperature > 0,
 * best_of rows per window).  The prompt, logits rules and stop rules are the same in
 * all three modes. */
int osw_decode_windows(osw_ctx* ctx, int32_t n, const osw_decode_opts* opts, osw_window_result* res);

/* Decode of n of the windows last encoded: windows[i] indexes the last osw_encode_windows call,
 * the indices distinct and in range, 1 <= n <= that call's window count (else OSW_EINVAL, before
 * any launch; OSW_EINVAL too while a session is open).  Entry i of every per-window array of
 * `opts` (prefix_tokens, language_tokens, token_budget) and of `res`, and confidence result i,
 * belong to windows[i]; decoder rows are i * group + k.  The result is bit for bit what
 * osw_decode_windows(n) returns after encoding just these windows in this order, in every mode,
 * the same seed giving the same draws.  The call reads the cross-K/V where it lies and writes
 * neither it nor the encoder output; the encode call's window count stays, so a later
 * osw_decode_windows, osw_detect_language or osw_align_windows (with the original window
 * indices) returns what it would have returned without this call. */
int osw_decode_window_list(osw_ctx* ctx, int32_t n, const int32_t* windows, const osw_decode_opts* opts,
                           osw_window_result* res);

/* mel + encode + decode (greedy, beam search or sampling per `opts`, as
 * osw_decode_windows) of window 0 (seek 0, min(frames, 2 * n_audio_ctx)) of every clip. */
int osw_transcribe_batch(osw_ctx* ctx, const int16_t* pcm, const int64_t* offsets, int32_t n_clips,
                         int32_t pcm_on_device, const osw_decode_opts* opts, osw_window_result* res);

/* Greedy transcription of window 0 of every clip (as osw_transcribe_batch) with row refill:
 * the decoder keeps max_batch rows, each with its own step counter, and a finished
 * window's row is refilled with the next queued clip (its window encoded straight into
 * that row's cross-K/V slot) once refill_min rows are free.  n_clips may exceed max_batch.
 * Each clip's result equals osw_transcribe_batch's.  Replaces the same per-file
 * WhisperModel.transcribe calls (src/backends/faster_whisper.py:235-246) when a caller has
 * many files queued; opts: temperature 0, beam_size 1, no prefix (OSW_EINVAL otherwise). */
int osw_transcribe_refill(osw_ctx* ctx, const int16_t* pcm, const int64_t* offsets, int32_t n_clips,
                          int32_t pcm_on_device, const osw_decode_opts* opts, osw_window_result* res,
                          int32_t refill_min);

/* ---- decode sessions: continuous batching of windows (greedy or beam search) ----
 * A session keeps max_batch window slots on the context (beam search: beam_size decoder
 * rows per slot, each with its own step counter and prompt).  Windows are queued with
 * osw_session_add and admitted into free slots between chunks of 4 decoder steps (their
 * encoder runs straight into the slot's cross-K/V); a finished window leaves its slot at
 * once.  So a window queued while others decode joins at the next chunk instead of
 * waiting for the longest window of a batch, and a caller can queue the next window of a
 * file (its previous-text prefix included) as soon as the previous one finished.  Each
 * window's result equals osw_decode_windows's for it alone: rows are independent in every
 * kernel.  Replaces the per-request WhisperModel.transcribe loops that the reference runs
 * from concurrent executor threads (src/main.py:305, src/streaming.py:366-375,
 * src/backends/faster_whisper.py:235-246) with one decoder batch per context.
 * opts: temperature 0 (greedy, or beam search with beam_size <= 5); its prefix_tokens,
 * language_tokens and token_budget are ignored (per window below).  While a session is
 * open the context's other decode entry points return OSW_EINVAL. */
typedef struct osw_session_window {
    int64_t tag;              /* the caller's id, returned with the result */
    int32_t seek;             /* first mel frame of the window in its clip */
    int32_t segment_size;     /* frames (<= 2 * n_audio_ctx) */
    int32_t language_token;   /* -1: detect */
    int32_t token_budget;     /* length control (benches): <= 0 none */
    int32_t n_prefix;         /* previous-text prompt tokens before <|startoftranscript|> */
    const int32_t* prefix;    /* <|startofprev|> and the previous tokens, or NULL */
    /* >= 0: the caller's key of the window's clip.  The first window of a key brings the
     * clip's PCM; its log-mel is computed once and stays on the device, so later windows of
     * the same key pass no samples (offsets[i] == offsets[i+1]) and are staged from it,
     * until osw_session_release_clip(key) or osw_session_end.  < 0: the window's own PCM,
     * used for this window only. */
    int64_t clip;
} osw_session_window;
int osw_session_begin(osw_ctx* ctx, const osw_decode_opts* opts);
/* Queue n windows; window i reads clip pcm[offsets[i], offsets[i+1]) (host int16, copied). */
int osw_session_add(osw_ctx* ctx, const int16_t* pcm, const int64_t* offsets, int32_t n,
                    const osw_session_window* windows);
/* Admit queued windows into free slots (when at least min(refill_min, queued) slots are
 * free, or nothing decodes) and run up to max_chunks chunks of decoder steps, returning
 * after the first chunk in which windows finished (max_chunks 0: only admit, and wait for
 * the admitted windows' encoder).  Their results go to res[0 .. *n_done)
 * (res->tokens rows of res->max_tokens), their tags to tags_out; cap >= max_batch.
 * *n_active / *n_queued: windows decoding / waiting after the call. */
int osw_session_step(osw_ctx* ctx, int32_t max_chunks, int32_t refill_min, osw_window_result* res,
                     int64_t* tags_out, int32_t cap, int32_t* n_done, int32_t* n_active, int32_t* n_queued);
/* Frees the resident log-mel of clip `clip` (no queued window may still read it; windows
 * already admitted were staged and are unaffected). */
int osw_session_release_clip(osw_ctx* ctx, int64_t clip);
/* Ends the session: queued and decoding windows are dropped, held windows (below) and resident
 * clips freed. */
int osw_session_end(osw_ctx* ctx);

/* ---- word timestamps on a session: hold, align, release ----
 * The alignment pass (osw_align_windows, below) needs a window's cross-K/V after the caller has
 * split the window into segments and knows its text tokens, but a session gives a finished
 * window's slot to the next admission in the call that returns it.  With hold on, the slot
 * waits: a window osw_session_step returns is HELD, its cross-K/V stays as the encoder left it,
 * nothing is admitted into its slot, osw_session_step never reports it again and it no longer
 * counts in *n_active (windows decoding).  The caller then aligns it (osw_session_align) or lets
 * it go (osw_session_release); either frees the slot for the next admission.  A caller is
 * expected to do so for everything a step returned before its next step: when nothing decodes,
 * every slot is held and windows are queued, osw_session_step returns at once with *n_done == 0,
 * launches nothing and waits for nothing.  osw_session_end frees whatever is still held.
 * A slot is free, decoding or held; the transitions are those of csrc/slots.h.
 *
 * osw_session_hold: valid after osw_session_begin and before the session's first
 * osw_session_add, else OSW_ESTATE (also without an open session).  enable != 0 turns hold on
 * for this session; a session that never calls it behaves as above ("leaves its slot at once"),
 * bit for bit.  In a hold-mode session a window is named by its tag from the step that returns
 * it to its align or release, so osw_session_add refuses (OSW_EINVAL, nothing queued) a tag that a
 * queued, decoding or held window of the session already carries, or that appears twice in the
 * call; a tag is free again once its window was aligned or released.
 *
 * osw_session_align: the alignment of n held windows, then their slots freed.  tags[i] names
 * entry i's window; w[i] is an osw_align_window (below) whose `window` is ignored and whose other
 * fields, and `res`, mean what they mean for osw_align_windows, with the same OSW_EINVAL checks
 * (n_tokens == 0 included: an empty result, the slot freed).  Every tag must be held and the tags
 * distinct: a tag that is unknown, still queued or decoding, or already aligned or released is
 * OSW_EINVAL.  A refused call (any OSW_EINVAL above) changes nothing: no slot is freed, nothing
 * is launched.  The pass runs one decoder row per entry on row state of its own and reads each
 * row's cross-K/V from its window's slot; it writes nothing a decoding row reads, so every other
 * window of the session still decodes exactly as it does alone, and entry i's result is bit for
 * bit what osw_align_windows returns for that window after a batched decode.  After the call
 * osw_get_alignment_matrix(ctx, i, ...) returns M of entry i.  Replaces the same ctranslate2
 * Whisper.align call as osw_align_windows [upstream], for windows decoded in a session.
 *
 * osw_session_release: frees the slots of n held windows without aligning them (a window skipped
 * as silence, one without text tokens, a failed request).  Tags as for osw_session_align: all
 * held and distinct, else OSW_EINVAL and nothing is freed.  n == 0 is a no-op.
 *
 * osw_align_windows stays OSW_EINVAL while a session is open, with or without hold. */
struct osw_align_window;
struct osw_align_result;
int osw_session_hold(osw_ctx* ctx, int32_t enable);
int osw_session_align(osw_ctx* ctx, int32_t n, const int64_t* tags, const struct osw_align_window* w,
                      struct osw_align_result* res);
int osw_session_release(osw_ctx* ctx, int32_t n, const int64_t* tags);

/* ---- temperature fallback on a session: retry a held window in place ----
 * faster-whisper's generate_with_fallback decodes a window again at the next temperature of a
 * ladder when its text is too repetitive or its average log-probability too low.  A held window
 * (above) has what a retry needs, its slot and its cross-K/V, so it goes back to decoding where it
 * is, with best_of sampled rows, beside slots that go on at temperature 0; the encoder does not run.
 *
 * osw_session_retries: valid in a hold-mode session, after osw_session_hold(1) and before the
 * session's first osw_session_add, else OSW_ESTATE (also without an open session).  1 <= best_of
 * <= 5, else OSW_EINVAL.  The session then keeps max(beam_size, best_of) decoder rows per slot
 * (the context has 5 x max_batch rows; nothing is allocated per row).  A session that never calls
 * it runs the statements and launches it ran before.
 *
 * osw_session_retry: n held windows decode again.  entries[i].tag names a held window; all tags
 * held and distinct, every temperature finite and > 0, every language_token inside the vocabulary
 * (an English-only model ignores it), else OSW_EINVAL; a session without osw_session_retries:
 * OSW_ESTATE.  A refused call launches nothing and changes nothing.  Each window's slot goes from
 * held to decoding; its rows restart at step 0 of the prompt it was admitted with (prefix, token
 * budget; the language position holds language_token: pass the language attempt 0 reported), rows
 * 0 .. best_of-1 sample at `temperature` with `seed`, the slot's other rows are parked.  When all
 * its sampled rows have ended, osw_session_step returns the window again, held: the row with the
 * highest sum_logprob / n_tokens^length_penalty (the first on ties), as osw_decode_windows returns
 * for temperature > 0.  That result is bit for bit what osw_decode_windows returns for the window
 * as the first of its call with the same temperature, best_of, seed, prefix, language and token
 * budget, and every window decoding beside it still decodes as it does alone.  The caller then
 * retries it again, aligns it or releases it; admission into a released slot puts its rows back
 * to temperature 0. */
typedef struct osw_retry_window {
    int64_t tag;
    float temperature;
    uint64_t seed;
    int32_t language_token;
} osw_retry_window;
int osw_session_retries(osw_ctx* ctx, int32_t best_of);
int osw_session_retry(osw_ctx* ctx, int32_t n, const osw_retry_window* entries);

/* ---- confidences: per-token log-probabilities and language probabilities ----
 * Off by default.  On, every decode entry point (osw_decode_windows, osw_transcribe_batch,
 * osw_transcribe_refill, osw_session_step) also keeps, per returned window, what the token
 * selection computes anyway: the row's cumulative log-probability after each sampled step and
 * the softmax over the language tokens' raw <|startoftranscript|> logits.  Tokens, sum_logprob,
 * no_speech_prob and language are the same bits on and off.  Replaces the scores CTranslate2's
 * Whisper.generate(return_scores=True) returns per hypothesis, refined to one value per token
 * (OpenAI's include[]=logprobs), and faster-whisper's TranscriptionInfo.language_probability /
 * all_language_probs [upstream]; the reference reads neither (src/backends/faster_whisper.py:
 * 235-260).  OSW_EINVAL while a session is open (a session keeps the setting it began with). */
int osw_set_confidences(osw_ctx* ctx, int32_t enable);
/* Result i of the last result-producing call on this context (window i of osw_decode_windows /
 * osw_transcribe_batch, clip i of osw_transcribe_refill, entry i of the last osw_session_step's
 * done-list; sampling: the best_of row that was returned).  cum[j] = the fp32 cumulative
 * log-probability after token j; *n = the window's n_tokens, plus one closing entry when the row
 * ended with an <|endoftext|> step (picked, or forced by its token budget), none when it was cut
 * at max_length.  The last entry equals the window's sum_logprob bit for bit; token j's own
 * log-probability is cum[j] - cum[j - 1] (the caller subtracts, in double).  cum may be NULL to
 * query *n.  OSW_ESTATE with confidences off or before any such call. */
int osw_get_token_logprobs(osw_ctx* ctx, int32_t i, float* cum, int32_t cap, int32_t* n);
/* probs[n_langs] of the same result i: softmax over logits[first_lang .. first_lang + n_langs) at
 * the <|startoftranscript|> step (CTranslate2 detect_language's distribution), whether the
 * language was detected or given.  n_langs must be the decode call's.  OSW_ESTATE as above, and
 * after an English-only decode (task_token < 0), which records no language distribution. */
int osw_get_language_probs(osw_ctx* ctx, int32_t i, float* probs, int32_t n_langs);
/* Language detection alone for the n windows of the last osw_encode_windows call: one decoder
 * step on <|startoftranscript|> (no prefix), then the same language softmax; probs [n][n_langs],
 * raw_logits (optional) [n][n_langs] the logits it was taken over.  opts supplies the token ids
 * only (sot, task_token, first_lang, n_langs).  Needs no osw_set_confidences, touches no result
 * of an earlier call, and a later osw_decode_windows of the same windows returns what it would
 * have without it.  Runs on the context's stream and allocates nothing.  Replaces
 * WhisperModel.detect_language() -> ctranslate2 Whisper.detect_language [upstream].  An
 * English-only model (opts->task_token < 0) has nothing to detect: OSW_EINVAL before any launch.  OSW_EINVAL
 * while a session is open. */
int osw_detect_language(osw_ctx* ctx, int32_t n, const osw_decode_opts* opts, float* probs, float* raw_logits);

/* ---- word timestamps: cross-attention alignment + dynamic time warping ----
 * The alignment heads as n (layer, head) pairs (an HF generation_config.json's
 * "alignment_heads"); n = 0 restores the default, every head of the last n_text_layer / 2
 * layers (openai-whisper's default).  Replaces the alignment_heads CTranslate2 reads from
 * the model's config.json [upstream]. */
int osw_set_alignment_heads(osw_ctx* ctx, const int32_t* layer_head_pairs, int32_t n);

/* One window to align: the forced sequence is [sot, language, task, no_timestamps,
 * tokens[0 .. n_tokens), eot] (no previous-text prefix; every text token < eot).  language < 0
 * and task < 0 together: an English-only model's [sot, no_timestamps, tokens..., eot]
 * (faster-whisper passes the tokenizer's sot_sequence, (sot,) for such a model); the rows kept
 * are [no_timestamps, tokens...] either way.  One of the two negative alone: OSW_EINVAL. */
typedef struct osw_align_window {
    int32_t window;               /* index into the last encode / decode / transcribe_batch call */
    int32_t sot, language, task, no_timestamps, eot;
    const int32_t* tokens;        /* text tokens, timestamp tokens removed */
    int32_t n_tokens;             /* 0: no work, empty results */
    int32_t num_frames;           /* the window's segment_size; F = num_frames / 2 key frames are aligned */
    int32_t median_filter_width;  /* <= 0: 7 (odd, <= 15) */
} osw_align_window;
typedef struct osw_align_result {
    int32_t* token_frame;         /* [n][stride]: n_tokens + 1 entries per window (the last is eot's); time = frame * 0.02 s */
    double* token_prob;           /* [n][stride]: n_tokens entries, softmax(logits[:eot])[token]; double, since a
                                   * forced token can be less likely than fp32 can hold (the device keeps log p) */
    int32_t stride;               /* >= the largest n_tokens + 1 */
} osw_align_result;
/* Teacher-forced decoder pass over the cross-K/V still resident from the last
 * osw_encode_windows / osw_decode_windows / osw_transcribe_batch call, for n distinct
 * windows of it: the alignment heads' softmax over the n_audio_ctx keys, cropped to F frames,
 * normalised per (head, frame) over the positions, median-filtered along the frames, averaged
 * over the heads, rows [no_timestamps, tokens...] kept (the matrix M), then DTW over -M
 * (transformers' _dynamic_time_warping tie rule) and the first frame of each token.  A
 * window's result does not depend on the others of the call.  Replaces ctranslate2
 * Whisper.align as faster-whisper's find_alignment calls it [upstream].  OSW_EINVAL while a
 * session is open, for a window index the last call does not hold, or n_tokens + 5 > n_text_ctx
 * (English-only: n_tokens + 3). */
int osw_align_windows(osw_ctx* ctx, int32_t n, const osw_align_window* w, osw_align_result* res);
/* M [T = n_tokens + 1][F] of `window` as the last osw_align_windows call left it (*T = *F = 0
 * when that call did not align it or it had no text); out may be NULL to query the shape. */
int osw_get_alignment_matrix(osw_ctx* ctx, int32_t window, float* out, int64_t out_floats, int32_t* T, int32_t* F);
/* The DTW kernel alone on a host cost matrix x [T][F] (T <= 511, F <= 4096): the path as
 * text_idx / time_idx [*len], *len <= T + F - 1 (caller buffers of T + F ints).  Replaces
 * openai-whisper timing.dtw / transformers' _dynamic_time_warping for the parity tests. */
int osw_debug_dtw(osw_ctx* ctx, const float* x, int32_t T, int32_t F, int32_t* text_idx, int32_t* time_idx,
                  int32_t* len);

/* ---- the other alignment kernels, one production launcher per call on host data (parity tests:
 * tests/test_gpu_align_kernels.py; references: tests/align_kernels_ref.py) ----
 * Like the attention calls below: temporary device buffers, exactly one call of the launcher the
 * alignment pass uses on the context's stream, the results copied back.  Shapes are arguments and
 * do not depend on the context's dims (head width 64; positions <= 448).  Whatever could make a
 * kernel index out of bounds is OSW_EINVAL before any launch.  Pure outputs are filled with 0xff
 * bytes (a NaN pattern) before the launch, so an unwritten element and a stray store both show;
 * in/out arrays come back as the launch left them.  They replace no reference interface: the
 * reference runs these steps inside CTranslate2 Whisper::align [upstream].
 *
 * launch_align_post: scores fp32 [n_slots][n_heads][pstride][TK] (raw scaled scores; rows p >= len
 * are never read) -> stats [n_slots][n_heads][pstride][2] (row max, sum of exp over all TK keys),
 * colstats [n_slots][n_heads][TK][2] (mean and population std over positions 0 .. len - 1 of the
 * probabilities of frames < frames[slot]), M [n_slots][pstride][TK] (rows 0 .. len - head - 2,
 * frames < frames[slot]).  OSW_EINVAL: pstride % 16 != 0 or > 448, len > pstride, len < head + 2,
 * frames outside [1, TK], an even width or one above 15, head not 1 or 3. */
int osw_debug_align_post(osw_ctx* ctx, const float* scores, int32_t n_slots, int32_t n_heads, int32_t pstride,
                         int32_t TK, const int32_t* len, const int32_t* head, const int32_t* frames,
                         const int32_t* width, float* stats, float* colstats, float* M);
/* launch_align_tail at position pos: logits fp32 [rows][V], forced [rows][ctx], per row slot (-1:
 * not aligned; else distinct, < n_slots), len (<= ctx) and head (1 or 3).  In/out: token_logprob
 * [n_slots][ctx], cur_tok [rows], done [rows] (packed into and unpacked from the kernel's row
 * state).  OSW_EINVAL: eot outside [1, V], ctx > 448, a forced token outside [0, V). */
int osw_debug_align_tail(osw_ctx* ctx, const float* logits, int32_t rows, int32_t V, int32_t eot, int32_t ctx_len,
                         int32_t pos, const int32_t* slot, const int32_t* len, const int32_t* head,
                         const int32_t* forced, int32_t n_slots, float* token_logprob, int32_t* cur_tok,
                         int32_t* done);
/* launch_align_self_attn at position pos (clamped to ctx_len - 1 by the kernel): qkv_slabs fp32
 * [ks][rows][3 D], D = 64 H, bias [3 D], done [rows] (a row with done != 0 is skipped).  In/out:
 * the fp32 caches kcache, vcache [rows][H][ctx_len][64].  out fp32 [rows][D] = the kernel's fp16
 * hi + lo pair, summed (NaN where nothing was written).  OSW_EINVAL: ctx_len > 448, pos < 0. */
int osw_debug_align_self_attn(osw_ctx* ctx, const float* qkv_slabs, int32_t ks, const float* bias, float* kcache,
                              float* vcache, int32_t rows, int32_t H, int32_t ctx_len, int32_t pos,
                              const int32_t* done, float* out);
/* launch_align_scores at position pos: q_slabs fp32 [ks][rows][D], D = 64 H, bias [D] or NULL, K
 * fp16 [rows][H][T][64], layer_heads n_layer_heads pairs {head < H, head_idx < n_heads} with
 * distinct head_idx, per row slot (-1 or distinct, < n_slots) and len (<= pstride).  In/out:
 * scores fp32 [n_slots][n_heads][pstride][T]; a row with slot >= 0 and pos < len writes row pos
 * of each listed head_idx. */
int osw_debug_align_scores(osw_ctx* ctx, const float* q_slabs, int32_t ks, const float* bias, const void* K,
                           int32_t rows, int32_t H, int32_t T, const int32_t* layer_heads, int32_t n_layer_heads,
                           int32_t n_heads, int32_t pos, const int32_t* slot, const int32_t* len, int32_t pstride,
                           int32_t n_slots, float* scores);

/* The history-rules kernel alone (osw_decode_opts::repetition_penalty / no_repeat_ngram_size) on
 * host data: logits [rows][V] in and out, row r's history tokens[r * stride .. + n_hist[r]).
 * Replaces CTranslate2's RepetitionPenalty / NoRepeatNgram (transformers'
 * RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor) for the parity tests.
 * OSW_EINVAL for n_hist[r] > stride, stride > n_text_ctx, or a token outside [0, V). */
int osw_debug_history_rules(osw_ctx* ctx, float* logits, int32_t rows, int32_t V, const int32_t* tokens,
                            int32_t stride, const int32_t* n_hist, float repetition_penalty,
                            int32_t no_repeat_ngram_size);
/* Timing helper (tools/history_rules_bench.py): the same kernel on `rows` rows of V zero logits,
 * every row with a period-3 history of n_hist tokens, launched `iters` times back to back;
 * *us = mean time per launch (HIP events).  OSW_EINVAL with both rules off. */
int osw_debug_history_rules_time(osw_ctx* ctx, int32_t rows, int32_t V, int32_t n_hist, float repetition_penalty,
                                 int32_t no_repeat_ngram_size, int32_t iters, float* us);

/* One selection step (launch_select and, for beam_size > 1, launch_beam: exactly what a decode
 * step launches after its logits GEMM, plus the history rules when the options turn them on) on
 * caller-supplied logits and state, for the per-kernel tests (tests/test_gpu_select.py).  The
 * entry builds the decode plan of `mode` from `opts` (seed included; token_budget is taken from
 * io->budget), binds it to the context's own buffers, uploads the state, launches, and copies
 * every in/out array back.  The arrival and ticket counters are the context's own and are NOT
 * reset: `counters` returns them as the launch left them (all zero, or the next call misbehaves).
 * SelState travels as 10 32-bit words per row {n_sampled, last, penult, last_ts, done, lang,
 * sum_lp (float), nsp (float), plen, n_lp}, BeamWin as 6 per window {n_hyp, best_len, done,
 * best_nlp, best_norm (float), best_raw (float)}.  Every *_len is the array's size in elements
 * (words); an array the mode does not use may be NULL with length 0.
 * OSW_EINVAL, before any launch, for whatever could make a kernel index out of bounds: rows not a
 * multiple of the group (beam_size, or best_of when sampling) or above the row capacity, windows
 * above max_batch, a step counter outside [0, n_text_ctx), n_sampled outside [0, max_tok], a
 * sampling row whose counter is not plen - 1 + n_sampled, plen out of range (sessions; 0
 * elsewhere), a prompt or history token outside [0, V) other than the -1 language placeholder,
 * rows of one beam window that differ in n_sampled / plen / done / counter, an ancestry entry
 * outside the window's rows, max_tok or pstride that are not the plan's, an undersized array, or
 * an open session. */
#define OSW_SELECT_BATCH 0
#define OSW_SELECT_REFILL 1
#define OSW_SELECT_SESSION 2
typedef struct osw_select_io {
    int32_t mode;      /* OSW_SELECT_* */
    int32_t n_prefix;  /* batch: prompt positions before <|startoftranscript|> */
    int32_t rows;      /* decoder rows: windows x group */
    int32_t max_tok;   /* ints per row of tokens / best_tok: max(1, max_length - prompt length) */
    int32_t pstride;   /* ints per row of prompt: the prompt length (sessions: n_text_ctx) */
    int64_t logits_len, pos_len, state_len, prompt_len, cur_tok_len, tokens_len, budget_len, anc_len, bwin_len,
        best_tok_len, lp_hist_len, best_lp_len, lang_probs_len, counters_len;
    float* logits;         /* [rows][V]; copied back only with a history rule on */
    int32_t* pos;          /* batch: [1] the shared step counter, else [rows]; in/out */
    int32_t* state;        /* [rows][10]; in/out */
    const int32_t* prompt; /* [rows][pstride] */
    int32_t* cur_tok;      /* [rows]; in/out */
    int32_t* tokens;       /* [rows][max_tok]; in/out */
    const int32_t* budget; /* [rows] or NULL: no budgets (sessions: zeros) */
    int32_t* anc;          /* beam: [rows][n_text_ctx]; in/out */
    int32_t* bwin;         /* beam: [windows][6]; in/out */
    int32_t* best_tok;     /* beam: [windows][max_tok]; in/out */
    float* lp_hist;        /* confidences on: [rows][n_text_ctx]; in/out */
    float* best_lp;        /* confidences on, beam: [windows][n_text_ctx]; in/out */
    float* lang_probs;     /* confidences on, multilingual: [windows][n_langs]; in/out */
    int32_t* counters;     /* out: [1 + rows] rows finalised, then each row's slice tickets */
} osw_select_io;
int osw_debug_select_step(osw_ctx* ctx, const osw_decode_opts* opts, const osw_select_io* io);
/* The same in OSW_SELECT_SESSION mode for a retry session (osw_session_retries): rows_per_slot =
 * max(beam_size, best_of) decoder rows per window slot (beam_size <= rows_per_slot <= 5), io->rows a
 * multiple of it, and the rows' sampling state row_inv_temp[rows] (finite, >= 0) / row_seed[rows].
 * A slot whose first row holds row_inv_temp > 0 samples on its rows with row_inv_temp > 0 and its
 * other rows are parked; any other slot steps its first beam_size rows at temperature 0 and the
 * rest are parked.  Parked rows are neither read nor written.  The beam-window consistency checks
 * above apply to the temperature-0 slots' first beam_size rows. */
int osw_debug_select_step_rows(osw_ctx* ctx, const osw_decode_opts* opts, const osw_select_io* io,
                               int32_t rows_per_slot, const float* row_inv_temp, const uint64_t* row_seed);

/* Parity helper: one encoder block on x [T][D] fp32 (host), result to y (host). */
int osw_encoder_layer_debug(osw_ctx* ctx, int32_t layer, const float* x, float* y, int32_t T);

/* Parity/timing helper: C[M][N] (fp32) = A[M][K] · W[N][K]ᵀ (fp16 host inputs) with GEMM
 * variant 0 = auto, 1 = 128x128 tile, 2 = 256x256 tile, 3 = skinny split-K (M <= 64);
 * runs `iters` times and stores the mean kernel time (ms, HIP events) in *ms. */
int osw_debug_gemm(osw_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t variant, const void* A, const void* W,
                   float* C, int32_t iters, float* ms);

/* ---- one attention launch on host data (parity tests: tests/test_gpu_attention.py) ----
 * Each call copies its inputs to temporary device buffers, launches the kernel once on the
 * context's stream and copies the result back; like osw_debug_gemm they allocate, so they wait
 * for a capture in progress.  They replace no reference interface: the reference's attention
 * runs inside CTranslate2 [upstream].
 *
 * Encoder self-attention softmax(Q Kᵀ / 8) V over the context's T = n_audio_ctx positions: qkv fp16
 * [3][nb][H][T][64] (the QKV GEMM's head-major output), out fp16 [nb * T][H * 64].  nb <= 64
 * and H <= 20 are independent of the context's dims.  form 0: the production launcher's choice
 * (64-query workgroups below 512 units of 128, lazy running max, unpipelined, unless the OSW_ATTN_*
 * environment says otherwise); an explicit form is OSW_ATTN_FORM | any of _EAGER (rescale O on
 * every key tile), _QB128 (128 queries per workgroup instead of 64), _PIPE (software-pipelined). */
#define OSW_ATTN_FORM 1
#define OSW_ATTN_FORM_EAGER 2
#define OSW_ATTN_FORM_QB128 4
#define OSW_ATTN_FORM_PIPE 8
int osw_debug_enc_attn(osw_ctx* ctx, const void* qkv, int32_t nb, int32_t H, int32_t form, void* out);
/* Decoder cross-attention of `rows` = windows x beam decoder rows (beam <= 8, windows <= max_batch)
 * over each window's T = n_audio_ctx encoder keys, with the context's n_text_head heads H and width D = 64 H:
 * q_slabs fp32 [ks][rows][D] are the q projection's split-K partials (q = fp16(bias + their sum)),
 * bias [D] or NULL, K and V fp16 [windows][H][T][64]; out fp32 [rows][D] = the kernel's fp16
 * hi + lo output pair, summed.  legacy 1 passes no workspace, which selects the one-workgroup-
 * per-(row, head) kernel; otherwise the key-chunk kernels run: beam 1 and ks > 8 the VALU form,
 * beam > 1 with ks <= 8 the MFMA form, in the instantiation the decoder's launcher picks at T
 * (legacy 0: ceil(ceil(T / 8) / 32) keys per lane, ceil(ceil(T / 8) / 64) key tiles per wave) or the
 * full-width one that serves T > 1280 (legacy 2: 6 keys per lane, 3 tiles per wave).  The device
 * copies of K and V are followed by 64 NaN keys, so a load past a window's T keys shows in `out`.
 * The context's arrival tickets it used are zero on return. */
int osw_debug_dec_xattn(osw_ctx* ctx, const float* q_slabs, int32_t ks, const float* bias, const void* K,
                        const void* V, int32_t rows, int32_t beam, int32_t legacy, float* out);
/* The same launch with a window map (osw_decode_window_list's form): K and V fp16
 * [kv_windows][H][T][64], kv_windows <= max_batch, and row group w (rows w * beam .. + beam - 1)
 * attends window window_map[w]; window_map holds rows / beam distinct indices below kv_windows (else
 * OSW_EINVAL).  Equals osw_debug_dec_xattn over K[window_map], V[window_map] bit for bit. */
int osw_debug_dec_xattn_windows(osw_ctx* ctx, const float* q_slabs, int32_t ks, const float* bias, const void* K,
                                const void* V, int32_t kv_windows, const int32_t* window_map, int32_t rows,
                                int32_t beam, int32_t legacy, float* out);
/* Decoder self-attention step of `rows` rows with the context's H, D and ctx = n_text_ctx:
 * qkv_slabs fp32 [ks][rows][3 D] are the qkv projection's split-K partials, bias [3 D]; kcache and
 * vcache fp16 [rows][H][ctx][64] are read, get fp16(k) and fp16(v) of row r written at position
 * pos[r] (pos_per_row != 0) or pos[0], and are copied back; the row attends positions 0 .. pos.
 * ancestry [rows][ctx] (beam search; NULL: every key is the row's own): key p < pos of row r is read
 * from row ancestry[r][p]'s cache, rows = windows x group.  out fp32 [rows][D] = hi + lo.  The form
 * is the production launcher's: <= 8 rows issue V with K, more rows V late; ancestry gathers. */
int osw_debug_dec_self_attn(osw_ctx* ctx, const float* qkv_slabs, int32_t ks, const float* bias, void* kcache,
                            void* vcache, int32_t rows, const int32_t* pos, int32_t pos_per_row,
                            const int32_t* ancestry, int32_t group, float* out);

/* ---- the decoder's linear path, one production launcher per call on host data
 * (parity tests: tests/test_gpu_dec_gemm.py; references and bounds: tests/dec_gemm_ref.py) ----
 * Like the attention calls above: temporary device buffers, one launch through the launcher the
 * decoder step uses, the result copied back.  Every precondition a launcher or kernel relies on is
 * checked first and reported as an error (K and K / ksplit multiples of 128 for the skinny kernel,
 * D % 4 == 0 and D <= 1280, the row limits of the fused prologues, the lo operand beyond 64 rows,
 * the capacity of `out`).  `out` receives out_floats floats: the result first, the rest a guard
 * band that the call fills with 0xff bytes before the launch, as it does the result's own floats,
 * so an unwritten element and a store past the result both show.  *ks_out: the split count used.
 *
 * C = (A_hi + A_lo) · Wᵀ: A_hi, A_lo fp16 [M][K] (A_lo NULL: one fp16 operand, M <= 64), W fp16
 * [N][K]; on the device the lo rows sit M rows after the hi rows with lda = K.  use_wf: W's
 * fragment-major copy is packed (launch_frag_pack) and passed as GemmArgs::Wf.
 *   form 0: launch_gemm_skinny_partial -> slabs [ks][M][N]
 *   form 1: launch_gemm_tiled_partial with tiled_ksplit(M, N, K) -> slabs [ks][M][N]
 *   form 2: the vocabulary projection as decoder_step runs it (the skinny kernel, split with
 *           splitk_reduce_kernel or unsplit, or the wide kernel) -> [M][N], ldc = N */
int osw_debug_dec_gemm(osw_ctx* ctx, int32_t form, int32_t M, int32_t N, int32_t K, const void* A_hi,
                       const void* A_lo, const void* W, int32_t use_wf, float* out, int64_t out_floats,
                       int32_t* ks_out);
/* osw_debug_dec_gemm's forms 0, 1 and 2 on int8 weights: W given as q int8 [N][K] plus mult fp32
 * [N], A_hi and A_lo both required (int8 weights serve hi/lo rows), K a multiple of 64.  The
 * device holds what osw_set_weight_quant leaves there.  use_q8_stream != 0: the skinny kernel
 * streams the int8 fragments (GemmArgs::Wq); 0: the fp16(q) copy (row-major and fragment-major)
 * with the multipliers, through the same launcher: the same bits.  The wide and tiled kernels
 * read the row-major fp16(q) either way.  Forms 3 and 4 pass the same operands to the GELU-tail
 * and attention-tail launchers, which refuse int8 weights before launching.  Same guard band,
 * precondition checks and *ks_out as osw_debug_dec_gemm. */
int osw_debug_dec_gemm_quant(osw_ctx* ctx, int32_t form, int32_t M, int32_t N, int32_t K, const void* A_hi,
                          const void* A_lo, const int8_t* q, const float* mult, int32_t use_q8_stream,
                          float* out, int64_t out_floats, int32_t* ks_out);
/* Per-launch HIP-event time of launch_gemm_skinny_partial on one decoder projection shape (M <= 64
 * hi/lo rows), float16 weights and int8 weights alternating in one call (tools/q8_bench.py): `warm`
 * untimed launches of each, then `launches` timed ones, us_f16[i] / us_q8[i] microseconds.  Each
 * stream exists in `copies` replicas walked round robin, so the weights come from where a decoder
 * step finds them rather than from the L2 the previous launch filled. */
int osw_debug_dec_gemm_time(osw_ctx* ctx, int32_t M, int32_t N, int32_t K, const void* A_hi, const void* A_lo,
                            const int8_t* q, const float* mult, int32_t copies, int32_t warm, int32_t launches,
                            float* us_f16, float* us_q8);
/* While profiling (osw_set_profiling 2: eager decoder steps): the summed HIP-event time and the
 * launch count of the fused (one-row) step's logits GEMM, which at batch 1 greedy carries the
 * selection in its epilogue, since profiling was last set. */
int osw_debug_logits_profile(osw_ctx* ctx, double* ms, int64_t* launches);
/* Residual update + LayerNorm of `rows` rows of width D: x' = x + bias + Σ slabs (slabs fp32
 * [ks][rows][D], bias [D] or NULL), or with slabs == NULL the embedding entry x' = tok_emb[tok[r]]
 * + pos_emb[pos] (tok_emb fp16 [V][D], pos_emb fp32 [ctx][D], tok [rows], pos [rows] when pos_row
 * else [1]; ids are clamped into [0, V), positions to ctx - 1); y = LayerNorm(x') * gain + shift.
 *   fused == 0: launch_dec_resid_ln.  x_out [rows][D] = x', y_hi / y_lo fp16 [rows][D] = the pair.
 *   fused != 0 (rows <= 1): launch_gemm_skinny_pro(PRO_RESLN) with W fp16 [N][D]: x_out = x' (written
 *     to a second buffer, as the fused step ping-pongs), x is read back from the device and must be
 *     unchanged, and out = the GEMM's split-K slabs [ks][rows][N], or with direct != 0 C [rows][N]. */
int osw_debug_dec_resln(osw_ctx* ctx, int32_t fused, int32_t direct, int32_t rows, int32_t D, const float* slabs,
                        int32_t ks, const float* bias, float* x, const float* gain, const float* shift,
                        const void* tok_emb, const float* pos_emb, const int32_t* tok, const int32_t* pos,
                        int32_t ctx_len, int32_t V, int32_t pos_row, const void* W, int32_t N, int32_t use_wf,
                        float* x_out, void* y_hi, void* y_lo, float* out, int64_t out_floats, int32_t* ks_out);
/* GELU reduce y = gelu(bias + Σ slabs), slabs fp32 [ks][M][K4], bias [K4].
 *   fused == 0: launch_dec_reduce_gelu -> the fp16 pair y_hi / y_lo [M][K4].
 *   fused != 0 (M <= 8, K4 / ksplit <= 256): launch_gemm_skinny_pro(PRO_GELU) with W fp16 [N][K4]
 *     -> out = its split-K slabs [ks][M][N]. */
int osw_debug_dec_gelu(osw_ctx* ctx, int32_t fused, int32_t M, int32_t K4, const float* slabs, int32_t ks,
                       const float* bias, const void* W, int32_t N, int32_t use_wf, void* y_hi, void* y_lo,
                       float* out, int64_t out_floats, int32_t* ks_out);

/* ---- the encoder's tiled GEMM and LayerNorm, one launch per call on host data
 * (parity tests: tests/test_gpu_enc_gemm.py; references and bounds: tests/enc_gemm_ref.py) ----
 * One launch of the tiled GEMM family with the full argument set of the encoder's launches: grouped
 * (overlapping) A rows, grouped C rows at an offset into their buffer, bias, the positional table,
 * any of the six epilogues and the head-major scatter with slot redirection.  Row m of A is at
 * A + (m / a_grp_rows) * a_grp_stride + (m % a_grp_rows) * lda and reads K elements; row m of C at
 * C + c_offset + (m / c_grp_rows) * c_grp_stride + (m % c_grp_rows) * ldc (elements of the
 * epilogue's type: fp16 for OSW_EPI_F16 / _F16_GELU / _HEADS, fp32 for the others).  OSW_EPI_HEADS
 * writes fp16 [N / (64 heads_H)][heads_nb][heads_H][heads_T][64] at C + c_offset, row m = window *
 * heads_T + t going to window heads_slot[window] (NULL: the window itself).
 * The whole C buffer (c_bytes) is uploaded before the launch and downloaded after it, so the caller
 * sees every byte the kernel did or did not touch (a canary; the residual of OSW_EPI_F32_RESID).
 * variant: 0 the production chooser (with the context's current CU sharing), 1 the 128 tile double
 * buffered, 2 the 256 tile, 4 the 8-phase 256 tile, 6 the 64 ring, 7 the 64 tile double buffered,
 * 11 the 128 ring, 16 the half-width 256 x 128 tile, 20 the 8-phase tile with the fp32 epilogues'
 * other residual prefetch depth (the kernels OSW_GEMM_RESID_PF selects), 21 the 8-phase tile on one workgroup
 * with the next tile's first K-tile staged under each epilogue (N % 8 == 0).  hi/lo operands, split-K and fragment-major
 * weights are not offered.
 * Every precondition is checked before anything is launched (OSW_EINVAL): K % 64; lda and
 * a_grp_stride multiples of 8; every A row inside a_count elements; every C row, or the head-major
 * extent, inside c_bytes; C rows and groups that do not overlap (ldc >= N, c_grp_stride >=
 * c_grp_rows * ldc); N, ldc and c_grp_stride multiples of 8 for every epilogue but OSW_EPI_F32
 * (run_gemm's rule) and of 4 for OSW_EPI_F32 (the 256-row tiles store it in 16-B chunks too), c_offset
 * a multiple of 8 (fp16) or 4 (fp32); pos [c_grp_rows][N] for OSW_EPI_F32_GELU_POS;
 * N % (64 heads_H) == 0, M % heads_T == 0 and distinct slots < heads_nb for OSW_EPI_HEADS; variant
 * 11 and 16 only where launch_gemm_variant would run the kernel they name. */
#define OSW_EPI_F16 0
#define OSW_EPI_F16_GELU 1
#define OSW_EPI_F32_RESID 2
#define OSW_EPI_F32_GELU_POS 3
#define OSW_EPI_F32 4
#define OSW_EPI_HEADS 5
typedef struct osw_enc_gemm_desc {
    int32_t M, N, K, variant, epi;
    int32_t heads_T, heads_H, heads_nb;  /* OSW_EPI_HEADS */
    int64_t lda, a_grp_rows, a_grp_stride;
    int64_t a_count;                     /* fp16 elements of A */
    int64_t ldc, c_grp_rows, c_grp_stride, c_offset;
    int64_t c_bytes;                     /* bytes of C */
    int64_t pos_count;                   /* floats of pos */
    const void* A;                       /* fp16 [a_count] */
    const void* W;                       /* fp16 [N][K] */
    const float* bias;                   /* [N] or NULL */
    const float* pos;                    /* [c_grp_rows][N], OSW_EPI_F32_GELU_POS */
    const int32_t* heads_slot;           /* [M / heads_T] or NULL */
    void* C;                             /* in/out */
} osw_enc_gemm_desc;
int osw_debug_enc_gemm(osw_ctx* ctx, const osw_enc_gemm_desc* desc);
/* launch_layernorm on host data: y[m] = fp16(LayerNorm(x[m]) * gain + shift) for m < M, x fp32
 * [M][D], y fp16 [M_alloc][D] in/out (uploaded first: rows M .. M_alloc-1 must come back unchanged).
 * OSW_EINVAL for a width launch_layernorm has no kernel for. */
int osw_debug_enc_layernorm(osw_ctx* ctx, int32_t M, int32_t M_alloc, int32_t D, const float* x, const float* gain,
                            const float* shift, void* y);

/* ---- the log-mel front end's intermediate values (parity tests: tests/test_gpu_mel.py) ----
 * The raw fp32 log10 mel of clip `clip` of the last osw_log_mel, time-major [n_frames][n_mels], as
 * mel_logmel_kernel stored it (before the max - 8 clamp and the (x + 4) / 4 scaling of osw_get_mel),
 * and in *clip_max the clip's maximum as the kernels read it (decoded from its ordered-int form). */
int osw_debug_get_logmel(osw_ctx* ctx, int32_t clip, float* out, int64_t out_floats, float* clip_max);
/* mel_window_kernel alone on n <= max_batch windows of the resident log-mel: the windows are checked
 * as osw_encode_windows checks them (OSW_EINVAL with the same message, before any launch), then
 * out_halfs receives the conv stem's operand X1 [n][2 * n_audio_ctx + 2][C1] ([n][3002][C1] at the default) as fp16 bits, C1 = n_mels rounded up
 * to a multiple of 64: row 1 + t is frame seek + t, normalised; rows 0 and 3001, rows past the
 * segment and columns past n_mels are zero.  out_count: the buffer's size in fp16 elements. */
int osw_debug_mel_windows(osw_ctx* ctx, const osw_window* windows, int32_t n, void* out_halfs, int64_t out_count);

/* Test hook for the concurrency contract: holds a stream capture open on the context's
 * stream for hold_ms (under the same locks as a decode-graph capture) and fails if it was
 * invalidated meanwhile.  Other threads' calls run during the hold. */
int osw_debug_hold_capture(osw_ctx* ctx, int32_t hold_ms);

/* 0 off; 1 per-stage HIP-event timers (decode steps stay in their hipGraph, so only
 * mel / encoder stages are timed); 2 also launches the decode steps eagerly so the
 * cross-attention timers see them.  Resets the counters. */
int osw_set_profiling(osw_ctx* ctx, int32_t enable);
int osw_get_profile(osw_ctx* ctx, osw_profile* out);
/* Device stream used by the context (hipStream_t as void*). */
void* osw_stream(osw_ctx* ctx);

/* ---- audio ingest (context-free: a per-device stream and scratch inside the library).
 * Host buffers in and out; the arithmetic runs on `device` and is bit-identical to the
 * reference's numpy / scipy code (csrc/ingest.hip).
 *
 * *out_mean = np.mean(np.square(mono)) in float32 with numpy's reduction order, where
 * mono = channel mean of pcm / 32768 (wav_bytes_to_float32_mono, preprocessing.py:9-20).
 * The caller derives the gain from it exactly as normalize_gain does (sqrt, log10,
 * 10 ** (dB / 20) on float32 scalars: preprocessing.py:36-41) and then calls
 * osw_ingest_apply_gain (apply_gain = 0 when normalize_gain returns early). */
int osw_ingest_mean_square(int32_t device, const int16_t* pcm, int64_t n_frames, int32_t channels, float* out_mean);
/* out[n_frames] = int16(clip(clip(mono * gain, -1, 1), -1, 1) * 32767) (truncating) */
int osw_ingest_apply_gain(int32_t device, const int16_t* pcm, int64_t n_frames, int32_t channels, int32_t apply_gain,
                          float gain, int16_t* out);
/* out[n_out] = resample_poly(pcm, up, down, padtype="line") clipped and truncated to
 * int16; h = the float32 filter resample_poly designs (firwin(2*10*max(up,down)+1,
 * 1/max(up,down), kaiser 5.0) cast to float32, times up), n_h odd; up/down already
 * divided by their gcd; n_in >= 2; n_out = ceil(n_in * up / down). */
int osw_ingest_resample(int32_t device, const int16_t* pcm, int64_t n_in, int32_t up, int32_t down, const float* h,
                        int32_t n_h, int16_t* out, int64_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* OSW_H */
