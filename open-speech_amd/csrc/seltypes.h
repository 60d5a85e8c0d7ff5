// The token selection's plain-data types, shared by the kernels (decode.h) and the host-only
// decode plan (plan.h).  No HIP header and no device helper: a host program can include it.
#pragma once

namespace osw {

// Per decoder row (a window, or one beam hypothesis of a window).  Lives in device
// memory so a step needs no host round trip.
struct SelState {
    int n_sampled, last, penult, last_ts, done, lang;
    float sum_lp, nsp;  // greedy: Σ log-prob of the picks; beam: the hypothesis' cumulative score
    int plen;           // this row's prompt length (0: SelParams::prompt_len; decode sessions admit
                        // windows with different previous-text prefixes)
    int n_lp;           // confidences on: cumulative log-probs recorded for this row (SelParams::lp_hist)
};

struct SelParams {
    int prompt_len;        // P: positions 0..P-1 are prompt (rows whose SelState::plen is 0)
    int sot_pos;           // position of <|startoftranscript|> in the prompt
    int lang_pos;          // prompt position holding the language token (-1 placeholder => detect)
    int max_length;
    int pstride;           // ints per row of the prompt buffer (>= every row's prompt length)
    int tail;              // prompt positions from <|startoftranscript|> to the end (3, or 4 with no-timestamps;
                           // English-only models: 1, or 2 with no-timestamps)
    int sot_last;          // 1: <|startoftranscript|> ends every row's prompt (English-only with timestamps), so
                           // the first sampled step also records the no-speech prob (select.h sot_sample_step)
    int V, eot, no_speech, no_ts, tb, blank, first_lang, n_langs;
    int suppress_blank, with_ts, max_init_ts;
    int beam;              // hypotheses per window (1 = greedy)
    int num_hyp, max_cand; // beam stop rule: num_hypotheses, round(beam * patience)
    float length_penalty;
    float inv_temp;        // sampling (temperature > 0): 1 / temperature, else 0
    const unsigned long long* seed;  // device word: the draw seed (not in the graph key, so a new
                                     // seed per call replays the captured decode graph)
    const int* budget;     // per decoder row: force <|endoftext|> after this many sampled tokens (<= 0: none);
                           // nullptr: no budgets (osw_decode_opts::token_budget, length-controlled benches)
    int pos_row;           // 1: row r's step counter is pos[r] (row refill, sessions), 0: one shared counter
    // Confidences (osw_set_confidences); every pointer nullptr when off, and nothing is stored.
    float* lp_hist;        // [rows][lp_stride]: the row's cumulative log-prob after its i-th sampled step (the
                           // <|endoftext|> step included).  Beam rows: written once at [physical row][i]; a
                           // hypothesis' entry i lives in the row its ancestry names at position plen + i
    float* best_lp;        // beam: [windows][lp_stride], the best finished hypothesis' history (beside best_tok)
    float* lang_probs;     // [windows][n_langs]: softmax over the language tokens' raw <|startoftranscript|> logits
    int lp_stride;         // floats per row of lp_hist / best_lp (n_text_ctx)
    int lp_group;          // decoder rows per window (beam_size or best_of): row w * lp_group writes lang_probs[w]
    // Retry sessions (osw_session_retries); both nullptr otherwise.  A window slot whose first row
    // has row_inv_temp > 0 samples: its rows with row_inv_temp > 0 draw at that 1 / temperature
    // with their row_seed, its other rows are parked.  A slot whose first row holds 0 decodes in
    // the session's temperature-0 mode on its first `beam` rows.
    const float* row_inv_temp;             // [rows]
    const unsigned long long* row_seed;    // [rows]
};

// Per window in beam mode: finished-hypothesis bookkeeping (the best one's tokens
// are copied to a per-window buffer when it improves).
struct BeamWin {
    int n_hyp, best_len, done;
    int best_nlp;  // confidences on: entries of SelParams::best_lp (best_len, + 1 when it ended with <|endoftext|>)
    float best_norm, best_raw;
};

constexpr int MAX_BEAM = 8;
constexpr int SEL_SPLIT = 16;  // vocabulary slices per row in the selection kernels
constexpr int LANG_CAP = 128;  // language tokens a window's language_probs row holds (Whisper: 99 or 100)

// History rules (osw_decode_opts::repetition_penalty / no_repeat_ngram_size): penalty <= 0 or == 1
// and ngram <= 0 are "off"; a caller with both off does not launch them (launch_history_rules).
inline bool history_rules_on(float penalty, int ngram) { return (penalty > 0.f && penalty != 1.f) || ngram > 0; }

}  // namespace osw
