/* CTC beam search with a phonotactic language model (companion of allophant_amx_beam.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_BEAM_LM_H
#define ALLOPHANT_AMX_BEAM_LM_H
#include "allophant_amx_beam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The decoder of amx_beam_ctc_emissions with shallow fusion of a token-level bigram: flashlight's LexiconFreeDecoder with a
 * language model in place of ZeroLM.  Symbols added to ABI 7 without a struct change (detect them with dlsym).  The
 * semantics are restated in DESIGN 9.
 *
 * A language model is a dense fp32 table lm[C + 1, C + 1] of natural-log scores: row p is the previous token of the prefix
 * (row C: begin, the empty prefix), column n the next token (column C: end).  The blank's row and column are never read.
 * Entries are finite or -inf.  A (state, token) pair that emits a new token n after the prefix P scores
 *     s + e[t, n] + (lm_weight * lm[last(P), n] + token_score)                                   (fp64)
 * and an -inf entry forbids the transition at every weight, 0 included.  Blank and repeat candidates add nothing.  The
 * frame threshold of 50 is taken against the best generated candidate with the language-model term included.  At the end
 * every state adds lm_weight * lm[last(P), C]; an -inf entry there drops the state, and a row with no state left has
 * hyp_counts 0.  `scores` are the fused totals.  Equal scores resolve by the rule of amx_beam_ctc_emissions, each
 * prefix's token list being cut by (emission as added + language-model term, then the lower class).
 *
 * `lm` is a DEVICE stack [n_lm, C + 1, C + 1], `lm_index` a DEVICE int32 [N]: the table of each row, or -1 for a row that
 * runs without one (no term, no end term: amx_beam_ctc_emissions bit for bit, as is every row at lm_weight 0 and
 * token_score 0 under a table without -inf).  A row whose index is neither -1 nor in [0, n_lm) reads no table and gets
 * hyp_counts 0.
 *
 * Limits: those of amx_beam_ctc_emissions, and 2 <= C <= 4095, n_lm >= 1, lm_weight and token_score finite; AMX_EINVAL
 * otherwise, before any device work.  Workspace, outputs, layouts and stream ordering are those of amx_beam_ctc_emissions. */
#define AMX_BEAM_LM_MAX_CLASSES 4095

int amx_beam_ctc_lm_workspace(int beam_width, int64_t rows, int64_t T, size_t* bytes);

int amx_beam_ctc_lm_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                              int N, int64_t T, int C, int blank_index, int beam_width, int n_best, uint32_t flags, const float* lm,
                              int n_lm, const int32_t* lm_index, double lm_weight, double token_score, void* workspace,
                              size_t workspace_bytes, int64_t* tokens, int64_t* timesteps, int32_t* counts, double* scores,
                              int32_t* hyp_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_BEAM_LM_H */
