/* CTC beam-search entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_BEAM_H
#define ALLOPHANT_AMX_BEAM_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `BeamCTCDecoder.__call__` (predictions.py:210-235): torchaudio's flashlight `ctc_decoder` as the reference builds it --
 * lexicon-free, no LM, blank = silence, log_add = True, beam_threshold 50, every token considered per frame -- decoded on
 * the device.  Symbols added to ABI 6 without a struct change (detect them with dlsym).  The semantics are restated in
 * DESIGN 9; scores are fp64 sums of the emissions as given (or of their exponentials under AMX_BEAM_EXP_EMISSIONS, which is
 * what the reference passes: `log_emissions.exp()`).  An emission of -inf is an ordinary value (under
 * AMX_BEAM_EXP_EMISSIONS it adds exactly 0); a frame with no finite emission, and NaN, are outside the contract.  Equal
 * scores resolve by one stated rule (candidates in (kind, beam slot, class) order, token lists by the value as
 * added and then the lower class), so the result is a function of the inputs alone.
 *
 * Limits: 1 <= beam_width <= 64, 1 <= n_best <= beam_width, 2 <= C <= 65535, 0 <= blank < C; AMX_EINVAL otherwise.
 *
 * The caller supplies the workspace: amx_beam_ctc_workspace gives its size for `rows` rows of T frames (rows x T x
 * beam_width x 4 bytes, one backpointer per frame and beam slot).  A row is one (output, utterance) pair.
 * Outputs, all DEVICE pointers, per row r:
 *   tokens, timesteps  int64 [rows, n_best, T]: hypothesis h holds counts[r, h] entries (timesteps 1-based)
 *   counts             int32 [rows, n_best]
 *   scores             fp64  [rows, n_best], descending; -inf past hyp_counts[r]
 *   hyp_counts         int32 [rows]: hypotheses found (<= n_best; 1 for an empty utterance: no tokens, score 0)
 * Stream-ordered on `stream`: no allocation, no host synchronisation beyond what amx_greedy_ctc does. */
#define AMX_BEAM_EXP_EMISSIONS 1u /* exponentiate every emission as it is read (fp32 exp), like the reference's decoder call */

int amx_beam_ctc_workspace(int beam_width, int64_t rows, int64_t T, size_t* bytes);

/* Every output of the last amx_forward, like amx_greedy_ctc: `out` is the device output buffer for a batch of geometry
 * (N, L) under the current inventory, `frame_lengths` the int64 [N] HOST `Predictions.lengths`; rows are o * N + n in the
 * order of amx_output_layout, blank 0. */
int amx_beam_ctc(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, int beam_width, int n_best,
                 uint32_t flags, void* workspace, size_t workspace_bytes, int64_t* tokens, int64_t* timesteps, int32_t* counts,
                 double* scores, int32_t* hyp_counts, void* stream);

/* One fp32 emission tensor [N, T, C] on `device` with element strides (stride_n, stride_t, 1), read in place (e.g. the
 * transposed view of a [T, N, C] output), with int32 [N] DEVICE frame lengths; rows are the N utterances. */
int amx_beam_ctc_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                           int N, int64_t T, int C, int blank_index, int beam_width, int n_best, uint32_t flags, void* workspace,
                           size_t workspace_bytes, int64_t* tokens, int64_t* timesteps, int32_t* counts, double* scores,
                           int32_t* hyp_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_BEAM_H */
