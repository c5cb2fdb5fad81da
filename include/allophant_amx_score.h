/* CTC forward-backward scoring entry points of liballophant_amx (companion of allophant_amx_align.h, same library, same ABI
 * version). */
#ifndef ALLOPHANT_AMX_SCORE_H
#define ALLOPHANT_AMX_SCORE_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How probable a known label sequence is given per-frame log-probabilities, and how sure the model is of each of its
 * symbols: the sum over every CTC path (forward-backward), where amx_ctc_align finds the one best path.  Symbols added to
 * ABI 6 without a struct change (detect them with dlsym).  Rows, targets, blank and the malformed-row rules are those of
 * allophant_amx_align.h: a row is one emission matrix lp[T][C] (fp32, T = the row's frame length), its targets y[0..L) and a
 * blank; S = 2L + 1; state i has label `blank` for even i and y[i / 2] for odd i; e[t][i] = lp[t][label(i)].  All
 * arithmetic is fp32 and -inf is an ordinary value: lse of a set is -inf when every member is -inf (never NaN from
 * -inf - -inf), else m + log(sum of exp(x - m)) with m the set's maximum.
 *
 *   a[0][0] = e[0][0];  a[0][1] = e[0][1] (L > 0);  every other a[0][i] = -inf
 *   a[t][i] = lse(a[t-1][i], a[t-1][i-1] (i >= 1), a[t-1][i-2] (i odd, i >= 3, y[i/2] != y[i/2 - 1])) + e[t][i]
 *   ll      = lse(a[T-1][S-1], a[T-1][S-2] (S > 1))
 *   b[T-1][S-1] = e[T-1][S-1];  b[T-1][S-2] = e[T-1][S-2] (S > 1);  every other b[T-1][i] = -inf
 *   b[t][i] = lse(b[t+1][i], b[t+1][i+1] (i + 1 < S), b[t+1][i+2] (i odd, i + 2 < S, y[i/2 + 1] != y[i/2])) + e[t][i]
 *   g[t][i] = exp(a[t][i] + b[t][i] - e[t][i] - ll), and 0 where a[t][i] or b[t][i] is -inf
 *
 * `candidates` G >= 1 scores G target rows per utterance (an n-best list): row r reads the emissions of utterance
 * (r / G) % N, and target_offsets has rows + 1 entries.
 *
 * Outputs, all DEVICE pointers, per row r (target l owns state 2l + 1):
 *   log_likelihood float [rows]: ll
 *   occupancy      float [rows, max_target]: sum over t of g[t][2l+1], the expected number of frames of target l
 *   position_sums  float [rows, max_target]: sum over t of t * g[t][2l+1] (divided by occupancy: the expected frame)
 *   score_sums     float [rows, max_target]: sum over t of g[t][2l+1] * e[t][2l+1], a term whose g is 0 counting as 0
 *   posteriors     float [rows, T, 2 max_target + 1], or NULL: g[t][i] for t < the row's frame length and i < S; every other
 *                  entry is untouched
 *   status         int32 [rows]:  0 scored (a row of no frames and no targets: ll 0);
 *                                -1 no path (ll == -inf, or no frames for L > 0): the row writes log_likelihood = -inf and
 *                                   its status, nothing else;
 *                                -2 malformed row, as in allophant_amx_align.h: the row writes its status only, and nothing
 *                                   out of range is read for it
 * Entries of the three per-target outputs at and past the row's L are untouched.  The three sums are fp32, added to 0 one
 * frame at a time in the order of the backward sweep (the last frame first) by the one lane that owns the state: there are
 * no floating-point atomics and results are bitwise reproducible run to run.  With NaN emissions the values are
 * unspecified, but every index read or written stays in range and the kernel terminates.
 *
 * Limits: 2 <= C, 0 <= blank < C, 1 <= candidates, 0 <= max_target <= AMX_SCORE_MAX_TARGET, rows * T < 2^31; AMX_EINVAL
 * otherwise, with amx_last_error naming the cause, before any device work.
 *
 * The caller supplies the workspace, which holds the forward values a[t][i]: one fp32 per (row, frame, state), the states
 * padded to whole strips of 64:
 *     bytes = rows * T * ceil((2 max_target + 1) / 64) * 64 * 4
 * Stream-ordered on `stream`: no allocation, no host synchronisation beyond what amx_ctc_align does. */
#define AMX_SCORE_MAX_TARGET 4095 /* 8191 states, as AMX_ALIGN_MAX_TARGET: a row that can be aligned can be scored */

/* Pure host function; AMX_EINVAL when a limit is broken or the size is not representable in size_t. */
int amx_ctc_score_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes);

/* One fp32 emission tensor [N, T, C] on `device` with element strides (stride_n, stride_t, 1), read in place; rows are
 * n * candidates + g (N * candidates of them).  frame_lengths int32 [N], target_offsets int32 [rows + 1] and target_ids
 * int32 [target_offsets[rows]] are DEVICE pointers.  N == 0 returns AMX_OK. */
int amx_ctc_score_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                            int N, int64_t T, int C, int blank_index, int candidates, const int32_t* target_offsets,
                            const int32_t* target_ids, int64_t max_target, void* workspace, size_t workspace_bytes,
                            float* log_likelihood, float* occupancy, float* position_sums, float* score_sums, float* posteriors,
                            int32_t* status, void* stream);

/* Every output of the last amx_forward, like amx_ctc_align: `out` is the device output buffer for a batch of geometry
 * (N, L) under the current inventory, `frame_lengths` the int64 [N] HOST `Predictions.lengths`; rows are
 * (o * N + n) * candidates + g in the order of amx_output_layout (O outputs), blank 0; target_offsets is DEVICE int32
 * [O * N * candidates + 1]. */
int amx_ctc_score(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, int candidates,
                  const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                  size_t workspace_bytes, float* log_likelihood, float* occupancy, float* position_sums, float* score_sums,
                  float* posteriors, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_SCORE_H */
