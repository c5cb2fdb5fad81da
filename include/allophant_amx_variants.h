/* CTC scoring of every one-edit variant of a transcript: entry points of liballophant_amx (companion of
 * allophant_amx_score.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_VARIANTS_H
#define ALLOPHANT_AMX_VARIANTS_H
#include "allophant_amx_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where the model disagrees with a transcript, and with what alternative: the log-likelihood (the sum over every CTC path)
 * of the transcript with one symbol substituted by each class, with one symbol deleted, and with each class inserted into
 * each gap.  Symbols added to ABI 7 without a struct change (detect them with dlsym).  Rows, targets, blank, the
 * malformed-row rules, lse, a, b and ll are those of allophant_amx_score.h, extended by two virtual frames:
 *
 *   a[-1][0] = 0 and every other a[-1][i] = -inf;  b[T][S-1] = 0 and every other b[T][i] = -inf;
 *   b[t][i] = -inf for i >= S, a[t][i] = -inf for i < 0
 *
 * which reproduce that header's first and last rows exactly.  All arithmetic is fp32 and -inf is an ordinary value; T is
 * the row's frame length.  A term in parentheses belongs to the lse only under its condition.  An lse of three may be formed
 * as an lse of two of them and the third, and an lse over the frames as a running maximum with a sum of exp(x - maximum).
 *
 * Substitution of y[l] by the class c != blank, 0 <= l < L:
 *   v[-1] = -inf
 *   v[t]  = lse(v[t-1], a[t-1][2l], a[t-1][2l-1] (l >= 1 and c != y[l-1])) + lp[t][c]
 *   sub[l][c] = lse over t in [0, T) of  v[t] + lse(b[t+1][2l+2], b[t+1][2l+3] (l + 1 < L and c != y[l+1]))
 * Deletion of y[l], stored in the blank column:
 *   sub[l][blank] = lse over t in [-1, T) of
 *         lse(a[t][2l], a[t][2l-1] (l >= 1 and (l + 1 == L or y[l-1] != y[l+1])))  +  x[t+1]
 *   x[t+1] = b[t+1][2l+3] when l + 1 < L;  when l + 1 == L: 0 for t + 1 == T, else -inf
 * Insertion of the class c != blank into gap p, 0 <= p <= L (the gap before y[p]; p == L is the end):
 *   u[-1] = w[-1] = -inf
 *   u[t] = lse(u[t-1], a[t-1][2p], a[t-1][2p-1] (p >= 1 and c != y[p-1])) + lp[t][c]
 *   w[t] = lse(w[t-1], u[t-1]) + lp[t][blank]
 *   ins[p][c] = lse over t in [0, T) of  lse(w[t], u[t] (c != y[p])) + b[t+1][2p+1]      (p < L)
 *   ins[L][c] = lse(u[T-1], w[T-1])
 *   ins[p][blank] = ll                                                                    (nothing inserted)
 * sub[l][y[l]] is computed like every other column and equals ll up to rounding, so a row sub[l][.] is the unnormalised
 * log-posterior over "what stands at position l, or nothing", and a row ins[p][.] the same over "what stands in gap p, or
 * nothing".
 *
 * Outputs, all DEVICE pointers, per row r:
 *   log_likelihood float [rows]: ll
 *   substitutions  float [rows, max_target, C]: sub[l][c]
 *   insertions     float [rows, max_target + 1, C]: ins[p][c]
 *   status         int32 [rows]:  0 every cell of the row's L substitution rows and L + 1 insertion rows is written; any of
 *                                   them may be -inf, ll included (a transcript with no path can have feasible deletions).  A
 *                                   row of no frames and no targets: ll = 0, ins[0][blank] = 0, every other ins[0][c] = -inf;
 *                                -1 no frames for L > 0: the row writes log_likelihood = -inf and its status, nothing else;
 *                                -2 malformed row, as in allophant_amx_align.h: the row writes its status only, and nothing
 *                                   out of range is read for it
 * Entries at and past the row's L (L + 1 for the insertions) are untouched.  Each cell is accumulated by one lane over the
 * frames in ascending order: there are no floating-point atomics and results are bitwise reproducible run to run.  With
 * NaN emissions the values are unspecified, but every index read or written stays in range and the kernel terminates.
 *
 * Limits: 2 <= C <= AMX_VARIANTS_MAX_CLASSES, 0 <= blank < C, 0 <= max_target <= AMX_VARIANTS_MAX_TARGET, rows * T < 2^31;
 * AMX_EINVAL otherwise, with amx_last_error naming the cause, before any device work.  Output offsets are 64-bit.
 *
 * The caller supplies the workspace, which holds a[t][i] and then b[t][i]: two fp32 per (row, frame, state), the states
 * padded to whole strips of 64:
 *     bytes = 2 * rows * T * ceil((2 max_target + 1) / 64) * 64 * 4
 * Stream-ordered on `stream`: no allocation, no host synchronisation. */
#define AMX_VARIANTS_MAX_TARGET 4095 /* as AMX_SCORE_MAX_TARGET: a row that can be scored can be varied */
#define AMX_VARIANTS_MAX_CLASSES 65535

/* Pure host function; AMX_EINVAL when a limit is broken or the size is not representable in size_t. */
int amx_ctc_variants_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes);

/* One fp32 emission tensor [N, T, C] on `device` with element strides (stride_n, stride_t, 1), read in place; one row per
 * utterance.  frame_lengths int32 [N], target_offsets int32 [N + 1] and target_ids int32 [target_offsets[N]] are DEVICE
 * pointers.  N == 0 returns AMX_OK. */
int amx_ctc_variants_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                               int N, int64_t T, int C, int blank_index, const int32_t* target_offsets, const int32_t* target_ids,
                               int64_t max_target, void* workspace, size_t workspace_bytes, float* log_likelihood,
                               float* substitutions, float* insertions, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_VARIANTS_H */
