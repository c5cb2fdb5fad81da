/* CTC forced-alignment entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_ALIGN_H
#define ALLOPHANT_AMX_ALIGN_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The best CTC path (Viterbi) of a known label sequence through per-frame log-probabilities, on the device.  Symbols
 * added to ABI 6 without a struct change (detect them with dlsym).  A row is one emission matrix lp[T][C] (fp32, T = the
 * row's frame length), its targets y[0..L) and a blank.  With S = 2L + 1, state i has label `blank` for even i and y[i / 2]
 * for odd i; all arithmetic is fp32 and -inf is an ordinary value:
 *
 *   a[0][0] = lp[0][blank];  a[0][1] = lp[0][y[0]] (if L > 0);  every other a[0][i] = -inf
 *   for t >= 1, every i:
 *       x0 = a[t-1][i]
 *       x1 = a[t-1][i-1]        (i >= 1, else -inf)
 *       x2 = a[t-1][i-2]        (only if i is odd, i >= 3 and y[i/2] != y[i/2 - 1]; else -inf)
 *       r, m = x0, 0;  if x1 > r: r, m = x1, 1;  if x2 > r: r, m = x2, 2        (ties go to the smaller move)
 *       a[t][i] = r + lp[t][label(i)];  move[t][i] = m
 *   end state e = S - 1 if (S == 1 or a[T-1][S-1] > a[T-1][S-2]) else S - 2;  total = a[T-1][e]
 *   walk t = T-1 .. 0:  state[t] = e;  e -= move[t][e]
 *
 * Outputs, all DEVICE pointers, per row r:
 *   paths        int32 [rows, T]: label(state[t]); -1 at and past the row's frame length
 *   frame_scores float [rows, T]: lp[t][paths[t]]; untouched at and past the row's frame length
 *   spans        int32 [rows, max_target, 2]: target l owns the frames of state 2l + 1, (first frame, last frame + 1)
 *   span_scores  float [rows, max_target]: the fp32 sum of the target's frame_scores, added to 0 in frame order
 *   totals       float [rows]
 *   status       int32 [rows]:  0 aligned (a row of no frames and no targets: total 0);
 *                              -1 no alignment exists (total == -inf, or no frames for L > 0);
 *                              -2 malformed row (a target outside [0, C) or equal to blank, offsets not ascending within
 *                                 [0, target_offsets[rows]], L > max_target, a frame length outside [0, T])
 * A row whose status is below 0 writes nothing but its status, and nothing out of range is read for it.  Entries of
 * spans / span_scores at and past the row's L are untouched.  With NaN emissions the result is unspecified (a NaN cell stays
 * NaN, so the walk may never visit some targets: their spans are then left untouched and their span_scores are 0), but every
 * index read or written stays in range.
 *
 * Limits: 2 <= C, 0 <= blank < C, 0 <= max_target <= AMX_ALIGN_MAX_TARGET, rows * T < 2^31; AMX_EINVAL otherwise.
 *
 * The caller supplies the workspace, which holds the recorded moves: per row, ceil((2 max_target + 1) / 64) strips of
 * 64 states, per strip one 16-byte word (two 64-bit ballots) per frame, frames padded to a multiple of 64.
 * Stream-ordered on `stream`: no allocation, no host synchronisation beyond what amx_greedy_ctc does. */
#define AMX_ALIGN_MAX_TARGET 4095 /* 8191 states: two fp32 state rows are 64 KiB of LDS */

/* Pure host function; AMX_EINVAL when a limit is broken or the size is not representable in size_t. */
int amx_ctc_align_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes);

/* One fp32 emission tensor [N, T, C] on `device` with element strides (stride_n, stride_t, 1), read in place (e.g. the
 * transposed view of a [T, N, C] output); rows are the N utterances.  frame_lengths int32 [N], target_offsets int32
 * [N + 1] and target_ids int32 [target_offsets[N]] are DEVICE pointers: row n's targets are
 * target_ids[target_offsets[n] .. target_offsets[n + 1]). */
int amx_ctc_align_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                            int N, int64_t T, int C, int blank_index, const int32_t* target_offsets, const int32_t* target_ids,
                            int64_t max_target, void* workspace, size_t workspace_bytes, int32_t* paths, float* frame_scores,
                            int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream);

/* Every output of the last amx_forward, like amx_beam_ctc: `out` is the device output buffer for a batch of geometry
 * (N, L) under the current inventory, `frame_lengths` the int64 [N] HOST `Predictions.lengths`; rows are o * N + n in the
 * order of amx_output_layout (O outputs), blank 0; target_offsets is DEVICE int32 [O * N + 1]. */
int amx_ctc_align(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, const int32_t* target_offsets,
                  const int32_t* target_ids, int64_t max_target, void* workspace, size_t workspace_bytes, int32_t* paths,
                  float* frame_scores, int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream);

/* The same contract for whole transcripts: rows of up to AMX_ALIGN_LONG_MAX_TARGET targets (symbols added to ABI 6; detect
 * them with dlsym).  Recurrence, tie rule, end-state rule, walk, outputs and status codes are those above, and every output
 * is bit for bit what the entry points above give on a row both accept: a cell's value depends only on the cells of its
 * dependency cone, however the trellis is cut.  The states of a row are spread over the device: after one launch that
 * validates the rows, one launch per block of AMX_ALIGN_LONG_FRAME_BLOCK frames runs a grid of (state tiles, rows), where a
 * tile owns AMX_ALIGN_LONG_TILE_STATES states and recomputes a left halo of twice the frame block; one launch walks back and
 * writes the outputs.  No workgroup waits for another: the only ordering between frame blocks is the stream's.
 *
 * Limits: those above with 0 <= max_target <= AMX_ALIGN_LONG_MAX_TARGET (any max_target from 0 up is accepted, so the small
 * rows of the entry points above run here too).  Stream-ordered on `stream`: no allocation, no host synchronisation beyond
 * what the forms above do, and a number of launches that depends on the geometry alone (2 + ceil(T / 64) per 65535 rows).
 *
 * The workspace, with strips = ceil((2 max_target + 1) / 64) and Tp = T padded to a multiple of 64, holds in this order
 *   moves        rows * strips * Tp * 16 bytes   (as above)
 *   state rows   rows * 2 * strips * 64 * 4      (the state row between launches, ping-ponged by the frame block's parity)
 *   span bounds  rows * max_target * 2 * 4, rounded up to a multiple of 16
 *   live flags   rows * 4, rounded up to a multiple of 16
 * and amx_ctc_align_long_workspace returns the sum.  Its contents need not be initialised. */
#define AMX_ALIGN_LONG_MAX_TARGET 262143 /* 524 287 states */
#define AMX_ALIGN_LONG_FRAME_BLOCK 64    /* frames per launch */
#define AMX_ALIGN_LONG_TILE_STATES 832   /* states a workgroup owns; it computes 128 more, its left halo */

/* Pure host function; AMX_EINVAL when a limit is broken or the size is not representable in size_t. */
int amx_ctc_align_long_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes);

/* amx_ctc_align_emissions for rows of up to AMX_ALIGN_LONG_MAX_TARGET targets: the same arguments. */
int amx_ctc_align_long_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                                 int N, int64_t T, int C, int blank_index, const int32_t* target_offsets, const int32_t* target_ids,
                                 int64_t max_target, void* workspace, size_t workspace_bytes, int32_t* paths, float* frame_scores,
                                 int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream);

/* amx_ctc_align for rows of up to AMX_ALIGN_LONG_MAX_TARGET targets: the same arguments. */
int amx_ctc_align_long(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, const int32_t* target_offsets,
                       const int32_t* target_ids, int64_t max_target, void* workspace, size_t workspace_bytes, int32_t* paths,
                       float* frame_scores, int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_ALIGN_H */
