/* CTC search entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_SEARCH_H
#define ALLOPHANT_AMX_SEARCH_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where in an utterance a short label sequence (a query) occurs, on the device: the best CTC path of the query through any
 * span of frames, start and end free.  Symbols added to ABI 6 without a struct change (detect them with dlsym).  A row is
 * (utterance n, query q), row index n * Q + q: the utterance's emission matrix lp[T][C] (fp32, T = its frame length), the
 * query y[0..L), L >= 1, and a blank.  S = 2L - 1 states: label(i) = y[i / 2] for even i and `blank` for odd i; there is no
 * leading or trailing blank state, so spans are tight.  All arithmetic is fp32 and -inf is an ordinary value:
 *
 *   m[t] = max_c lp[t][c]
 *   e[t][i] = -inf if lp[t][label(i)] == -inf, else lp[t][label(i)] - m[t]      (one fp32 subtraction; <= 0, and +0 exactly
 *                                                                               where the label is the frame's argmax)
 *   d[-1][i] = -inf, b[-1][i] = -1
 *   for t = 0 .. T-1, every i:
 *       r, s = d[t-1][i], b[t-1][i]
 *       if i >= 1 and d[t-1][i-1] > r:                                   r, s = d[t-1][i-1], b[t-1][i-1]
 *       if i even, i >= 2, y[i/2] != y[i/2 - 1] and d[t-1][i-2] > r:     r, s = d[t-1][i-2], b[t-1][i-2]
 *       if i == 0 and 0 > r:                                             r, s = 0, t          (a fresh start)
 *       d[t][i] = r + e[t][i];  b[t][i] = s                              (one fp32 addition)
 *   end_scores[t] = d[t][S-1];  end_starts[t] = b[t][S-1] if d[t][S-1] > -inf else -1
 *   best: scan t ascending; if end_scores[t] > -inf and end_scores[t] >= best: best = end_scores[t], span = (end_starts[t], t + 1)
 *
 * Ties go to the smaller move and a fresh start needs a strict >, so the start is the first frame of the first symbol's run;
 * among equal end scores the later frame wins, so the end is the last frame of the last symbol's run and of two equally good
 * occurrences the later one is reported.  The score is the log-likelihood ratio of the query's best path through
 * [start, end) against the frame-wise best path over the same frames: <= 0, and 0 exactly when the argmax path over the
 * span reads the query.  A frame whose emissions are all -inf is impassable.
 *
 * Outputs, all DEVICE pointers, per row r:
 *   best_scores float [N * Q]       written for status 0
 *   best_spans  int32 [N * Q, 2]    (start frame, end frame + 1), written for status 0
 *   status      int32 [N * Q]       always written:
 *                                     0 found;
 *                                    -1 no occurrence (every end score is -inf: no frames, too few frames for the symbols and
 *                                       their repeats, -inf on every path): the row writes its status and its curves
 *                                       (-inf / -1 over its frames), not its best_* entries;
 *                                    -2 malformed row (L == 0 or L > max_query, an id outside [0, C) or equal to blank,
 *                                       offsets not ascending within [0, query_offsets[Q]], a frame length outside [0, T]):
 *                                       the row writes its status only, and nothing out of range is read for it
 *   end_scores  float [N * Q, T]    optional; both curve pointers NULL or both non-NULL
 *   end_starts  int32 [N * Q, T]    optional
 * The curves are untouched at and past the row's frame length.  With NaN emissions the values are unspecified, but every
 * index read or written stays in range.  A row's result is bitwise the same run to run.
 *
 * Limits: 2 <= C, 0 <= blank < C, 1 <= max_query <= AMX_SEARCH_MAX_QUERY, N * Q * T < 2^31 (and N * Q < 2^31 where T is 0);
 * AMX_EINVAL otherwise.
 *
 * The caller supplies the workspace, which holds the per-frame maxima m[N][T] (fp32) and nothing per row: there is no
 * back-trace, the start frame is carried forward with the score.  Stream-ordered on `stream`: no allocation and no host
 * synchronisation, so a call can be captured in a graph. */
#define AMX_SEARCH_MAX_QUERY 256 /* 511 states: eight strips of 64 states in one wave */

/* Pure host function; AMX_EINVAL when a limit is broken or the size is not representable in size_t. */
int amx_ctc_search_workspace(int64_t N, int64_t Q, int64_t T, int64_t max_query, size_t* bytes);

/* One fp32 emission tensor [N, T, C] on `device` with element strides (stride_n, stride_t, 1), read in place (e.g. the
 * transposed view of a [T, N, C] output).  frame_lengths int32 [N], query_offsets int32 [Q + 1] and query_ids int32
 * [query_offsets[Q]] are DEVICE pointers: query q is query_ids[query_offsets[q] .. query_offsets[q + 1]).  Every utterance
 * is searched for every query. */
int amx_ctc_search_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                             int N, int64_t T, int C, int blank_index, const int32_t* query_offsets, const int32_t* query_ids, int Q,
                             int64_t max_query, void* workspace, size_t workspace_bytes, float* best_scores, int32_t* best_spans,
                             int32_t* status, float* end_scores, int32_t* end_starts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_SEARCH_H */
