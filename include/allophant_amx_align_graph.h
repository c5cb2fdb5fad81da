/* CTC forced alignment over pronunciation graphs: entry points of liballophant_amx (companion of allophant_amx.h and
 * allophant_amx_align.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_ALIGN_GRAPH_H
#define ALLOPHANT_AMX_ALIGN_GRAPH_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The best CTC path (Viterbi) through a graph of alternative label sequences, on the device.  Symbols added to ABI 7
 * without a struct change (detect them with dlsym).  A row is one emission matrix lp[T][C] (fp32, T = the row's frame
 * length), a blank, and a label graph of L nodes.  Node j has a class y[j] (never the blank), a flag word (bit 0: initial,
 * bit 1: final) and an ordered list pred[j][0..d_j) of predecessor nodes, every one < j (node order is a topological order),
 * d_j <= AMX_ALIGN_GRAPH_MAX_IN; at most AMX_ALIGN_GRAPH_MAX_IN nodes are final.
 *
 * States: S = 2L + 1.  2j is the leading blank of node j, 2j + 1 its label state, E = 2L the closing blank.  All
 * arithmetic is fp32 and -inf is an ordinary value:
 *
 *   a[0][2j] = lp[0][blank], a[0][2j+1] = lp[0][y[j]]  for every initial j;  a[0][E] = lp[0][blank] if L == 0;
 *   every other a[0][i] = -inf
 *   candidates of state i, in order (an absent candidate is skipped):
 *       label state 2j+1:  m = 0 itself;  m = 1 state 2j;  m = 2 + k state 2 pred[j][k] + 1, only if y[pred[j][k]] != y[j]
 *       blank state 2j:    m = 0 itself;  m = 2 + k state 2 pred[j][k] + 1 (always);  m = 1 is never taken
 *       E:                 m = 0 itself;  m = 2 + k the label state of the k-th final node in ascending node order
 *   for t >= 1, every i:
 *       r, m = a[t-1][cand_0], 0;  then in candidate order: if a[t-1][cand] > r: r, m = that value, its index
 *       a[t][i] = r + lp[t][label(i)];  move[t][i] = m                                    (ties go to the earlier candidate)
 *   end: candidates are the final nodes' label states in ascending node order, then E; start from the first and replace on
 *        strict >;  total = the chosen value
 *   walk t = T-1 .. 0:  state[t] = e;  e = cand_{move[t][e]}(e)
 *
 * A chain (pred[j] = {j - 1}, node 0 initial, node L - 1 final) gives every output of amx_ctc_align bit for bit.
 *
 * Outputs, all DEVICE pointers, per row r, shaped like amx_ctc_align's with max_nodes for max_target:
 *   paths        int32 [rows, T]: label(state[t]); -1 at and past the row's frame length
 *   frame_scores float [rows, T]: lp[t][paths[t]]; untouched at and past the row's frame length
 *   spans        int32 [rows, max_nodes, 2]: per NODE, (first frame, last frame + 1) of its label state when the path
 *                visits it, (-1, -1) for every other node < L
 *   span_scores  float [rows, max_nodes]: the fp32 sum of the node's frame_scores, added to 0 in frame order; 0 for an
 *                unvisited node
 *   totals       float [rows]
 *   status       int32 [rows]:  0 aligned (L == 0 included; a row of no frames and no nodes: total 0);
 *                              -1 no path (total == -inf, or no frames for L > 0);
 *                              -2 malformed row (a class outside [0, C) or equal to blank, a predecessor >= j or < 0,
 *                                 d_j > AMX_ALIGN_GRAPH_MAX_IN, more than AMX_ALIGN_GRAPH_MAX_IN finals, L > 0 without
 *                                 an initial or without a final node, offsets that do not ascend or lie outside the
 *                                 arrays, L > max_nodes, a frame length outside [0, T])
 * The chosen pronunciation is the visited nodes in ascending index.  A row whose status is below 0 writes nothing but its
 * status, and nothing out of range is read for it.  Entries of spans / span_scores at and past the row's L are untouched.
 * With NaN emissions the result is unspecified, but every index read or written stays in range.
 *
 * Graph arrays, all DEVICE int32:
 *   node_offsets [rows + 1]                  row r has the nodes node_offsets[r] .. node_offsets[r + 1]
 *   node_classes [node_offsets[rows]]
 *   node_flags   [node_offsets[rows]]
 *   arc_offsets  [node_offsets[rows] + 1]    one CSR over all nodes of all rows
 *   arc_preds    [arc_offsets[last]]         row-local node indices
 *
 * Limits: those of amx_ctc_align with max_nodes for max_target (2 <= C, 0 <= blank < C, 0 <= max_nodes <=
 * AMX_ALIGN_GRAPH_MAX_NODES, rows * T < 2^31); AMX_EINVAL otherwise.
 *
 * The caller supplies the workspace, which holds the recorded moves: rows * ceil((2 max_nodes + 1) / 64) * Tp * 32 bytes,
 * Tp = T padded to a multiple of 64: one 32-byte record per (strip of 64 states, frame), three 64-bit ballots (one per bit
 * of m) and 8 spare bytes.  Its contents need not be initialised.  Stream-ordered on `stream`: no allocation, no host
 * synchronisation beyond what amx_ctc_align does.  No atomics: the outputs are bitwise reproducible. */
#define AMX_ALIGN_GRAPH_MAX_NODES 4095 /* 8191 states: two fp32 state rows are 64 KiB of LDS */
#define AMX_ALIGN_GRAPH_MAX_IN 6       /* predecessors per node, and final nodes per row */

/* Pure host function; AMX_EINVAL when a limit is broken or the size is not representable in size_t. */
int amx_ctc_align_graph_workspace(int64_t rows, int64_t T, int64_t max_nodes, size_t* bytes);

/* One fp32 emission tensor [N, T, C] on `device` with element strides (stride_n, stride_t, 1), read in place; rows are the
 * N utterances.  frame_lengths int32 [N] and the five graph arrays are DEVICE pointers. */
int amx_ctc_align_graph_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                  const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                  const int32_t* node_offsets, const int32_t* node_classes, const int32_t* node_flags,
                                  const int32_t* arc_offsets, const int32_t* arc_preds, int64_t max_nodes, void* workspace,
                                  size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores,
                                  float* totals, int32_t* status, void* stream);

/* Every output of the last amx_forward, like amx_ctc_align: rows are o * N + n in the order of amx_output_layout (O outputs),
 * blank 0; `frame_lengths` is the int64 [N] HOST `Predictions.lengths`; node_offsets is DEVICE int32 [O * N + 1]. */
int amx_ctc_align_graph(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, const int32_t* node_offsets,
                        const int32_t* node_classes, const int32_t* node_flags, const int32_t* arc_offsets, const int32_t* arc_preds,
                        int64_t max_nodes, void* workspace, size_t workspace_bytes, int32_t* paths, float* frame_scores,
                        int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_ALIGN_GRAPH_H */
