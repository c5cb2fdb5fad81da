/* Edit-distance evaluation entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_EDIT_H
#define ALLOPHANT_AMX_EDIT_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upstream's `run.py evaluate` on decoded hypotheses: `levensthein_statistics(expected, actual)` (uniform costs, the full
 * matrix and its back-trace, edit_distance.rs:372-481) per (output, utterance, candidate), the candidate of the lowest fp32
 * `word_error_rate` per (output, utterance) (the first strictly lower one wins, run.py:447-464), and its statistics added to
 * per-group totals.  Symbols added to ABI 6 without a struct change (detect them with dlsym).  The contract is restated in
 * DESIGN 9 and, as Python, in tests/edit_util.py.
 *
 * Statistics are int32 (insertions, deletions, substitutions, correct), in that order everywhere.
 *
 * Sequences are compared as ids.  Each output o has a LABEL map and, per hypothesis-map set h, a HYPOTHESIS map.  A map is a
 * CSR over int32 ids: its descriptor (first, entries) names entries e in [0, entries), and entry e expands to
 *     map_values[map_offsets[first + e] .. map_offsets[first + e + 1])
 * Expected = the concatenated expansions of the utterance's label ids through output o's label map; actual = those of the
 * candidate's tokens through the hypothesis map of set h = (H == 1 ? 0 : groups[n]).  (The Python binding builds both maps
 * from strings: contours, complex-segment splitting, remapping, label replacements and the blank offset all live in them.)
 *
 * Limits (AMX_EINVAL otherwise): 1 <= K <= AMX_EDIT_MAX_CANDIDATES, 0 <= max_expected, max_actual <= AMX_EDIT_MAX_LENGTH,
 * O, N, T >= 0, O * N * K < 2^31, G >= 1, H == 1 or H == G.
 *
 * The caller supplies the workspace (amx_edit_workspace gives its size): per scored row, max_expected + max_actual int32 for
 * the expanded sequences and 4 (max_actual + 1) int32 for two boundary rows of the DP.  It always lives in device memory:
 * the boundary rows of a 65535-long hypothesis do not fit in LDS, and one path serves every length. */
#define AMX_EDIT_MAX_LENGTH 65535   /* expanded symbols per side */
#define AMX_EDIT_MAX_CANDIDATES 64  /* K: the beam's width limit */

/* Pure host function (no device, no HIP call): workspace bytes for `rows` = O * N * K scored rows. */
int amx_edit_workspace(int64_t rows, int64_t max_expected, int64_t max_actual, size_t* bytes);

/* Scores every candidate on `device`.  All pointers are DEVICE pointers:
 *   tokens        int64 [O, N, K, T] with element strides (stride_o, stride_n, stride_k, 1): candidate k of row (o, n)
 *                 holds counts[o, n, k] tokens (e.g. `Decoded.tokens` as [O, N, 1, T], `BeamDecoded.tokens`)
 *   counts        int32 [O, N, K] contiguous
 *   hyp_counts    int32 [O, N] candidates present per row (`BeamDecoded.hyp_counts`), or NULL for K everywhere; clamped to [0, K]
 *   label_offsets int32 [N + 1], label_ids int32: utterance n's label is label_ids[label_offsets[n] .. label_offsets[n + 1])
 *   groups        int32 [N]: the totals slot (the language) of each utterance, in [0, G)
 *   label_maps    int32 [O, 2], hyp_maps int32 [H, O, 2]: map descriptors (first, entries)
 *   workspace     workspace_bytes >= amx_edit_workspace(O * N * K, max_expected, max_actual)
 * and writes
 *   statistics    int32 [O, N, K, 4]: scored candidates their statistics; candidates at or past the row's hyp_counts -1 x 4;
 *                 a row with a token or label id outside its map, a count outside [0, T], a bad group or an expansion longer
 *                 than max_expected / max_actual -2 x 4 (nothing out of range is read)
 *   best          int32 [O, N]: the chosen candidate; -1 if none has a finite rate below +inf (an empty label gives 0/0 or
 *                 x/0: upstream skips such rows); -2 if any candidate of the row is flagged (-2 statistics)
 *   totals        uint64 [G, O, 4]: best >= 0 adds its four counts to totals[groups[n], o] (integer atomics: the sums are
 *                 the same in any order).  Accumulated, never cleared.
 * Two launches (score, then select-and-add), stream-ordered on `stream`: no allocation and no host synchronisation (the
 * call can be captured in a graph). */
int amx_edit_statistics(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k, int O, int N,
                        int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts, const int32_t* label_offsets,
                        const int32_t* label_ids, const int32_t* groups, int G, const int32_t* map_offsets,
                        const int32_t* map_values, const int32_t* label_maps, const int32_t* hyp_maps, int H,
                        int64_t max_expected, int64_t max_actual, void* workspace, size_t workspace_bytes, int32_t* statistics,
                        int32_t* best, uint64_t* totals, void* stream);

/* Upstream's `run.py edits` on decoded hypotheses: `levensthein_operations(expected, actual)` (uniform costs, the walk of
 * edit_distance.rs:101-279, the same path as the statistics) and `to_substitutions` per (output, utterance), for candidate 0
 * only.  Added to ABI 6 like the statistics.  The contract is restated in DESIGN 9 and, as Python, in tests/edit_ops_util.py.
 *
 * An operation is the record int32 (action, i, j, expected id, actual id): the action (below), the coordinates after the move
 * (i indexes expected for a deletion or substitution, j indexes actual for an insertion or substitution; the other one is
 * where the walk stood) and the symbol ids expected[i] / actual[j] it names, -1 where to_substitutions writes "".  A row's
 * records are in upstream's order (the back-trace reversed), one per unit of cost: their count is the edit distance, at most
 * max(m, n).  Maps and limits as amx_edit_statistics with K = 1; also max(max_expected, max_actual) <= max_ops < 2^31.
 *
 * The workspace (amx_edit_operations_workspace gives its size) holds, per row, the statistics row's buffers and the path:
 * 16 bytes per wave step of the DP, ceil(max_expected / 64) strips x (max_actual + 64, padded to 16) steps. */
#define AMX_EDIT_INSERTION 1
#define AMX_EDIT_DELETION 2
#define AMX_EDIT_SUBSTITUTION 3

/* Pure host function (no device, no HIP call): workspace bytes for `rows` = O * N rows; AMX_EINVAL when not representable. */
int amx_edit_operations_workspace(int64_t rows, int64_t max_expected, int64_t max_actual, size_t* bytes);

/* The operations of candidate 0 on `device`.  All pointers are DEVICE pointers:
 *   tokens        int64 [O, N, T] with element strides (stride_o, stride_n, 1): row (o, n) holds counts[o, n] tokens
 *                 (`Decoded.tokens`, or the k = 0 view of `BeamDecoded.tokens`)
 *   counts        int32 [O, N] contiguous
 *   hyp_counts    int32 [O, N] candidates present per row, or NULL: a row with 0 (or fewer) has no candidate
 *   label_offsets, label_ids, groups, map_offsets, map_values, label_maps, hyp_maps, H: as amx_edit_statistics
 *   workspace     workspace_bytes >= amx_edit_operations_workspace(O * N, max_expected, max_actual)
 * and writes
 *   operations        int32 [O, N, max_ops, 5]: records [0, operation_counts[o, n]) of each row; nothing past them
 *   operation_counts  int32 [O, N]: the cost (the number of records); -1 for a row with no candidate; -2 for a row flagged
 *                     as amx_edit_statistics flags it (an id outside its map, a count outside [0, T], a bad group, an
 *                     expansion longer than max_expected / max_actual; nothing out of range is read)
 * One launch, stream-ordered on `stream`: no allocation and no host synchronisation (the call can be captured in a graph). */
int amx_edit_operations(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int O, int N, int64_t T,
                        const int32_t* counts, const int32_t* hyp_counts, const int32_t* label_offsets, const int32_t* label_ids,
                        const int32_t* groups, int G, const int32_t* map_offsets, const int32_t* map_values,
                        const int32_t* label_maps, const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual,
                        void* workspace, size_t workspace_bytes, int64_t max_ops, int32_t* operations,
                        int32_t* operation_counts, void* stream);

/* Upstream's `PropertyWeighting(insertion_cost, deletion_cost, property_table)` (edit_distance.rs:498-599) on decoded
 * hypotheses: levensthein_statistics, levensthein_operations and levensthein_matrix with fp32 costs, a substitution costing the
 * number of feature columns in which the two symbols' rows differ.  Added to ABI 6 like the calls above.  The contract is
 * restated in DESIGN 9 and, as Python, in tests/edit_weighted_util.py.  With expected of length m and actual of length n, all
 * arithmetic in fp32:
 *     M[0][j] = (float)j                      (one per insertion whatever insertion_cost is: upstream's first row)
 *     M[i][0] = M[i - 1][0] + deletion_cost   (repeated addition, rounded each time)
 *     M[i][j] = min(min(M[i][j - 1] + insertion_cost, M[i - 1][j] + deletion_cost), M[i - 1][j - 1] + d(expected_i, actual_j))
 * and the walk is the uniform calls' (it reads matrix values only).  The kernels perform these additions and minima, so every
 * cost is upstream's bit for bit.  Two different symbols with equal rows cost 0: a match, no record.
 *
 * d comes from a COST TABLE per id space: uint8 [V, V], entry (x, y) the number of differing feature columns of symbols x and
 * y, built on the device by amx_edit_cost_table from feature codes uint8 [V, F] (the caller canonicalises each column's values
 * to codes: only equality matters).  Limits (AMX_EINVAL otherwise): 1 <= V <= AMX_EDIT_MAX_SYMBOLS (a table of at most 64 MiB;
 * PHOIBLE's about 3200 phonemes and their split segments fit), 0 <= F <= AMX_EDIT_MAX_FEATURES (a count fits a byte); both
 * costs finite and > 0 (with a cost of 0 upstream's walk can stop off the diagonal, where its `correct` count means nothing).
 *
 * Each output o has a cost-table descriptor int64 (first, V) in cost_tables [O, 2] (device memory): its table starts at
 * cost_table_data + first; V == 0 says "none": d = (expected_i != actual_j), and cost_table_data may be NULL if every output
 * says so.  A row with an expanded symbol id outside [0, V) of its output's table is flagged -2; nothing out of range is read. */
#define AMX_EDIT_MAX_SYMBOLS 8192  /* V: symbols of one cost table */
#define AMX_EDIT_MAX_FEATURES 255  /* F: feature columns of a row */

/* Pure host function (no device, no HIP call): bytes of a cost table over V symbols (V * V). */
int amx_edit_cost_table_bytes(int64_t V, size_t* bytes);

/* Builds table uint8 [V, V] from codes uint8 [V, F] (DEVICE pointers) on `device`.  One launch, stream-ordered on `stream`. */
int amx_edit_cost_table(int device, const uint8_t* codes, int64_t V, int64_t F, uint8_t* table, void* stream);

/* amx_edit_statistics under the weighted costs: arguments, limits, workspace (amx_edit_workspace), flags (-1 / -2), candidate
 * choice (the first candidate of strictly lowest fp32 word_error_rate of its integer counts) and totals as there.  Also
 *   costs         float [O, N, K]: M[m][n] of every scored candidate (flagged and absent candidates: not written)
 * Two launches, stream-ordered on `stream`: no allocation and no host synchronisation (capturable in a graph). */
int amx_edit_weighted_statistics(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k, int O,
                                 int N, int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                 const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                 const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                 const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual, void* workspace,
                                 size_t workspace_bytes, float insertion_cost, float deletion_cost, const int64_t* cost_tables,
                                 const uint8_t* cost_table_data, int32_t* statistics, int32_t* best, uint64_t* totals,
                                 float* costs, void* stream);

/* amx_edit_operations under the weighted costs: arguments, limits, workspace (amx_edit_operations_workspace), records and
 * flags as there, except that an operation no longer costs 1:
 *   operation_counts  int32 [O, N]: the number of records, S + D + I of the row's statistics (or -1 / -2)
 *   costs             float [O, N]: M[m][n] (rows flagged or without a candidate: not written)
 * A dear substitution may be replaced by a deletion and an insertion, so a row holds up to m + n records:
 * max_expected + max_actual <= max_ops < 2^31.  One launch, stream-ordered on `stream`; capturable in a graph. */
int amx_edit_weighted_operations(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int O, int N, int64_t T,
                                 const int32_t* counts, const int32_t* hyp_counts, const int32_t* label_offsets,
                                 const int32_t* label_ids, const int32_t* groups, int G, const int32_t* map_offsets,
                                 const int32_t* map_values, const int32_t* label_maps, const int32_t* hyp_maps, int H,
                                 int64_t max_expected, int64_t max_actual, void* workspace, size_t workspace_bytes,
                                 float insertion_cost, float deletion_cost, const int64_t* cost_tables,
                                 const uint8_t* cost_table_data, int64_t max_ops, int32_t* operations, int32_t* operation_counts,
                                 float* costs, void* stream);

/* levensthein_matrix for pairs of id sequences handed over directly (no maps).  All pointers are DEVICE pointers:
 *   expected_offsets int32 [rows + 1], expected_ids int32: row r's expected is expected_ids[expected_offsets[r] ..
 *                    expected_offsets[r + 1]); actual_offsets / actual_ids the same for actual
 *   cost_table       uint8 [V, V] of the pairs' id space, or V == 0 (then it may be NULL): d = (expected_i != actual_j); unit
 *                    costs with V == 0 give upstream's module-level levensthein_matrix
 *   workspace        workspace_bytes >= amx_edit_workspace(rows, max_expected, max_actual)
 * and writes
 *   matrix  float [rows, max_expected + 1, max_actual + 1]: cells [0, m] x [0, n] of row r; nothing outside them
 *   status  int32 [rows]: 0, or -2 for a row longer than max_expected / max_actual, with bad offsets or with an id outside
 *           [0, V) (its matrix is not written; nothing out of range is read)
 * Limits: 0 <= rows < 2^31, lengths as above, 0 <= V <= AMX_EDIT_MAX_SYMBOLS, costs finite and > 0; the caller's matrix buffer
 * bounds the size.  One launch, stream-ordered on `stream`; capturable in a graph. */
int amx_edit_matrix(int device, const int32_t* expected_offsets, const int32_t* expected_ids, const int32_t* actual_offsets,
                    const int32_t* actual_ids, int64_t rows, int64_t max_expected, int64_t max_actual, float insertion_cost,
                    float deletion_cost, const uint8_t* cost_table, int64_t V, void* workspace, size_t workspace_bytes,
                    float* matrix, int32_t* status, void* stream);

/* Confusion tables: which symbol is taken for which, what is deleted and inserted, and how often each symbol is right, per
 * (group, output), accumulated on the device over any number of calls.  Added to ABI 7 without a struct change (detect the
 * symbols with dlsym).  The contract is restated in DESIGN 9 and, as Python, in tests/confusion_util.py.
 *
 * A scored row, with expanded expected A[0, m) and actual B[0, n), contributes the EVENTS of upstream's back-trace from (m, n)
 * (the path of amx_edit_statistics and amx_edit_operations, same tie-breaking), continued to the origin where upstream's walk
 * stops at cost 0 (below such a cell every move is diagonal and i == j): a diagonal move is the event (A[i-1], B[j-1]), match
 * and substitution alike; a deletion (A[i-1], eps); an insertion (eps, B[j-1]).  That is m + n - #diagonal events.  Summed over
 * a row, events with eps on neither side and expected != actual are its S, (e, eps) its D, (eps, a) its I and (e, e) its C
 * (weighted costs: pairs of table cost 0 are C, pairs of cost > 0 are S).
 *
 * TABLE: `capacity` slots of 16 bytes in device memory, a slot a uint64 key followed by a uint64 count.  Key 0 is an empty
 * slot: the caller zeroes a new table.  An occupied slot's key packs
 *     (g * O + o + 1) << 42 | (expected id + 1) << 21 | (actual id + 1)          eps: id -1, i.e. the field 0
 * (AMX_EDIT_CONFUSION_GROUP_BITS / _SYMBOL_BITS: 22 / 21 / 21 bits; ids are those of the output's id space, what the maps
 * expand to).  A row whose symbol ids exceed 2^21 - 2, or any row when G * O exceeds 2^22 - 1, is flagged -2 rather than
 * truncated.  A key lives in the first free slot of the linear probe sequence that starts at hash(key) & (capacity - 1); an
 * empty slot is claimed with a 64-bit compare-and-swap and counts grow by 64-bit integer atomic adds only, so every count is
 * the same whatever the order of arrival and a table is bitwise reproducible once its occupied slots are sorted by key.  SLOT
 * POSITIONS ARE NOT reproducible: they depend on which key arrives first.  A probe sequence ends after `capacity` slots; an
 * event that finds none is added to counters[1] and otherwise lost (a full table cannot spin).
 *
 *   counters  uint64 [2]: [0] events added to the table (the sum of its counts), [1] events dropped.  Accumulated, never
 *             cleared: the caller zeroes them with the table. */
#define AMX_EDIT_CONFUSION_GROUP_BITS 22
#define AMX_EDIT_CONFUSION_SYMBOL_BITS 21
#define AMX_EDIT_CONFUSION_MIN_CAPACITY 16
#define AMX_EDIT_CONFUSION_MAX_CAPACITY (1 << 28)

/* Pure host function (no device, no HIP call): bytes of a table of `capacity` slots (16 * capacity).  `capacity` must be a
 * power of two, AMX_EDIT_CONFUSION_MIN_CAPACITY <= capacity <= AMX_EDIT_CONFUSION_MAX_CAPACITY (AMX_EINVAL otherwise). */
int amx_edit_confusion_table_bytes(int64_t capacity, size_t* bytes);

/* Adds the events of one candidate of every (output, utterance) row to `table`.  Arguments up to workspace_bytes as
 * amx_edit_statistics (tokens [O, N, K, T], counts [O, N, K], the same limits), except that the workspace is that of
 * amx_edit_operations_workspace(O * N, max_expected, max_actual).  All pointers are DEVICE pointers:
 *   best        int32 [O, N] as amx_edit_statistics wrote it, or NULL.  Row (o, n) walks candidate best[o, n]; best == -1 gives
 *               row_events -1 and best == -2 (or a best at or past the candidates present) row_events -2, and such a row adds
 *               nothing.  NULL: candidate 0, and a row whose hyp_counts is 0 (or less) has no candidate
 *   table, capacity   as above
 * and writes
 *   row_events  int32 [O, N]: the number of events of the row (added or dropped); -1 for a row with no candidate; -2 for a row
 *               flagged as amx_edit_operations flags it, or whose ids do not fit a key: nothing out of range is read and
 *               nothing of the row is added
 *   counters    as above
 * One launch, stream-ordered on `stream`: no allocation and no host synchronisation (the call can be captured in a graph). */
int amx_edit_confusions(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k, int O, int N,
                        int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts, const int32_t* label_offsets,
                        const int32_t* label_ids, const int32_t* groups, int G, const int32_t* map_offsets,
                        const int32_t* map_values, const int32_t* label_maps, const int32_t* hyp_maps, int H,
                        int64_t max_expected, int64_t max_actual, void* workspace, size_t workspace_bytes, const int32_t* best,
                        void* table, int64_t capacity, int32_t* row_events, uint64_t* counters, void* stream);

/* amx_edit_confusions on the path of the weighted costs: cost arguments, their limits and the extra flag (a symbol outside its
 * output's cost table: -2) as amx_edit_weighted_operations; `best` as amx_edit_weighted_statistics wrote it.  One launch. */
int amx_edit_weighted_confusions(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k, int O,
                                 int N, int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                 const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                 const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                 const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual, void* workspace,
                                 size_t workspace_bytes, float insertion_cost, float deletion_cost, const int64_t* cost_tables,
                                 const uint8_t* cost_table_data, const int32_t* best, void* table, int64_t capacity,
                                 int32_t* row_events, uint64_t* counters, void* stream);

/* Adds every occupied slot of `src` (key, count) into `dst`: growing a table (into a zeroed larger one) or combining two.  The
 * tables must not overlap.  counters[0] grows by the events that found a slot in `dst`, counters[1] by those that did not (a
 * `dst` that is too small).  One launch over the slots of `src`, stream-ordered on `stream`. */
int amx_edit_confusion_merge(int device, const void* src, int64_t src_capacity, void* dst, int64_t dst_capacity,
                             uint64_t* counters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_EDIT_H */
