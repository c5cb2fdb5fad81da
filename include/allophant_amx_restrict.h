/* Per-utterance inventory restriction of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_RESTRICT_H
#define ALLOPHANT_AMX_RESTRICT_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One pass under the UNION of several languages' phoneme inventories holds every language's logits (a composed phoneme's
 * logit depends on its own feature row only); this call restricts such an output to each utterance's own language, on the
 * device: the log-softmax over a language's classes is the union row restricted to them and renormalised.  Symbol added to
 * ABI 6 without a struct change (detect it with dlsym).  Stateless, like the other *_emissions calls.
 *
 *   src, out       fp32 [T, N, C] DEVICE tensors with element strides (stride_t, stride_n, 1) and (out_stride_t, out_stride_n,
 *                  1), e.g. the composed block of amx_forward's output buffer, or its transposed view; strides are >= 0
 *   frame_lengths  int32 [N] DEVICE
 *   language_ids   int32 [N] DEVICE
 *   member_bits    uint64 [n_lang, (C + 63) / 64] DEVICE: bit c % 64 of word c / 64 of row l is set where class c belongs to
 *                  language l.  The blank is a class like any other: the caller sets its bit.  Bits at and past C are ignored.
 *   status         int32 [N] DEVICE
 *
 * All arithmetic is fp32 and -inf is an ordinary value.  For utterance n with l = language_ids[n] and members M_l:
 *
 *   for t < frame_lengths[n]:
 *       m = max over c in M_l of src[t][n][c]                                (-inf where M_l is empty)
 *       if m == -inf:  lse = -inf                                            (no member, or every member is -inf)
 *       else:          lse = m + log(sum over c in M_l of exp(src[t][n][c] - m))
 *       c in M_l, with AMX_RESTRICT_NORMALIZE:   out[t][n][c] = -inf if lse == -inf, else src[t][n][c] - lse
 *                                                (one fp32 subtraction; nothing subtracts -inf from -inf)
 *       c in M_l, without the flag:              out[t][n][c] = src[t][n][c], bit for bit (the raw-logit form)
 *       c not in M_l:                            out[t][n][c] = -inf, in both forms
 *   for t >= frame_lengths[n]:  out[t][n][c] = 0.0f for all C classes (the library's contract for frames beyond the lengths)
 *
 *   status[n] =  0  a well-formed utterance;
 *               -2  language_ids[n] outside [0, n_lang) or frame_lengths[n] outside [0, T]: the utterance writes its status
 *                   only, and nothing out of range is read for it
 *
 * `out` may be `src` with equal strides (in place), and the in-place result is bitwise the out-of-place one; any other overlap
 * is the caller's error.  The sum runs in a fixed order (per lane of a 64-lane wave over the columns lane, lane + 64, ...
 * ascending, then one fixed reduction tree) and there are no atomics: a row's result is bitwise the same run to run.  With NaN
 * inputs the values are unspecified, but every index read or written stays in range.
 *
 * Limits: 2 <= C <= AMX_RESTRICT_MAX_CLASSES, n_lang >= 1, N >= 0, T >= 0, strides >= 0, no flag but AMX_RESTRICT_NORMALIZE,
 * the last element's offset (T - 1) * stride_t + (N - 1) * stride_n + C - 1 of either tensor below 2^63 and N * T below 2^32;
 * non-null pointers where N > 0 and T > 0; AMX_EINVAL otherwise.  N == 0 or T == 0 does nothing (status included) and
 * returns AMX_OK.
 *
 * Stream-ordered on `stream`: no allocation and no host synchronisation, so a call can be captured in a graph.  It knows no
 * handle: the forward pass's graphs and its range report are left alone (the range check ran in the forward pass, before these
 * -inf exist). */
#define AMX_RESTRICT_NORMALIZE 1u
#define AMX_RESTRICT_MAX_CLASSES 65535

int amx_restrict_outputs(int device, const float* src, int64_t stride_t, int64_t stride_n, int C, const int32_t* frame_lengths,
                         const int32_t* language_ids, const uint64_t* member_bits, int n_lang, int N, int64_t T, uint32_t flags,
                         float* out, int64_t out_stride_t, int64_t out_stride_n, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_RESTRICT_H */
