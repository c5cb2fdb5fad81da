/* Allophone-layer entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_ALLOPHONES_H
#define ALLOPHANT_AMX_ALLOPHONES_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Language-specific phoneme outputs through the allophone layer: `AllophoneMapping.map_allophones` (acoustic_model.py:142-159)
 * for models built with allophone_layer = 1.  Symbols added to ABI 6 without a struct change (detect them with dlsym);
 * declared in this companion header so that allophant_amx.h keeps naming exactly the ABI-6 surface.
 *
 * amx_set_allophones takes the reference's host arrays: `matrices` fp32 [n_lang, P1, Q1] (the trained `_allophone_matrices`)
 * and `mask` uint8 [n_lang, P1, Q1] (`_allophone_mask`: 1 = masked, derived from the mapping's structure).  P1 is the phone
 * output width (shared phones + blank), Q1 the phoneme classifier's size + 1.  Keeps, per (language, phoneme) column, only its
 * unmasked entries on the device; allocates and synchronises; a second call replaces the first.  AMX_EINVAL for a model
 * without an allophone layer or a P1 / Q1 that does not match it (P1 <= 16384).
 *
 * amx_map_allophones: out[t, n, q] = max over unmasked p of phone[t, n, p] * W[l, p, q] with l = language_ids[n], finfo(float32)
 * .min for a column with masked entries when that is larger, NaN propagating -- bitwise the reference's values.
 *   phone         fp32 [T, N, P1] DEVICE, element strides (stride_t, stride_n, 1): e.g. the "phone" output of amx_forward
 *   language_ids  int32 [N] DEVICE, dense indices in [0, n_lang)
 *   out           fp32 [T, N, Q1] DEVICE, contiguous
 * Stream-ordered on `stream`: no allocation, no host synchronisation; leaves the forward pass's graphs and range report alone.
 * N = 0 or T = 0 does nothing.  AMX_ESTATE before amx_set_allophones. */
int amx_set_allophones(amx_handle h, int n_lang, int P1, int Q1, const float* matrices, const uint8_t* mask);
int amx_map_allophones(amx_handle h, const float* phone, int64_t stride_t, int64_t stride_n, const int32_t* language_ids, int N,
                       int64_t T, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_ALLOPHONES_H */
