/* Sinc resampling entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_RESAMPLE_H
#define ALLOPHANT_AMX_RESAMPLE_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `torchaudio.functional.resample(x, orig_freq, new_freq, lowpass_filter_width, rolloff, "sinc_interp_hann")`, which
 * upstream applies to every utterance before `Estimator.predict` (README recipe; datasets/speech_corpus.py through
 * `transforms.Resample(sr, 16000)`).  Symbols added to ABI 6 without a struct change (detect them with dlsym).
 *
 * Contract (restated in DESIGN 9 and, as float64 code, in tests/resample_util.py): with g = gcd(orig, new), o = orig / g,
 * m = new / g, f_c = min(o, m) * rolloff and W = ceil(lpw * o / f_c), phase j in [0, m) has the taps i in [0, 2W + o)
 *     tau = clamp(((i - W) / o - j / m) * f_c, -lpw, lpw),  h_j[i] = f_c / o * cos^2(pi tau / (2 lpw)) * sinc(pi tau)
 * and y[f * m + j] = sum_i h_j[i] * x[f * o + i - W] with x = 0 outside [0, len), for the len' = ceil(m * len / o) outputs.
 * o == m copies the input.  Only the taps with |unclamped tau| < lpw are kept (a contiguous run per phase): the others are
 * below 1e-30 in float64.
 *
 * Limits (AMX_EINVAL otherwise): 1 <= orig, new <= 2^31 - 1; 1 <= lowpass_filter_width <= 1024; 0 < rolloff <= 1; the
 * reduced m <= 4096; taps * m <= 2^22 floats of bank; and a window (below) of at most AMX_RESAMPLE_MAX_WINDOW floats,
 * which admits decimation by up to about 15 at the default filter (192 kHz -> 16 kHz passes, 256 kHz -> 16 kHz does
 * not). */
#define AMX_RESAMPLE_MAX_PHASES 4096
#define AMX_RESAMPLE_MAX_WINDOW 16384 /* floats of LDS one tile of output samples stages (64 KiB) */

/* What amx_resample_bank reports for one (orig, new, lowpass_filter_width, rolloff). */
typedef struct amx_resample_geometry {
    int64_t o, m;      /* the reduced rates */
    int64_t width;     /* W */
    int64_t taps;      /* K: the longest kept run of any phase; every phase is padded with zeros to K taps */
    int64_t bank_size; /* K * m floats (0 for o == m) */
    int64_t window;    /* input floats one kernel tile stages for this geometry: pass the largest over a launch's rows */
} amx_resample_geometry;

/* Pure host function (no device, no HIP call).  Fills `geometry`; when `bank` / `phases` are not NULL it also writes
 *   bank    float [K, m], tap-major: bank[k * m + j] = fp32(h_j[first_j + k]) for k < count_j, else 0
 *   phases  int32 [2 m]: first_j (index i of phase j's first kept tap) at [j], count_j at [m + j]
 * Call it once with NULL buffers to size them.  o == m gives K = 0, W = 0, an empty bank and no phase entries. */
int amx_resample_bank(int64_t orig_freq, int64_t new_freq, int32_t lowpass_filter_width, double rolloff,
                      amx_resample_geometry* geometry, float* bank, int32_t* phases);

/* One utterance's geometry in a launch: the fields of its amx_resample_geometry, and where its bank (in floats) and phase
 * table (in int32) start inside the `bank` and `phases` buffers given to amx_resample. */
typedef struct amx_resample_row {
    int64_t o, m, width, taps;
    int64_t bank_offset, phase_offset;
} amx_resample_row;

/* Resamples a padded fp32 batch on `device`: row n of x (element stride `stride` >= L_in between rows, unit stride in time)
 * holds lengths[n] valid samples, at most L_in; y is [N, L_out] contiguous.  y[n, t] for t < min(L_out, len'_n) is the
 * contract's output; every later sample of the row is written 0, so y may be uninitialised memory.  Input samples at or
 * past lengths[n] are never read.  All pointers except the geometry values are DEVICE pointers: lengths int64 [N],
 * rows [N], bank / phases the concatenated amx_resample_bank outputs.  `window` is the largest amx_resample_geometry.window
 * among the rows (at most AMX_RESAMPLE_MAX_WINDOW); a row whose window exceeds it comes out as NaN.
 * Limits: 0 <= N <= 65535, L_out <= 2^40.  Stream-ordered on `stream`: no allocation and no host synchronisation (the
 * launch can be captured in a graph). */
int amx_resample(int device, const float* x, int64_t stride, int64_t L_in, const int64_t* lengths, const amx_resample_row* rows,
                 const float* bank, const int32_t* phases, int64_t window, int N, int64_t L_out, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_RESAMPLE_H */
