/* Long-recording entry points of liballophant_amx (companion of allophant_amx.h, same library, same ABI version). */
#ifndef ALLOPHANT_AMX_LONG_H
#define ALLOPHANT_AMX_LONG_H
#include "allophant_amx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A recording too long for one forward pass is predicted as overlapping WINDOWS of utterance size, and the windows' output
 * frames are stitched into the output of the recording, on the device.  Symbols added to ABI 6 without a struct change (detect
 * them with dlsym).  All three entry points know no handle; the forward pass in between is amx_forward on the gathered batch.
 *
 * Constants of a conv stack (kernel k_i, stride s_i, i < n_conv):
 *
 *   S  = prod s_i                                   the hop: samples between two frames                (wav2vec 2.0: 320)
 *   RF = 1 + sum (k_i - 1) * prod_{j < i} s_j       the receptive field of one frame, in samples       (wav2vec 2.0: 400)
 *   frames(L) = 0 if L < RF, else (L - RF) / S + 1  (equal to the per-layer formula (len - k_i) / s_i + 1 applied n_conv times)
 *
 * Frame g of a recording covers the samples [g * S, g * S + RF): a window that starts at sample a * S produces the
 * recording's frames a, a + 1, ... as its own frames 0, 1, ...
 *
 * The plan.  `window` samples per window, Wf = frames(window); `context` = c frames dropped on each inner side of a window;
 * K = Wf - 2c frames kept per inner window.  For a recording of `len` samples, T = frames(len):
 *
 *   n = 0 if T == 0, 1 if T <= Wf, else ceil((T - Wf) / K) + 1 windows; window i of them has
 *   start   = min(i * K, max(0, T - Wf))            first frame (the last window is right-aligned, not short)
 *   keep_lo = 0 if i == 0,     else i * K + c       the frames [keep_lo, keep_hi) of the recording are taken from this window;
 *   keep_hi = T if i == n - 1, else (i + 1) * K + c the kept ranges of a recording partition [0, T)
 *   samples = min(window, len - start * S)          what the window reads, starting at sample start * S
 *
 * Rows are ordered by recording, then by i. */
typedef struct amx_long_window { int32_t recording, index, start, keep_lo, keep_hi, samples; } amx_long_window; /* start / keep_* in frames */
typedef struct amx_long_block  { int64_t src_offset, dst_offset; int32_t classes; } amx_long_block;               /* offsets in floats */
#define AMX_LONG_MAX_BLOCKS 64

/* The plan of R recordings of lengths[r] samples (host arrays; pure host code, no HIP call).  Always writes *n_windows (0
 * where the arguments are refused) and, when non-NULL, frames[r] = frames(lengths[r]); windows == NULL only sizes the plan,
 * otherwise the first *n_windows entries of `windows` (room for `capacity`) are written.  AMX_EINVAL: windows non-NULL with
 * capacity < *n_windows (which is still written), window < RF or >= 2^31, K < 1, context < 0, a negative length, R < 0,
 * n_conv outside [1, AMX_MAX_CONV], a kernel or stride below 1, any frame count at or above 2^31, a null n_windows / conv
 * array / lengths (R > 0). */
int amx_long_plan(const int64_t* lengths, int R, int64_t window, int32_t context, const int32_t* conv_kernel,
                  const int32_t* conv_stride, int n_conv, amx_long_window* windows, int64_t capacity,
                  int64_t* n_windows, int64_t* frames /* [R] */);

/* The windows' audio as one padded batch.  All pointers are DEVICE pointers: audio fp32, row r at audio + r * stride;
 * lengths int64 [R]; windows [n]; batch fp32 [n, L_out] contiguous, may be uninitialised; status int32 [n].  For row w with
 * r = recording:  batch[w][s] = audio[r * stride + start * hop + s] for s < samples, and 0 for samples <= s < L_out.  No
 * sample at or past lengths[r] is read.  A row is malformed if recording is outside [0, R), start < 0, samples < 0, samples >
 * L_out or start * hop + samples > lengths[r]: status[w] = -2, the row is written as zeros and reads nothing.  Any other row
 * gets status 0.  Rows move 16 bytes per lane where audio and batch are 16-byte aligned and stride, L_out and hop are
 * multiples of 4, and 4 bytes per lane otherwise; the values are the same.
 *
 * Limits: n >= 0, R >= 0, L_out >= 0, stride >= 0, 1 <= hop < 2^31, R * stride and n * L_out below 2^63; non-null pointers
 * where n > 0; AMX_EINVAL otherwise.  n == 0 does nothing and returns AMX_OK.  Stream-ordered on `stream`: no allocation and no
 * host synchronisation, so a call can be captured in a graph. */
int amx_long_gather(int device, const float* audio, int64_t stride, const int64_t* lengths, int R,
                    const amx_long_window* windows, int n, int64_t hop, int64_t L_out, float* batch,
                    int32_t* status, void* stream);

/* The kept frames of the windows' outputs, copied into the recordings' outputs.  src, dst, windows and status are DEVICE
 * pointers; `windows` are the n rows of src, in order.  `blocks` is a HOST array whose values are captured at enqueue (they
 * travel in the kernel arguments; nothing is uploaded): block b is fp32 [src_T, n, C_b] at src + src_offset and fp32
 * [dst_T, R, C_b] at dst + dst_offset (the blocks of amx_output_layout(n, .) and of amx_output_layout(R, .)).  For every row
 * w and every g in [keep_lo, keep_hi):  dst_b[g][recording][:] = src_b[g - start][w][:].  Nothing else in dst is touched.  A
 * row is malformed if keep_lo > keep_hi, keep_lo < start, keep_lo < 0, keep_hi > start + src_T, keep_hi > dst_T or recording is
 * outside [0, R): status[w] = -2 and the row writes nothing.  Any other row gets status 0.  Rows whose kept ranges overlap in one
 * recording are the caller's error (every index stays in range).  Every offset into dst is 64-bit.  A block moves 16 bytes
 * per lane where src and dst are 16-byte aligned and C_b and both offsets are multiples of 4, and 4 bytes per lane otherwise.
 *
 * Limits: n >= 0, R >= 0, src_T >= 0, dst_T >= 0, 0 <= n_blocks <= AMX_LONG_MAX_BLOCKS (the caller calls again for the rest),
 * C_b >= 1, src_T * C_b below 2^31, offsets >= 0, the extent of every block below 2^62 floats; non-null pointers where there
 * is work; AMX_EINVAL otherwise.  n == 0 or n_blocks == 0 does nothing (status included) and returns AMX_OK.  Stream-ordered
 * on `stream`: no allocation and no host synchronisation, so a call can be captured in a graph. */
int amx_long_stitch(int device, const float* src, int64_t src_T, int n, const amx_long_window* windows,
                    const amx_long_block* blocks, int n_blocks, float* dst, int R, int64_t dst_T,
                    int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOPHANT_AMX_LONG_H */
