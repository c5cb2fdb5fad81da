// CTC prefix beam search on the device: the reference's `BeamCTCDecoder` (predictions.py:210-235), which is torchaudio's
// flashlight `ctc_decoder` built lexicon-free with no LM (ZeroLM), blank = silence, log_add = True, beam_threshold = 50,
// every token considered per frame.  The contract restated from flashlight's LexiconFreeDecoder is in DESIGN 9 and, as
// executable code, in tests/ctc_beam_util.py; this kernel must match that restatement.
//
// One workgroup decodes one (output, utterance) row.  States, candidates, merging, the tie order, backpointers and the end
// step are described in amx_ctc_beam.inc, which holds what this decoder shares with the one that fuses a language model
// (amx_ctc_beam_lm.hip).
//
// Candidate reduction.  Every state adds the same e[t, n], so within one prefix the plain candidates are monotone in
// e[t, n], and one list serves all prefixes: the frame's top beam_width + 2 tokens by (emission as added, then lower
// index).  A token outside them has beam_width + 2 tokens ahead of it in that order; leaving out blank and last(P) (whose
// candidates may lie below), beam_width tokens m remain whose extension P+m is at least as high.  Where P+m is not a beam
// state it is a plain candidate of the same leader and, at an equal score, has the lower token.  Where it is a beam state
// the repeat candidate of that state holds it, and repeat candidates come first in candidate order.  So the unlisted
// token's plain candidate has beam_width candidates ahead of it and is not enumerated.
//
// The frame's best, for the threshold of 50, is the maximum over all (state, token) of s + e = max s + max e.
#include "amx_common.h"

namespace amx {

namespace {

#include "amx_ctc_beam.inc"

constexpr int BM_TILE = BM_MMAX - BM_KMAX;  // classes whose keys are staged at a time for the token list

struct BeamSmem {
    uint64_t key[BM_MMAX];  // candidate keys of the frame (0 = no candidate): the merged fp64 score, order-preserving;
                            // before that, the staged token-list keys of step 1
    uint8_t par[BM_MMAX];   // slot of the candidate's highest member
    double sc[2][BEAM_MAX];
    uint64_t hs[2][BEAM_MAX];  // prefix hash
    uint64_t ph[2][BEAM_MAX];  // hash of the prefix without its last token (read for non-blank states only)
    int tk[2][BEAM_MAX];       // last frame token
    int pb[2][BEAM_MAX];       // prevBlank
    int partner[BEAM_MAX];     // for a group leader (lowest slot of its prefix): the other state of the prefix, or -1
    int leader[BEAM_MAX];
    int parent[BEAM_MAX];      // for a non-blank state: leader of P[:-1] in the beam, or -1
    int childp[BEAM_MAX];      // its last token's position in S, or -1
    double ek[BEAM_MAX];       // e[t, k] of a non-blank state
    uint64_t Sk[BM_KMAX];      // the frame's top tokens, index order: their token-list keys,
    int S[BM_KMAX];            //   the tokens
    double Se[BM_KMAX];        //   and their emissions as added
    int win[BEAM_MAX];
    int hist[256];
    int wtmp[BM_WAVES];
    uint64_t sel_prefix, sel_mask;
    int sel_take, sel_done, nvalid, carry[2];
    double e0, cut;
};

// The decoder policy (amx_ctc_beam.inc).  What a new token adds: its emission, from the frame's one list (which may hold
// the blank).
struct PlainDecoder {
    struct Term {
        double e;
    };
    static __device__ __forceinline__ bool plain(const BeamSmem& sm, int L, int p, int blank, int* n, Term* x) {
        *n = sm.S[p];
        if (sm.leader[L] != L || *n == blank) return false;
        x->e = sm.Se[p];
        return true;
    }
    static __device__ __forceinline__ Term repeat(const BeamSmem&, int, double e) { return {e}; }
    static __device__ __forceinline__ double add(double s, Term x) { return s + x.e; }
    // the end step: a state's end total is its score, and every state takes part
    static __device__ __forceinline__ double total(const BeamSmem& sm, int cur, int slot) { return sm.sc[cur][slot]; }
    static __device__ __forceinline__ bool ends(double) { return true; }
};

// One row: frame t's C emissions at row + t * stride_t.  Outputs: tokens / timesteps [n_best, T], counts / scores [n_best],
// *hyp_count; bp [T, beam] of the workspace.
__device__ __forceinline__ void beam_row(const float* __restrict__ row, int64_t stride_t, int C, int T, int len, int blank, int beam, int n_best,
                         bool exp_mode, uint32_t* __restrict__ bp, int64_t* __restrict__ tokens, int64_t* __restrict__ timesteps,
                         int* __restrict__ counts, double* __restrict__ scores, int* __restrict__ hyp_count, BeamSmem& sm) {
    const int tid = threadIdx.x;
    sm.hist[tid] = 0;
    if (tid == 0) {
        sm.sc[0][0] = 0.0;
        sm.hs[0][0] = BM_ROOT;
        sm.ph[0][0] = BM_ROOT;
        sm.tk[0][0] = blank;
        sm.pb[0][0] = 0;
    }
    __syncthreads();
    int cur = 0, nS = 1;
    const int KS = min(beam + 2, C);
    for (int t = 0; t < len; ++t) {
        const float* e = row + (int64_t)t * stride_t;
        // 1. the frame's top KS tokens by (emission as added, then lower index), in class order.  Under EXP the value as
        // added is the fp32 exponential, one value for every raw emission below about -104 and for neighbours that round
        // together: the raw value would rank tokens that the candidates cannot tell apart, and differently from the decoder
        // with a language model.  Each class is converted once: its key (value image << 16 | 0xffff - class) is staged in
        // sm.key, which is free until step 4, a tile of classes at a time behind the winners of the tiles before.  (+ 0.0f:
        // -0.0f and 0.0f are one value and must be one key.  sm.ek and sm.e0 of step 2 keep the sign of a raw -0.0f, which
        // no sum shows: the scores they are added to are never -0.0.)
        int nb = 0;
        for (int c0 = 0; c0 < C; c0 += BM_TILE) {
            const int n = min(BM_TILE, C - c0);
            uint64_t* dst = KS == C ? sm.Sk : sm.key + nb;  // KS == C: every class, nothing to select
            if (tid < nb) sm.key[tid] = sm.Sk[tid];
            for (int i = tid; i < n; i += BM_THREADS) {
                const int c = c0 + i;
                dst[i] = ((uint64_t)key32((float)emission(e[c], exp_mode) + 0.0f) << 16) | (uint64_t)(0xffffu - (unsigned)c);
            }
            if (KS == C) {
                __syncthreads();
                break;
            }
            const int tot = nb + n;  // > KS
            auto fkey = [&](int i) -> uint64_t { return sm.key[i]; };
            radix_select<uint64_t, 48>(tot, KS, fkey, sm);  // (begins with a barrier: the staged keys are visible)
            compact<uint64_t>(tot, KS, fkey, [&](int pos, int i) { sm.Sk[pos] = sm.key[i]; }, sm);
            __syncthreads();
            nb = KS;
        }
        // 2. tokens and emissions of S, the blank's emission, per-state structure
        if (tid < KS) {
            const uint64_t k = sm.Sk[tid];
            sm.S[tid] = 0xffff - (int)(k & 0xffffu);
            sm.Se[tid] = (double)unkey32((uint32_t)(k >> 16));
        }
        if (tid == BM_THREADS - 1) sm.e0 = emission(e[blank], exp_mode);
        if (tid < nS) {
            const uint64_t h = sm.hs[cur][tid];
            int ld = tid, pt = -1;
            for (int j = 0; j < nS; ++j)
                if (sm.hs[cur][j] == h) {
                    if (j < ld) ld = j;
                    if (j != tid) pt = j;
                }
            sm.leader[tid] = ld;
            sm.partner[tid] = pt;
            int P = -1, cp = -1;
            const int k = sm.tk[cur][tid];
            if (k != blank && !sm.pb[cur][tid]) {
                const uint64_t ph = sm.ph[cur][tid];
                for (int j = nS - 1; j >= 0; --j)
                    if (sm.hs[cur][j] == ph) P = j;
                if (P >= 0)
                    for (int p = 0; p < KS; ++p)
                        if (0xffff - (int)(sm.Sk[p] & 0xffffu) == k) cp = p;
                sm.ek[tid] = emission(e[k], exp_mode);
            }
            sm.parent[tid] = P;
            sm.childp[tid] = cp;
        }
        __syncthreads();
        // 3. threshold: best = max over all (state, token) of s + e = max s + max e
        if (tid < 64) {
            double sm_ = tid < nS ? sm.sc[cur][tid] : -INFINITY;
            double em = tid < KS ? sm.Se[tid] : -INFINITY;
            if (tid + 64 < KS) em = fmax(em, sm.Se[tid + 64]);
            sm_ = wave_max_f64(sm_);
            em = wave_max_f64(em);
            if (tid == 0) {
                sm.cut = (sm_ + em) - BM_THRESHOLD;
                sm.nvalid = 0;
            }
        }
        __syncthreads();
        // 4. candidate keys
        const int M = nS * (KS + 2);
        int valid = 0;
        for (int i = tid; i < M; i += BM_THREADS) {
            int best;
            const Members g = members<PlainDecoder>(sm, cur, nS, KS, blank, sm.cut, i);
            uint64_t k = 0;
            if (g.m) {
                k = key64(fold(g, &best));
                sm.par[i] = (uint8_t)best;
                ++valid;
            }
            sm.key[i] = k;
        }
        if (valid) atomicAdd(&sm.nvalid, valid);
        __syncthreads();
        const int nW = select_candidates(sm, nS, KS, beam);  // steps 5 and 6
        // 7. the new states and their backpointers
        const int nxt = cur ^ 1;
        if (tid < nW) {
            const int i = sm.win[tid];
            const double v = unkey64(sm.key[i]);
            const int par = sm.par[i];
            const int tok = i < nS ? sm.tk[cur][i] : (i < nS + nS * KS ? sm.S[(i - nS) % KS] : blank);
            if (i >= nS && i < nS + nS * KS) {
                const int L = (i - nS) / KS;
                sm.hs[nxt][tid] = extend_hash(sm.hs[cur][L], tok);
                sm.ph[nxt][tid] = sm.hs[cur][L];
                sm.tk[nxt][tid] = tok;
                sm.pb[nxt][tid] = 0;
            } else if (i >= nS) {
                const int L = i - nS - nS * KS;
                sm.hs[nxt][tid] = sm.hs[cur][L];
                sm.ph[nxt][tid] = sm.ph[cur][L];
                sm.tk[nxt][tid] = blank;
                sm.pb[nxt][tid] = 1;
            } else {
                const int j = i;
                sm.hs[nxt][tid] = sm.hs[cur][j];
                sm.ph[nxt][tid] = sm.ph[cur][j];
                sm.tk[nxt][tid] = tok;
                sm.pb[nxt][tid] = 0;
            }
            sm.sc[nxt][tid] = v;
            bp[(int64_t)t * beam + tid] = ((uint32_t)par << 16) | (uint32_t)tok;
        }
        __syncthreads();
        cur = nxt;
        nS = nW;
    }

    // End: every state becomes (P, blank, false, s); threshold against the best state; merge by prefix; rank.
    group_prefixes(sm, cur, nS);
    if (tid < 64) {
        double s = tid < nS ? sm.sc[cur][tid] : -INFINITY;
        s = wave_max_f64(s);
        if (tid == 0) sm.cut = s - BM_THRESHOLD;
    }
    __syncthreads();
    end_merge<PlainDecoder>(sm, cur, nS, sm.cut, n_best, len, T, beam, blank, bp, tokens, timesteps, counts, scores, hyp_count);
}

__global__ __launch_bounds__(BM_THREADS) void beam_ctc_kernel(const OutDesc* __restrict__ descs, const float* __restrict__ out,
                                                              const int* __restrict__ frame_len, int N, int T, int beam, int n_best,
                                                              int exp_mode, uint32_t* __restrict__ ws, int64_t* __restrict__ tokens,
                                                              int64_t* __restrict__ timesteps, int* __restrict__ counts,
                                                              double* __restrict__ scores, int* __restrict__ hyp_counts) {
    __shared__ BeamSmem sm;
    const int o = blockIdx.y, n = blockIdx.x;
    const OutDesc d = descs[o];
    const int64_t r = (int64_t)o * N + n;
    const int len = max(0, min(frame_len[n], T));
    beam_row(out + (int64_t)T * N * d.prefix + (int64_t)n * d.C, (int64_t)N * d.C, d.C, T, len, 0, beam, n_best, exp_mode != 0,
             ws + r * T * beam, tokens + r * n_best * T, timesteps + r * n_best * T, counts + r * n_best, scores + r * n_best,
             hyp_counts + r, sm);
}

__global__ __launch_bounds__(BM_THREADS) void beam_ctc_emissions_kernel(
    const float* __restrict__ emissions, int64_t stride_n, int64_t stride_t, const int* __restrict__ frame_len, int T, int C,
    int blank, int beam, int n_best, int exp_mode, uint32_t* __restrict__ ws, int64_t* __restrict__ tokens,
    int64_t* __restrict__ timesteps, int* __restrict__ counts, double* __restrict__ scores, int* __restrict__ hyp_counts) {
    __shared__ BeamSmem sm;
    const int64_t n = blockIdx.x;
    const int len = max(0, min(frame_len[n], T));
    beam_row(emissions + n * stride_n, stride_t, C, T, len, blank, beam, n_best, exp_mode != 0, ws + n * T * beam,
             tokens + n * n_best * T, timesteps + n * n_best * T, counts + n * n_best, scores + n * n_best, hyp_counts + n, sm);
}

}  // namespace

void launch_beam_ctc(const BeamArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_kernel, dim3(a.N, a.n_out), dim3(BM_THREADS), 0, s, a.descs, a.emissions, a.frame_lengths, a.N, a.T,
                       a.beam, a.n_best, a.exp_mode, a.workspace, a.tokens, a.timesteps, a.counts, a.scores, a.hyp_counts);
}

void launch_beam_ctc_emissions(const BeamArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_emissions_kernel, dim3(a.N), dim3(BM_THREADS), 0, s, a.emissions, a.stride_n, a.stride_t,
                       a.frame_lengths, a.T, a.C, a.blank, a.beam, a.n_best, a.exp_mode, a.workspace, a.tokens, a.timesteps,
                       a.counts, a.scores, a.hyp_counts);
}

}  // namespace amx
