// CTC prefix beam search with shallow fusion of a token-level bigram language model (flashlight's LexiconFreeDecoder with
// an LM instead of ZeroLM): the decoder of amx_ctc_beam.hip, whose every new token n after a prefix P additionally costs
// a = w * lm[last(P), n] + beta, and whose end step adds w * lm[last(P), end].  The contract is in DESIGN 9 and, as
// executable code, in tests/ctc_beam_lm_util.py; this kernel must match that restatement.  States, merging, thresholds, the
// end step, backpointers and outputs are those of amx_ctc_beam.hip (described, with the shared pieces, in amx_ctc_beam.inc).
//
// One workgroup decodes one row under the table lm[lm_index[row]] ([C + 1, C + 1] fp32: row = previous token, C = begin;
// column = next token, C = end; the blank's row and column are never read).  An index of -1 runs the row with a = 0 and no
// end term, which is the decoder without a language model, bit for bit.  An -inf entry forbids its transition at every
// weight: the candidate is not generated.
//
// Candidate reduction.  Without an LM every state adds the same e[t, n], and one list of the frame's top tokens serves all
// prefixes.  Here a prefix P adds g_P(n) = e[t, n] + a_P(n), so each prefix leader keeps its OWN top min(beam + 2, C)
// non-blank tokens by (g_P, then lower index), g_P being the fp64 sum of the emission as added and a.  A token outside
// that list has beam + 2 tokens of the same prefix ahead of it; leaving out last(P) (whose candidate may lie below), at
// least beam tokens m remain whose extension P+m is at least as high: a plain candidate of the same leader with the lower
// token, or, where P+m is a beam state, that state's repeat candidate, which comes first in candidate order (see
// amx_ctc_beam.inc for why it must, and for the tie order).  So the token's plain candidate cannot survive and is not
// enumerated.  Plain candidates whose key is already a beam state go to that state's repeat candidate whether or not the
// token is in the list (the repeat branch of members()).  That leaves at most B * (B + 4) candidates per frame, as
// without an LM.
//
// The per-prefix selection is the hot loop: one wave per prefix, classes across lanes (the table row is read as contiguous
// 4-byte values), in ONE pass over the classes.  A lane whose key beats the running threshold appends it to a per-wave
// buffer in class order; when the buffer cannot take another 64 the wave keeps its top K by a bitwise radix select over
// the (at most 192) buffered keys held in registers -- ballots and popcounts, no atomics -- and the K-th key becomes the
// threshold.  The frame's emissions (exponentiated once under EXP) are staged in LDS for all prefixes.
//
// The frame's best, for the threshold of 50, is the maximum over the generated candidates with `a` included: every state
// against every token of its prefix's list, its blank and its repeat candidate.
#include "amx_common.h"

namespace amx {

namespace {

#include "amx_ctc_beam.inc"

constexpr int BL_WCAP = 192;                        // per-wave selection buffer: three keys per lane

struct BeamLmSmem {
    uint64_t key[BM_MMAX];            // candidate keys of the frame (0 = no candidate)
    double la[BEAM_MAX][BM_KMAX];     // per prefix leader and list position: a = w * lm + beta
    float le[BEAM_MAX][BM_KMAX];      //   the emission as added (an fp32 value in both modes)
    uint16_t ltok[BEAM_MAX][BM_KMAX]; //   the token, class order
    uint64_t wk[BM_WAVES][BL_WCAP];   // per-wave selection buffer: keys of g_P, class order
    uint16_t wt[BM_WAVES][BL_WCAP];
    float ef[BEAM_LM_MAX_CLASSES + 1];  // the frame's emissions as added
    uint8_t par[BM_MMAX];             // slot of the candidate's highest member
    double sc[2][BEAM_MAX];
    uint64_t hs[2][BEAM_MAX];  // prefix hash
    uint64_t ph[2][BEAM_MAX];  // hash of the prefix without its last token (read for non-blank states only)
    int tk[2][BEAM_MAX];       // last frame token
    int pb[2][BEAM_MAX];       // prevBlank
    int lt[2][BEAM_MAX];       // last token of the prefix, C for the empty prefix: the table row
    int partner[BEAM_MAX];     // for a group leader (lowest slot of its prefix): the other state of the prefix, or -1
    int leader[BEAM_MAX];
    int parent[BEAM_MAX];      // for a non-blank state: leader of P[:-1] in the beam, or -1 (also when P[:-1] may not emit k)
    int childp[BEAM_MAX];      // its last token's position in the parent's list, or -1
    int nl[BEAM_MAX];          // list length of a leader
    double ek[BEAM_MAX];       // e[t, k] of a non-blank state
    double ak[BEAM_MAX];       // a of P[:-1] emitting k
    double wmax[BM_WAVES];
    int win[BEAM_MAX];
    int hist[256];
    int wtmp[BM_WAVES];
    uint64_t sel_prefix, sel_mask;
    int sel_take, sel_done, nvalid, carry[2];
    double e0;
};
static_assert(sizeof(BeamLmSmem) <= 160 * 1024, "one workgroup per CU: 160 KiB of LDS");

// a = w * lm + beta in two roundings (no fused multiply-add), as the restatement computes it
__device__ __forceinline__ double lm_term(double w, float v, double beta) { return __dadd_rn(__dmul_rn(w, (double)v), beta); }

// LDS written by some lanes of this wave is read by others: orders the accesses (a wave's LDS operations execute in order)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Keeps the `want` largest of the cnt buffered keys (want < cnt <= BL_WCAP), equal keys by lower position, in position
// order, and returns the smallest key kept.  Wave-uniform control flow; the keys live in three registers per lane.
__device__ __forceinline__ uint64_t wave_keep_top(uint64_t* wk, uint16_t* wt, int cnt, int want, int lane, uint64_t below) {
    uint64_t k[3];
    uint16_t t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int j = lane + 64 * r;
        k[r] = j < cnt ? wk[j] : 0;
        t[r] = j < cnt ? wt[j] : 0;
    }
    // bit by bit from the top: the region is {key & mask == prefix}, of which `take` are still to be chosen
    uint64_t prefix = 0, mask = 0;
    int take = want, region = cnt;
    for (int bit = 63; bit >= 0 && region != take; --bit) {
        const uint64_t b = 1ull << bit, m = mask | b, p1 = prefix | b;
        int n1 = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) n1 += __popcll(__ballot((k[r] & m) == p1));
        if (n1 >= take) {
            prefix = p1;
            region = n1;
        } else {
            take -= n1;
            region -= n1;
        }
        mask = m;
    }
    int base = 0, eq_base = 0, pos[3];
    bool in[3];
    uint64_t low = ~0ull;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint64_t km = k[r] & mask;
        const bool eq = k[r] != 0 && km == prefix;
        const uint64_t eqm = __ballot(eq);
        const int eq_rank = eq_base + __popcll(eqm & below);
        eq_base += __popcll(eqm);
        in[r] = (k[r] != 0 && km > prefix) || (eq && eq_rank < take);
        const uint64_t inm = __ballot(in[r]);
        pos[r] = base + __popcll(inm & below);
        base += __popcll(inm);
        if (in[r] && k[r] < low) low = k[r];
    }
    wave_sync();  // every lane has its keys in registers before any position is overwritten
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (in[r]) {
            wk[pos[r]] = k[r];
            wt[pos[r]] = t[r];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(low, o, 64);
        low = other < low ? other : low;
    }
    wave_sync();
    return low;
}

// The list of prefix leader L, by this wave: the top KS non-blank tokens by (g = e + a, lower index), transitions with an
// -inf table entry left out.  lmrow = the table row of last(P), or null (a = 0).
__device__ __forceinline__ void prefix_list(BeamLmSmem& sm, const float* __restrict__ lmrow, double w, double beta, int C, int blank,
                                            int KS, int L) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1;
    uint64_t* wk = sm.wk[wv];
    uint16_t* wt = sm.wt[wv];
    int cnt = 0;
    uint64_t tau = 0;  // a key must exceed it (an equal one comes later in class order and loses)
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        uint64_t k = 0;
        if (c < C && c != blank) {
            double a = 0.0;
            bool ok = true;
            if (lmrow) {
                const float v = lmrow[c];
                ok = v != -INFINITY;
                a = lm_term(w, v, beta);
            }
            if (ok) k = key64((double)sm.ef[c] + a);
        }
        const bool take = k > tau;
        const uint64_t m = __ballot(take);
        if (m) {
            if (take) {
                const int pos = cnt + __popcll(m & below);
                wk[pos] = k;
                wt[pos] = (uint16_t)c;
            }
            cnt += __popcll(m);
            if (cnt > BL_WCAP - 64) {
                wave_sync();
                tau = wave_keep_top(wk, wt, cnt, KS, lane, below);
                cnt = KS;
            }
        }
    }
    wave_sync();
    if (cnt > KS) {
        wave_keep_top(wk, wt, cnt, KS, lane, below);
        cnt = KS;
    }
    for (int p = lane; p < cnt; p += 64) {
        const int n = wt[p];
        sm.ltok[L][p] = (uint16_t)n;
        sm.le[L][p] = sm.ef[n];
        sm.la[L][p] = lmrow ? lm_term(w, lmrow[n], beta) : 0.0;
    }
    if (lane == 0) sm.nl[L] = cnt;
    wave_sync();  // the buffer is free for the wave's next prefix
}

// The decoder policy (amx_ctc_beam.inc).  What a new token adds: its emission and a, from the list of its prefix leader.
struct LmDecoder {
    struct Term {
        double e, a;
    };
    static __device__ __forceinline__ bool plain(const BeamLmSmem& sm, int L, int p, int, int* n, Term* x) {
        if (sm.leader[L] != L || p >= sm.nl[L]) return false;
        *n = sm.ltok[L][p];
        x->e = (double)sm.le[L][p];
        x->a = sm.la[L][p];
        return true;
    }
    static __device__ __forceinline__ Term repeat(const BeamLmSmem& sm, int j, double e) { return {e, sm.ak[j]}; }
    static __device__ __forceinline__ double add(double s, Term x) { return (s + x.e) + x.a; }
    // the end step: the end totals are in sm.ak, -inf for a state that is dropped
    static __device__ __forceinline__ double total(const BeamLmSmem& sm, int, int slot) { return sm.ak[slot]; }
    static __device__ __forceinline__ bool ends(double x) { return x > -INFINITY; }
};

// workgroup maximum of v; every thread gets it
__device__ __forceinline__ double block_max(double v, BeamLmSmem& sm) {
    v = wave_max_f64(v);
    if ((threadIdx.x & 63) == 0) sm.wmax[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = sm.wmax[0];
#pragma unroll
    for (int i = 1; i < BM_WAVES; ++i) m = fmax(m, sm.wmax[i]);
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(BM_THREADS) void beam_ctc_lm_kernel(
    const float* __restrict__ emissions, int64_t stride_n, int64_t stride_t, const int* __restrict__ frame_len, int T, int C,
    int blank, int beam, int n_best, int exp_flag, const float* __restrict__ lm, int n_lm, const int* __restrict__ lm_index,
    double w, double beta, uint32_t* __restrict__ ws, int64_t* __restrict__ tokens_all, int64_t* __restrict__ timesteps_all,
    int* __restrict__ counts_all, double* __restrict__ scores_all, int* __restrict__ hyp_counts) {
    __shared__ BeamLmSmem sm;
    const int tid = threadIdx.x, wv = tid >> 6;
    const int64_t row_n = blockIdx.x;
    const int len = max(0, min(frame_len[row_n], T));
    const bool exp_mode = exp_flag != 0;
    const float* __restrict__ row = emissions + row_n * stride_n;
    uint32_t* __restrict__ bp = ws + row_n * T * beam;
    int64_t* __restrict__ tokens = tokens_all + row_n * n_best * T;
    int64_t* __restrict__ timesteps = timesteps_all + row_n * n_best * T;
    int* __restrict__ counts = counts_all + row_n * n_best;
    double* __restrict__ scores = scores_all + row_n * n_best;
    const int index = lm_index[row_n];
    if (index < -1 || index >= n_lm) {  // not a table of the stack: the row has no hypotheses
        if (tid == 0) hyp_counts[row_n] = 0;
        if (tid < n_best) {
            counts[tid] = 0;
            scores[tid] = -INFINITY;
        }
        return;
    }
    const int W = C + 1;
    const float* __restrict__ table = index >= 0 ? lm + (int64_t)index * W * W : nullptr;

    sm.hist[tid] = 0;
    if (tid == 0) {
        sm.sc[0][0] = 0.0;
        sm.hs[0][0] = BM_ROOT;
        sm.ph[0][0] = BM_ROOT;
        sm.tk[0][0] = blank;
        sm.pb[0][0] = 0;
        sm.lt[0][0] = C;
    }
    __syncthreads();
    int cur = 0, nS = 1;
    const int KS = min(beam + 2, C);
    for (int t = 0; t < len; ++t) {
        const float* e = row + (int64_t)t * stride_t;
        // 1. the frame's emissions as added, per-state structure
        for (int c = tid; c < C; c += BM_THREADS) sm.ef[c] = (float)emission(e[c], exp_mode);
        group_prefixes(sm, cur, nS);
        if (tid < nS) {
            int P = -1;
            const int k = sm.tk[cur][tid];
            if (k != blank && !sm.pb[cur][tid]) {
                const uint64_t ph = sm.ph[cur][tid];
                for (int j = nS - 1; j >= 0; --j)
                    if (sm.hs[cur][j] == ph) P = j;
                double a = 0.0;
                if (P >= 0 && table) {
                    const float v = table[(int64_t)sm.lt[cur][P] * W + k];
                    a = lm_term(w, v, beta);
                    if (v == -INFINITY) P = -1;
                }
                sm.ak[tid] = a;
            }
            sm.parent[tid] = P;
        }
        __syncthreads();
        // 2. one wave per prefix: its list
        for (int L = wv; L < nS; L += BM_WAVES)
            if (sm.leader[L] == L) prefix_list(sm, table ? table + (int64_t)sm.lt[cur][L] * W : nullptr, w, beta, C, blank, KS, L);
        if (tid < nS) {
            const int k = sm.tk[cur][tid];
            if (k != blank && !sm.pb[cur][tid]) sm.ek[tid] = (double)sm.ef[k];
        }
        if (tid == BM_THREADS - 1) {
            sm.e0 = (double)sm.ef[blank];
            sm.nvalid = 0;
        }
        __syncthreads();
        // 3. threshold: the best generated candidate, a included; position of each state's last token in its parent's list
        if (tid < nS) {
            int cp = -1;
            const int P = sm.parent[tid];
            if (P >= 0) {
                const int k = sm.tk[cur][tid];
                for (int p = 0; p < sm.nl[P]; ++p)
                    if (sm.ltok[P][p] == k) cp = p;
            }
            sm.childp[tid] = cp;
        }
        double best = -INFINITY;
        for (int i = tid; i < nS * KS; i += BM_THREADS) {
            const int j = i / KS, p = i - j * KS, L = sm.leader[j];
            if (p < sm.nl[L]) {
                const int n = sm.ltok[L][p];
                if (n != sm.tk[cur][j] || sm.pb[cur][j]) best = fmax(best, (sm.sc[cur][j] + (double)sm.le[L][p]) + sm.la[L][p]);
            }
        }
        if (tid < nS) {
            best = fmax(best, sm.sc[cur][tid] + sm.e0);
            if (sm.tk[cur][tid] != blank && !sm.pb[cur][tid]) best = fmax(best, sm.sc[cur][tid] + sm.ek[tid]);
        }
        const double cut = block_max(best, sm) - BM_THRESHOLD;
        // 4. candidate keys
        const int M = nS * (KS + 2);
        int valid = 0;
        for (int i = tid; i < M; i += BM_THREADS) {
            int bs;
            const Members g = members<LmDecoder>(sm, cur, nS, KS, blank, cut, i);
            uint64_t k = 0;
            if (g.m) {
                k = key64(fold(g, &bs));
                sm.par[i] = (uint8_t)bs;
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
            int tok;
            if (i >= nS && i < nS + nS * KS) {
                const int L = (i - nS) / KS;
                tok = sm.ltok[L][(i - nS) - L * KS];
                sm.hs[nxt][tid] = extend_hash(sm.hs[cur][L], tok);
                sm.ph[nxt][tid] = sm.hs[cur][L];
                sm.tk[nxt][tid] = tok;
                sm.pb[nxt][tid] = 0;
                sm.lt[nxt][tid] = tok;
            } else if (i >= nS) {
                const int L = i - nS - nS * KS;
                tok = blank;
                sm.hs[nxt][tid] = sm.hs[cur][L];
                sm.ph[nxt][tid] = sm.ph[cur][L];
                sm.tk[nxt][tid] = blank;
                sm.pb[nxt][tid] = 1;
                sm.lt[nxt][tid] = sm.lt[cur][L];
            } else {
                const int j = i;
                tok = sm.tk[cur][j];
                sm.hs[nxt][tid] = sm.hs[cur][j];
                sm.ph[nxt][tid] = sm.ph[cur][j];
                sm.tk[nxt][tid] = tok;
                sm.pb[nxt][tid] = 0;
                sm.lt[nxt][tid] = sm.lt[cur][j];
            }
            sm.sc[nxt][tid] = v;
            bp[(int64_t)t * beam + tid] = ((uint32_t)par << 16) | (uint32_t)tok;
        }
        __syncthreads();
        cur = nxt;
        nS = nW;
    }

    // End: every state becomes (P, blank, false, s + w * lm[last(P), end]), an -inf entry drops it; threshold against the
    // best of them; merge by prefix; rank.  The end totals go to sm.ak, -inf for a dropped state.
    group_prefixes(sm, cur, nS);
    double fin = -INFINITY;
    if (tid < nS) {
        fin = sm.sc[cur][tid];
        if (table) {
            const float v = table[(int64_t)sm.lt[cur][tid] * W + C];
            fin = v == -INFINITY ? -INFINITY : fin + __dmul_rn(w, (double)v);
        }
        sm.ak[tid] = fin;
    }
    const double cut = block_max(fin, sm) - BM_THRESHOLD;
    end_merge<LmDecoder>(sm, cur, nS, cut, n_best, len, T, beam, blank, bp, tokens, timesteps, counts, scores, hyp_counts + row_n);
}

}  // namespace

void launch_beam_ctc_lm_emissions(const BeamLmArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_lm_kernel, dim3(a.N), dim3(BM_THREADS), 0, s, a.emissions, a.stride_n, a.stride_t, a.frame_lengths,
                       a.T, a.C, a.blank, a.beam, a.n_best, a.exp_mode, a.lm, a.n_lm, a.lm_index, a.lm_weight, a.token_score,
                       a.workspace, a.tokens, a.timesteps, a.counts, a.scores, a.hyp_counts);
}

}  // namespace amx
