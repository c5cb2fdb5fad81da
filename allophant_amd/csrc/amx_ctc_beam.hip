// CTC prefix beam search on the device: the reference's `BeamCTCDecoder` (predictions.py:210-235), which is torchaudio's
// flashlight `ctc_decoder` built lexicon-free with no LM (ZeroLM), blank = silence, log_add = True, beam_threshold = 50,
// every token considered per frame.  The contract restated from flashlight's LexiconFreeDecoder is in DESIGN 9 and, as
// executable code, in tests/ctc_beam_util.py; this kernel must match that restatement.
//
// One workgroup decodes one (output, utterance) row.  A state is (prefix P, last frame token k, prevBlank b) with an fp64
// score.  Per frame every (state, token) pair yields one candidate; candidates below best - 50 are dropped, equal keys merge
// by log-add (members folded in descending order, the merged state keeps the path of its highest member), and the
// beam_width best merged candidates survive.  Prefixes are identified by a 64-bit hash h' = mix(h, n): a collision between
// two prefixes of one beam is treated as impossible (2^-64 per pair and frame).
//
// Candidate reduction.  Only two states share a prefix, (P, last(P), false) and (P, blank, true), so merge groups are small:
//   plain    (P+n, n, false) from the <= 2 states of P eligible for n (n != blank, n != k or b)
//   blank    (P, blank, true) from the <= 2 states of P
//   repeat   (P, k, false) from the state itself (k != blank, !b) plus the states of P[:-1] eligible for k
// Every state adds the same e[t, n], so within one prefix the plain candidates are monotone in e[t, n].  The frame's top
// beam_width + 2 tokens are taken by (emission as added, then lower index).  A token outside them has beam_width + 2
// tokens ahead of it in that order; leaving out blank and last(P) (whose candidates may lie below), beam_width tokens m
// remain whose extension P+m is at least as high.  Where P+m is not a beam state it is a plain candidate of the same
// leader and, at an equal score, has the lower token.  Where it is a beam state the repeat candidate of that state holds
// it, and repeat candidates come first in candidate order -- they must: such a repeat can equal the plain score exactly
// (a state 37 or more below the extension vanishes in the log-add) and would otherwise lose that tie to the token off the
// list.  So the unlisted token's plain candidate has beam_width candidates ahead of it and is not enumerated.  Plain
// candidates whose key is a repeat (P+n already a beam state) are dropped; the repeat holds them.
// That leaves at most B * (B + 4) candidates per frame, whose top B are found exactly by a radix select over their
// order-preserving 64-bit keys and compacted in index order.
//
// Tie order (the rule of DESIGN 9, which tests/ctc_beam_util.py restates without reference to this file).  Candidate
// index is (kind, slot, token): one repeat candidate per state at its slot j, then the plain candidates of leader L (the
// lowest slot of its prefix) at nS + L * KS + p with the list in class order, then one blank candidate per leader.  Equal
// scores resolve by lower candidate index, and the survivors take the new slots in index order, not in score order.
// Equal members of a merged candidate resolve in push order (fold keeps the first of equal ones): leader before partner,
// and for a repeat the state itself, then the leader of P[:-1], then its partner.  The end step ranks equal merged scores
// by lower leader slot.  Frames with no finite emission, and NaN, are outside the contract.
//
// A backpointer (parent slot << 16 | frame token) per (frame, slot) goes to a caller-supplied workspace; the end step
// merges by prefix, ranks, and traces the n-best paths back into tokens and 1-based timesteps.
//
// What this decoder shares with the one that fuses a language model (amx_ctc_beam_lm.hip) is in amx_ctc_beam.inc.
#include "amx_common.h"

namespace amx {

namespace {

#include "amx_ctc_beam.inc"

constexpr int BM_KMAX = BEAM_MAX + 2;                  // tokens considered for plain extensions per frame
constexpr int BM_MMAX = BEAM_MAX * (BM_KMAX + 2);      // candidates per frame: repeat, plain, blank
constexpr int BM_TILE = BM_MMAX - BM_KMAX;             // classes whose keys are staged at a time for the token list

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

// Members of candidate i (see the header comment for the layout): their scores x and state slots, after the threshold.
__device__ __forceinline__ Members members(const BeamSmem& sm, int cur, int nS, int KS, int blank, int i, int* token) {
    Members g;
    g.m = 0;
    const double cut = sm.cut;
    if (i >= nS && i < nS + nS * KS) {
        const int L = (i - nS) / KS, p = (i - nS) - L * KS;
        const int n = sm.S[p];
        *token = n;
        if (sm.leader[L] != L || n == blank) return g;
        const double e = sm.Se[p];
        const int q = sm.partner[L];
        if (n != sm.tk[cur][L] || sm.pb[cur][L]) {
            const double v = sm.sc[cur][L] + e;
            if (v >= cut) g.push(v, L);
        }
        if (q >= 0 && (n != sm.tk[cur][q] || sm.pb[cur][q])) {
            const double v = sm.sc[cur][q] + e;
            if (v >= cut) g.push(v, q);
        }
    } else if (i >= nS) {
        const int L = i - nS - nS * KS;
        *token = blank;
        if (sm.leader[L] != L) return g;
        const double e = sm.e0;
        const int q = sm.partner[L];
        double v = sm.sc[cur][L] + e;
        if (v >= cut) g.push(v, L);
        if (q >= 0) {
            v = sm.sc[cur][q] + e;
            if (v >= cut) g.push(v, q);
        }
    } else {
        const int j = i;
        const int n = sm.tk[cur][j];
        *token = n;
        if (n == blank || sm.pb[cur][j]) return g;
        const double e = sm.ek[j];
        double v = sm.sc[cur][j] + e;
        if (v >= cut) g.push(v, j);
        const int P = sm.parent[j];
        if (P >= 0) {
            if (n != sm.tk[cur][P] || sm.pb[cur][P]) {
                v = sm.sc[cur][P] + e;
                if (v >= cut) g.push(v, P);
            }
            const int q = sm.partner[P];
            if (q >= 0 && (n != sm.tk[cur][q] || sm.pb[cur][q])) {
                v = sm.sc[cur][q] + e;
                if (v >= cut) g.push(v, q);
            }
        }
    }
    return g;
}

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
            int tok, best;
            const Members g = members(sm, cur, nS, KS, blank, i, &tok);
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
        // 5. a plain candidate onto a prefix already in the beam is that state's repeat candidate
        if (tid < nS && sm.parent[tid] >= 0 && sm.childp[tid] >= 0) {
            const int i = nS + sm.parent[tid] * KS + sm.childp[tid];
            if (sm.key[i]) {
                sm.key[i] = 0;
                atomicSub(&sm.nvalid, 1);
            }
        }
        __syncthreads();
        // 6. the top `beam` candidates, index order
        const int nvalid = sm.nvalid;
        const int nW = min(beam, nvalid);
        auto ckey = [&](int i) -> uint64_t { return sm.key[i]; };
        if (nvalid > beam) {
            radix_select<uint64_t, 64>(M, beam, ckey, sm);
        } else {
            if (tid == 0) {
                sm.sel_prefix = 0;
                sm.sel_mask = ~0ull;
                sm.sel_take = 0;
            }
            __syncthreads();
        }
        compact<uint64_t>(M, beam, ckey, [&](int pos, int i) { sm.win[pos] = i; }, sm);
        __syncthreads();
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
    }
    if (tid < 64) {
        double s = tid < nS ? sm.sc[cur][tid] : -INFINITY;
        s = wave_max_f64(s);
        if (tid == 0) sm.cut = s - BM_THRESHOLD;
    }
    __syncthreads();
    // merged value of each leader in sm.ek, its best member in sm.childp
    if (tid < nS) {
        double v = -INFINITY;
        int bs = tid, valid = 0;
        if (sm.leader[tid] == tid) {
            Members g;
            g.m = 0;
            int best;
            if (sm.sc[cur][tid] >= sm.cut) g.push(sm.sc[cur][tid], tid);
            const int q = sm.partner[tid];
            if (q >= 0 && sm.sc[cur][q] >= sm.cut) g.push(sm.sc[cur][q], q);
            if (g.m) {
                v = fold(g, &best);
                bs = best;
                valid = 1;
            }
        }
        sm.ek[tid] = v;
        sm.childp[tid] = bs;
        sm.parent[tid] = valid;
    }
    __syncthreads();
    if (tid < nS && sm.parent[tid]) {
        const double v = sm.ek[tid];
        int rank = 0;
        for (int j = 0; j < nS; ++j)
            if (sm.parent[j] && (sm.ek[j] > v || (sm.ek[j] == v && j < tid))) ++rank;
        if (rank < n_best) {
            sm.win[rank] = sm.childp[tid];
            scores[rank] = v;
        }
    }
    if (tid < 64) {
        int g = tid < nS ? sm.parent[tid] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o, 64);
        if (tid == 0) sm.nvalid = min(g, n_best);
    }
    __syncthreads();
    const int nh = sm.nvalid;
    if (tid == 0) *hyp_count = nh;
    if (tid >= nh && tid < n_best) {
        counts[tid] = 0;
        scores[tid] = -INFINITY;
    }
    trace_and_collapse(nh, len, T, beam, blank, bp, tokens, timesteps, counts, sm);
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

void launch_beam_ctc(const OutDesc* descs_dev, int n_out, const float* out, const int* frame_len, int N, int T, int beam, int n_best,
                     int exp_mode, uint32_t* ws, int64_t* tokens, int64_t* timesteps, int* counts, double* scores, int* hyp_counts,
                     hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_kernel, dim3(N, n_out), dim3(BM_THREADS), 0, s, descs_dev, out, frame_len, N, T, beam, n_best,
                       exp_mode, ws, tokens, timesteps, counts, scores, hyp_counts);
}

void launch_beam_ctc_emissions(const float* emissions, int64_t stride_n, int64_t stride_t, const int* frame_len, int N, int T, int C,
                               int blank, int beam, int n_best, int exp_mode, uint32_t* ws, int64_t* tokens, int64_t* timesteps,
                               int* counts, double* scores, int* hyp_counts, hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_emissions_kernel, dim3(N), dim3(BM_THREADS), 0, s, emissions, stride_n, stride_t, frame_len, T, C,
                       blank, beam, n_best, exp_mode, ws, tokens, timesteps, counts, scores, hyp_counts);
}

}  // namespace amx
