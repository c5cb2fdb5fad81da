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
// beam_width + 2 tokens are taken by (emission, then lower index): ties at the cut go by index, not all tied tokens (tie
// order is one of the open points of DESIGN 9).  A token outside them has beam_width + 2 tokens ahead of it; leaving out
// blank and last(P) (whose candidates may lie below), at least beam_width candidates of the same prefix are at least as
// high, so its plain candidate cannot survive except by a tie.  Plain candidates whose key is a repeat (P+n already a beam
// state) are dropped; the repeat holds them.
// That leaves at most B * (B + 4) candidates per frame, whose top B are found exactly by a radix select over their
// order-preserving 64-bit keys and compacted in index order (deterministic; equal scores resolve by candidate index).
//
// A backpointer (parent slot << 16 | frame token) per (frame, slot) goes to a caller-supplied workspace; the end step
// merges by prefix, ranks, and traces the n-best paths back into tokens and 1-based timesteps.
#include "amx_common.h"

namespace amx {

namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int BM_KMAX = BEAM_MAX + 2;                  // tokens considered for plain extensions per frame
constexpr int BM_MMAX = BEAM_MAX * (BM_KMAX + 2);      // candidates per frame: plain, blank, repeat
constexpr double BM_THRESHOLD = 50.0;                   // torchaudio's beam_threshold default
constexpr uint64_t BM_ROOT = 0x6a09e667f3bcc908ull;     // hash of the empty prefix

struct BeamSmem {
    uint64_t key[BM_MMAX];  // candidate keys of the frame (0 = no candidate): the merged fp64 score, order-preserving
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
    int S[BM_KMAX];            // the frame's top tokens, index order
    double Se[BM_KMAX];
    int win[BEAM_MAX];
    int hist[256];
    int wtmp[BM_WAVES];
    uint64_t sel_prefix, sel_mask;
    int sel_take, sel_done, nvalid, carry[2];
    double e0, cut;
};

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t extend_hash(uint64_t h, int n) { return splitmix64(h ^ ((uint64_t)(unsigned)n * 0xd6e8feb86659fd93ull)); }

// order-preserving integer images (larger float -> larger key); candidate keys are kept >= 1 so that 0 means "none"
__device__ __forceinline__ uint32_t key32(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t key64(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint64_t k = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    return k ? k : 1;
}
__device__ __forceinline__ double unkey64(uint64_t k) {
    const uint64_t sign = 0x8000000000000000ull;
    return __longlong_as_double((long long)((k & sign) ? (k ^ sign) : ~k));
}

// the emission as flashlight adds it: the fp32 value, or (EXP) its fp32 exponential -- exp in fp64 rounded once to fp32, so
// the value is the correctly rounded expf (up to a double-rounding tie)
__device__ __forceinline__ double emission(float x, bool exp_mode) { return exp_mode ? (double)(float)exp((double)x) : (double)x; }

// the members of one merge group (at most three): scores and state slots, in the order they were found
struct Members {
    double x0, x1, x2;
    int s0, s1, s2, m;
    __device__ __forceinline__ void push(double v, int slot) {
        if (m == 0) { x0 = v; s0 = slot; }
        else if (m == 1) { x1 = v; s1 = slot; }
        else { x2 = v; s2 = slot; }
        ++m;
    }
};

__device__ __forceinline__ double logadd(double a, double c) {
    const double hi = fmax(a, c), lo = fmin(a, c);
    return hi + log1p(exp(lo - hi));
}

// log-add of the members folded in descending order; *best = the slot of the highest member (the first of equal ones)
__device__ __forceinline__ double fold(Members g, int* best) {
    double a = g.x0, b = g.x1, c = g.x2;
    int sa = g.s0, sb = g.s1, sc = g.s2;
    if (g.m > 1 && b > a) { double t = a; a = b; b = t; int u = sa; sa = sb; sb = u; }
    if (g.m > 2) {
        if (c > b) { double t = b; b = c; c = t; int u = sb; sb = sc; sc = u; }
        if (b > a) { double t = a; a = b; b = t; int u = sa; sa = sb; sb = u; }
    }
    double acc = a;
#pragma nounroll
    for (int r = 1; r < g.m; ++r) acc = logadd(acc, r == 1 ? b : c);
    *best = sa;
    return acc;
}

// exclusive prefix sum over the workgroup in thread order
__device__ __forceinline__ int block_scan(int v, int* wtmp, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtmp[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < BM_WAVES; ++i) {
        const int c = wtmp[i];
        base += i < w ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// Radix select (8-bit digits from the top) of the `want` largest of n integer keys, want <= n.  Leaves in sm.sel_* the
// boundary region: keys with (key & mask) > prefix are in, of those with (key & mask) == prefix the first `take` in index
// order.  Expects sm.hist zero and leaves it zero.
template <typename K, int BITS, typename KeyF>
__device__ __forceinline__ void radix_select(int n, int want, KeyF key, BeamSmem& sm) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        sm.sel_prefix = 0;
        sm.sel_mask = 0;
        sm.sel_take = want;
        sm.sel_done = 0;
    }
    __syncthreads();
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        const K prefix = (K)sm.sel_prefix, mask = (K)sm.sel_mask;
        for (int i = tid; i < n; i += BM_THREADS) {
            const K k = key(i);
            if ((k & mask) == prefix) atomicAdd(&sm.hist[(int)(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < 64) {
            // lane l owns bins 255 - 4l .. 252 - 4l: an inclusive scan over lanes counts keys from the top
            int c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = sm.hist[255 - 4 * tid - j];
                sm.hist[255 - 4 * tid - j] = 0;
            }
            const int sum = c[0] + c[1] + c[2] + c[3];
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o, 64);
                if (tid >= o) incl += y;
            }
            const int take = sm.sel_take;
            int cum = incl - sum;
            if (cum < take && take <= incl) {
                bool found = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!found && cum + c[j] >= take) {
                        found = true;
                        sm.sel_prefix |= (uint64_t)(255 - 4 * tid - j) << shift;
                        sm.sel_mask |= (uint64_t)0xff << shift;
                        sm.sel_take = take - cum;
                        sm.sel_done = c[j] == take - cum;  // the region is taken whole: lower digits cannot change the set
                    }
                    if (!found) cum += c[j];
                }
            }
        }
        __syncthreads();
        if (sm.sel_done) break;
    }
}

// Emits the selected keys in index order: emit(position, index), positions < cap.  Each thread owns a contiguous range.
template <typename K, typename KeyF, typename EmitF>
__device__ __forceinline__ void compact(int n, int cap, KeyF key, EmitF emit, BeamSmem& sm) {
    const K prefix = (K)sm.sel_prefix, mask = (K)sm.sel_mask;
    const int take = sm.sel_take;
    const int per = (n + BM_THREADS - 1) / BM_THREADS;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int gt = 0, eq = 0;
    for (int i = lo; i < hi; ++i) {
        const K k = key(i) & mask;
        gt += k > prefix;
        eq += k == prefix;
    }
    int total;
    const int ex = block_scan((gt << 16) | eq, sm.wtmp, &total);
    int gb = ex >> 16, eb = ex & 0xffff;
    for (int i = lo; i < hi; ++i) {
        const K k = key(i) & mask;
        int pos = -1;
        if (k > prefix) {
            pos = gb + min(eb, take);
            ++gb;
        } else if (k == prefix) {
            if (eb < take) pos = gb + eb;
            ++eb;
        }
        if (pos >= 0 && pos < cap) emit(pos, i);
    }
}

// Members of candidate i (see the header comment for the layout): their scores x and state slots, after the threshold.
__device__ __forceinline__ Members members(const BeamSmem& sm, int cur, int nS, int KS, int blank, int i, int* token) {
    Members g;
    g.m = 0;
    const double cut = sm.cut;
    if (i < nS * KS) {
        const int L = i / KS, p = i - L * KS;
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
    } else if (i < nS * KS + nS) {
        const int L = i - nS * KS;
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
        const int j = i - nS * KS - nS;
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

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
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
        // 1. the frame's top KS tokens by (emission, -index)
        if (KS == C) {
            if (tid < C) sm.S[tid] = tid;
        } else {
            auto fkey = [&](int c) -> uint64_t { return ((uint64_t)key32(e[c]) << 16) | (uint64_t)(0xffffu - (unsigned)c); };
            radix_select<uint64_t, 48>(C, KS, fkey, sm);
            compact<uint64_t>(C, KS, fkey, [&](int pos, int c) { sm.S[pos] = c; }, sm);
        }
        __syncthreads();
        // 2. emissions of S, blank, per-state structure
        if (tid < KS) sm.Se[tid] = emission(e[sm.S[tid]], exp_mode);
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
                        if (sm.S[p] == k) cp = p;
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
            const int i = sm.parent[tid] * KS + sm.childp[tid];
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
            const int tok = i < nS * KS ? sm.S[i % KS] : (i < nS * KS + nS ? blank : sm.tk[cur][i - nS * KS - nS]);
            if (i < nS * KS) {
                const int L = i / KS;
                sm.hs[nxt][tid] = extend_hash(sm.hs[cur][L], tok);
                sm.ph[nxt][tid] = sm.hs[cur][L];
                sm.tk[nxt][tid] = tok;
                sm.pb[nxt][tid] = 0;
            } else if (i < nS * KS + nS) {
                const int L = i - nS * KS;
                sm.hs[nxt][tid] = sm.hs[cur][L];
                sm.ph[nxt][tid] = sm.ph[cur][L];
                sm.tk[nxt][tid] = blank;
                sm.pb[nxt][tid] = 1;
            } else {
                const int j = i - nS * KS - nS;
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
    // trace back: the frame tokens of hypothesis r go to timesteps[r, t] first
    if (tid < nh) {
        int slot = sm.win[tid];
        int64_t* raw = timesteps + (int64_t)tid * T;
        for (int t = len - 1; t >= 0; --t) {
            const uint32_t v = bp[(int64_t)t * beam + slot];
            raw[t] = (int64_t)(v & 0xffffu);
            slot = (int)(v >> 16);
        }
    }
    __syncthreads();
    // collapse in place, 4 frames per thread per chunk: non-blank tokens that differ from the previous frame's token
    constexpr int IT = 4, CH = BM_THREADS * IT;
    for (int r = 0; r < nh; ++r) {
        int64_t* tok = tokens + (int64_t)r * T;
        int64_t* ts = timesteps + (int64_t)r * T;
        int pos_base = 0;
        for (int c0 = 0, ci = 0; c0 < len; c0 += CH, ++ci) {
            const int t0 = c0 + tid * IT;
            int v[IT], prev;
            prev = tid == 0 ? (c0 == 0 ? blank : sm.carry[(ci - 1) & 1]) : (t0 - 1 < len ? (int)ts[t0 - 1] : blank);
#pragma unroll
            for (int j = 0; j < IT; ++j) v[j] = t0 + j < len ? (int)ts[t0 + j] : blank;
            if (tid == BM_THREADS - 1 && t0 + IT <= len) sm.carry[ci & 1] = v[IT - 1];  // the next chunk's first `prev`
            int cnt = 0;
            bool emit[IT];
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                emit[j] = t0 + j < len && v[j] != blank && v[j] != (j ? v[j - 1] : prev);
                cnt += emit[j];
            }
            int total;
            int pos = pos_base + block_scan(cnt, sm.wtmp, &total);
#pragma unroll
            for (int j = 0; j < IT; ++j)
                if (emit[j]) {
                    tok[pos] = v[j];
                    ts[pos] = t0 + j + 1;
                    ++pos;
                }
            pos_base += total;
        }
        if (tid == 0) counts[r] = pos_base;
        __syncthreads();
    }
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
