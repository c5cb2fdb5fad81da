// What the two CTC beam-search kernels share (amx_ctc_beam.hip, the decoder without a language model, and
// amx_ctc_beam_lm.hip, the one with a phonotactic bigram): prefix hashes, the order-preserving key images, the grouping
// of states by prefix, the members of a candidate and their merge, the workgroup scan, the exact radix select with its
// compaction, steps 5 and 6 of a frame, and the end step behind its threshold with the trace and collapse.  Included
// inside namespace amx { namespace { ... } } by each of them.  The templates take the including file's shared-memory
// struct `Smem`, of which they use the per-state fields (sc hs ph tk pb partner leader parent childp ek) and the frame's
// candidates and scratch (key par win hist wtmp sel_* nvalid carry e0); the two structs hold these fields in different
// orders, each the one its kernel's register allocation was found with.  What differs between the decoders the templates
// take as a decoder policy `D`, all static and inlined, so that the decoder without a language model carries none of the
// other's terms (see members and end_merge).  Each kernel keeps its own LDS struct, token lists, threshold, step 4's
// loop and step 7: written as shared functions these change the kernels' frame loops, and the loops as they are
// compile to the instructions they had before anything was shared.
//
// A state is (prefix P, last frame token k, prevBlank b) with an fp64 score.  Per frame every (state, token) pair yields
// one candidate; candidates below best - 50 are dropped, equal keys merge by log-add (members folded in descending order,
// the merged state keeps the path of its highest member), and the beam_width best merged candidates survive.  Prefixes are
// identified by a 64-bit hash h' = mix(h, n): a collision between two prefixes of one beam is treated as impossible
// (2^-64 per pair and frame).
//
// Candidates.  Only two states share a prefix, (P, last(P), false) and (P, blank, true), so merge groups are small:
//   repeat   (P, k, false) from the state itself (k != blank, !b) plus the states of P[:-1] eligible for k
//   plain    (P+n, n, false) from the <= 2 states of P eligible for n (n != blank, n != k or b)
//   blank    (P, blank, true) from the <= 2 states of P
// Plain candidates are enumerated for the tokens of a list of KS = min(beam_width + 2, C) only; why no other token can
// survive is each decoder's own argument, at the head of its file.  Plain candidates whose key is a repeat (P+n already a
// beam state) are dropped; the repeat holds them.  That leaves at most B * (B + 4) candidates per frame, whose top B are
// found exactly by a radix select over their order-preserving 64-bit keys and compacted in index order.
//
// Tie order (the rule of DESIGN 9, which tests/ctc_beam_util.py restates without reference to the kernels).  Candidate
// index is (kind, slot, token): one repeat candidate per state at its slot j, then the plain candidates of leader L (the
// lowest slot of its prefix) at nS + L * KS + p with the list in class order, then one blank candidate per leader.  Repeat
// candidates come first because they must: such a repeat can equal the plain score of a token off the list exactly (a
// state 37 or more below the extension vanishes in the log-add) and would otherwise lose that tie to it.  Equal scores
// resolve by lower candidate index, and the survivors take the new slots in index order, not in score order.  Equal
// members of a merged candidate resolve in push order (fold keeps the first of equal ones): leader before partner, and
// for a repeat the state itself, then the leader of P[:-1], then its partner.  The end step ranks equal merged scores by
// lower leader slot.  Frames with no finite emission, and NaN, are outside the contract.
//
// A backpointer (parent slot << 16 | frame token) per (frame, slot) goes to a caller-supplied workspace; the end step
// merges by prefix, ranks, and traces the n-best paths back into tokens and 1-based timesteps.

constexpr int BM_THREADS = 256;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr double BM_THRESHOLD = 50.0;                   // torchaudio's beam_threshold default
constexpr uint64_t BM_ROOT = 0x6a09e667f3bcc908ull;     // hash of the empty prefix
constexpr int BM_KMAX = BEAM_MAX + 2;                   // list length: tokens considered for plain extensions
constexpr int BM_MMAX = BEAM_MAX * (BM_KMAX + 2);       // candidates per frame: repeat, plain, blank

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
__device__ __forceinline__ float unkey32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
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

// leader (lowest slot) and partner (the other state) of every state's prefix
template <typename Smem>
__device__ __forceinline__ void group_prefixes(Smem& sm, int cur, int nS) {
    const int tid = threadIdx.x;
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
}

// Members of candidate i, in (repeat, plain, blank) order: their scores and state slots, after the threshold.  What a
// new token adds is the decoder's: D::Term, D::plain(sm, L, p, blank, &n, &x) (false: leader L has no plain candidate at
// list position p; else its token n and term x), D::repeat(sm, j) (the term of P[:-1] emitting k, for the repeat
// candidate of state j) and D::add(s, x), the score s after x.
template <typename D, typename Smem>
__device__ __forceinline__ Members members(const Smem& sm, int cur, int nS, int KS, int blank, double cut, int i) {
    Members g;
    g.m = 0;
    if (i >= nS && i < nS + nS * KS) {
        const int L = (i - nS) / KS, p = (i - nS) - L * KS;
        int n;
        typename D::Term x;
        if (!D::plain(sm, L, p, blank, &n, &x)) return g;
        const int q = sm.partner[L];
        if (n != sm.tk[cur][L] || sm.pb[cur][L]) {
            const double v = D::add(sm.sc[cur][L], x);
            if (v >= cut) g.push(v, L);
        }
        if (q >= 0 && (n != sm.tk[cur][q] || sm.pb[cur][q])) {
            const double v = D::add(sm.sc[cur][q], x);
            if (v >= cut) g.push(v, q);
        }
    } else if (i >= nS) {
        const int L = i - nS - nS * KS;
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
        if (n == blank || sm.pb[cur][j]) return g;
        const double e = sm.ek[j];
        double v = sm.sc[cur][j] + e;
        if (v >= cut) g.push(v, j);
        const int P = sm.parent[j];
        if (P >= 0) {
            const typename D::Term x = D::repeat(sm, j, e);
            if (n != sm.tk[cur][P] || sm.pb[cur][P]) {
                v = D::add(sm.sc[cur][P], x);
                if (v >= cut) g.push(v, P);
            }
            const int q = sm.partner[P];
            if (q >= 0 && (n != sm.tk[cur][q] || sm.pb[cur][q])) {
                v = D::add(sm.sc[cur][q], x);
                if (v >= cut) g.push(v, q);
            }
        }
    }
    return g;
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
template <typename K, int BITS, typename KeyF, typename Smem>
__device__ __forceinline__ void radix_select(int n, int want, KeyF key, Smem& sm) {
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
template <typename K, typename KeyF, typename EmitF, typename Smem>
__device__ __forceinline__ void compact(int n, int cap, KeyF key, EmitF emit, Smem& sm) {
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

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// The end step's last part, for the nh ranked hypotheses whose final slots are in sm.win: traces the backpointers
// (parent slot << 16 | frame token per (frame, slot)) back into timesteps[r, t], then collapses them in place into tokens
// and 1-based timesteps.
template <typename Smem>
__device__ __forceinline__ void trace_and_collapse(int nh, int len, int T, int beam, int blank, const uint32_t* __restrict__ bp,
                                                   int64_t* __restrict__ tokens, int64_t* __restrict__ timesteps,
                                                   int* __restrict__ counts, Smem& sm) {
    const int tid = threadIdx.x;
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

// Steps 5 and 6 of a frame, behind the barrier that follows the candidate keys (sm.key, sm.nvalid of them valid): the
// move of a plain candidate onto a beam state to that state's repeat candidate, and the `beam` best, whose candidate
// indices go to sm.win in index order.  Returns the number of survivors; ends with a barrier.
template <typename Smem>
__device__ __forceinline__ int select_candidates(Smem& sm, int nS, int KS, int beam) {
    const int tid = threadIdx.x;
    const int M = nS * (KS + 2);
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
    return nW;
}

// The end step behind its threshold `cut`: merges the states by prefix (leader and partner as group_prefixes left them,
// D::total(sm, cur, slot) a state's end total, D::ends(total) whether it takes part), ranks the merged totals, counts the
// hypotheses, fills the unused counts and scores, and traces the n_best first.
template <typename D, typename Smem>
__device__ __forceinline__ void end_merge(Smem& sm, int cur, int nS, const double& cut, int n_best, int len, int T, int beam, int blank,
                                          const uint32_t* __restrict__ bp, int64_t* __restrict__ tokens,
                                          int64_t* __restrict__ timesteps, int* __restrict__ counts, double* __restrict__ scores,
                                          int* __restrict__ hyp_count) {
    const int tid = threadIdx.x;
    // merged value of each leader in sm.ek, its best member in sm.childp
    if (tid < nS) {
        double v = -INFINITY;
        int bs = tid, valid = 0;
        if (sm.leader[tid] == tid) {
            Members g;
            g.m = 0;
            int best;
            if (D::ends(D::total(sm, cur, tid)) && D::total(sm, cur, tid) >= cut) g.push(D::total(sm, cur, tid), tid);
            const int q = sm.partner[tid];
            if (q >= 0 && D::ends(D::total(sm, cur, q)) && D::total(sm, cur, q) >= cut) g.push(D::total(sm, cur, q), q);
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
