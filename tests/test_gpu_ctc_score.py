"""On-device CTC forward-backward scoring (amx_ctc_score.hip) against the float64 truth (tests/ctc_score_util.py), held to
4x the error of torch's own fp32 CPU ctc_loss measured on the same pool at test time (never against the code under test):
the pool itself, state counts around the 64-state strips and at every strips-per-wave variant of the kernel, frame counts
around the emission-prefetch depth, ragged lengths, 2 to 1025 classes and a non-zero blank, the feasibility boundary, -inf and
NaN emissions, malformed rows, the transposed view, candidates, a long row, determinism, graph capture and the Estimator
façade with rescoring.  Every buffer is pre-filled with a sentinel and fenced by guard elements, so what the contract leaves
untouched is checked too."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_score_util as U
import edit_util as E

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F = -77, -12345.5
GUARD = 64  # sentinel elements before and after every buffer
PREFETCH = 4  # the kernel's deepest emission prefetch (frames)


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


@pytest.fixture(scope="module")
def pool():
    return U.make_pool()


@pytest.fixture(scope="module")
def yard(pool):
    y = U.yardsticks(pool)
    print(f"\nyardsticks: E_ll = {y.E_ll:.3e}  E_post = {y.E_post:.3e}")
    return y


# the device's worst errors: ll and g as multiples of the yardsticks (bound: 4), the per-target sums as a share of their bound
WORST = {"ll": 0.0, "g": 0.0, "sums": 0.0}


def _emissions(N, T, Cn, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(N, T, Cn, generator=g) * scale, dim=-1)


def _targets(rng, L, Cn, blank=0, repeat=0.2):
    """L targets among the non-blank classes; adjacent repeats with probability `repeat` (always, when there is one class)."""
    classes = [c for c in range(Cn) if c != blank]
    out = []
    for _ in range(L):
        if out and (len(classes) == 1 or rng.random() < repeat):
            out.append(out[-1])
        else:
            out.append(int(rng.choice([c for c in classes if not out or c != out[-1]])))
    return out


def _fenced(count, dtype, sentinel, device):
    whole = torch.full((count + 2 * GUARD,), sentinel, dtype=dtype, device=device)
    return whole, whole[GUARD:GUARD + count]


class _Call:
    """One amx_ctc_score_emissions call on sentinel-filled, fenced buffers; `run` may be repeated (graph capture)."""

    def __init__(self, em, lengths, offsets, ids, max_target, blank=0, candidates=1, posteriors=True):
        from allophant_amd import lib as L

        self.lib, self.handle = L, L.load()
        self.em = em  # [N, T, C] cuda view, unit class stride
        N, T, Cn = em.shape
        R = N * candidates
        self.shape, self.blank, self.max_target, self.candidates, self.R = (N, T, Cn), blank, max_target, candidates, R
        dev = em.device
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
        self.ids = torch.tensor(list(ids) + [0], dtype=torch.int32, device=dev)
        size = C.c_size_t()
        assert self.handle.amx_ctc_score_workspace(R, T, max_target, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.fences = {}
        self.fences["workspace"], self.workspace = _fenced(size.value, torch.uint8, 0x5A, dev)
        m, P = max(1, max_target), 2 * max_target + 1
        self.fences["log_likelihood"], self.log_likelihood = _fenced(R, torch.float32, SENTINEL_F, dev)
        self.fences["occupancy"], self.occupancy = _fenced(R * m, torch.float32, SENTINEL_F, dev)
        self.fences["position_sums"], self.position_sums = _fenced(R * m, torch.float32, SENTINEL_F, dev)
        self.fences["score_sums"], self.score_sums = _fenced(R * m, torch.float32, SENTINEL_F, dev)
        self.fences["status"], self.status = _fenced(R, torch.int32, SENTINEL_I, dev)
        self.posteriors = None
        if posteriors:
            self.fences["posteriors"], self.posteriors = _fenced(R * T * P, torch.float32, SENTINEL_F, dev)

    def refill(self):
        for name, whole in self.fences.items():
            whole.fill_(0x5A if name == "workspace" else SENTINEL_I if name == "status" else SENTINEL_F)

    def run(self):
        N, T, Cn = self.shape
        p = lambda t: C.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
        code = self.handle.amx_ctc_score_emissions(
            self.em.device.index or 0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), N, T, Cn, self.blank,
            self.candidates, p(self.offsets), p(self.ids), self.max_target, p(self.workspace), self.size, p(self.log_likelihood),
            p(self.occupancy), p(self.position_sums), p(self.score_sums), p(self.posteriors), p(self.status),
            C.c_void_p(torch.cuda.current_stream(self.em.device).cuda_stream))
        assert code == self.lib.AMX_OK, self.handle.amx_last_error(None)

    def buffers(self):
        """ll, occupancy, position_sums, score_sums, posteriors (or None), status as numpy; the fences are checked."""
        for name, whole in self.fences.items():
            host = whole.cpu()
            sentinel = 0x5A if name == "workspace" else SENTINEL_I if name == "status" else SENTINEL_F
            assert bool((host[:GUARD] == sentinel).all()) and bool((host[-GUARD:] == sentinel).all()), f"write outside {name}"
        N, T, _ = self.shape
        m, P = max(1, self.max_target), 2 * self.max_target + 1
        per_target = [t.cpu().numpy().reshape(self.R, m)[:, :self.max_target] for t in (self.occupancy, self.position_sums, self.score_sums)]
        posteriors = None if self.posteriors is None else self.posteriors.cpu().numpy().reshape(self.R, T, P)
        return (self.log_likelihood.cpu().numpy(), *per_target, posteriors, self.status.cpu().numpy())


NAMES = ("log_likelihood", "occupancy", "position_sums", "score_sums", "posteriors", "status")


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _untouched(a):
    return bool((_bits(np.ascontiguousarray(a)) == _bits(np.float32(SENTINEL_F))).all())


def _compare(got, truth, lengths, candidates, yard, where=""):
    """Every row of one call's buffers against its truth row: the values within the bounds, everything else untouched."""
    ll, occupancy, position_sums, score_sums, posteriors, status = got
    for r, want in enumerate(truth):
        tag = (where, r)
        assert status[r] == want.status, (tag, status[r], want.status)
        scored = want.status == 0
        if want.status == -2:
            assert _untouched(ll[r:r + 1]), tag
        elif want.status == -1:
            assert ll[r] == -np.inf, (tag, ll[r])
        L = len(want.occupancy) if scored else 0
        k = int(lengths[r // candidates]) if scored else 0
        for buffer in (occupancy, position_sums, score_sums):
            assert _untouched(buffer[r, L:]), tag
        if posteriors is not None:
            assert _untouched(posteriors[r, k:]) and _untouched(posteriors[r, :k, 2 * L + 1:]), tag
        if not scored:
            continue
        unit_ll, unit_g = yard.E_ll * U.scale(want.ll), yard.E_post * U.scale(want.ll)
        error = abs(float(ll[r]) - want.ll)
        WORST["ll"] = max(WORST["ll"], error / unit_ll)
        assert error <= U.ll_bound(yard, want.ll), (tag, float(ll[r]), want.ll, error / unit_ll)
        if posteriors is not None and k:
            error = float(np.abs(posteriors[r, :k, :2 * L + 1] - want.g).max())
            WORST["g"] = max(WORST["g"], error / unit_g)
            assert error <= U.g_bound(yard, want.ll), (tag, "g", error / unit_g)
        for name, g, w in (("occupancy", occupancy, want.occupancy), ("position_sums", position_sums, want.position_sums),
                           ("score_sums", score_sums, want.score_sums)):
            if L:
                error = np.abs(g[r, :L] - w)
                bound = U.sum_bound(yard, want.ll, k, w)
                WORST["sums"] = max(WORST["sums"], float((error / bound).max()))
                assert (error <= bound).all(), (tag, name, int(np.argmax(error / bound)), float((error / bound).max()))


def _check(yard, em_host, lengths, rows, blank=0, max_target=None, em_device=None, offsets=None, ids=None, candidates=1,
           posteriors=True):
    """Runs the kernel on `em_host` ([N, T, C] fp32 cpu tensor; `em_device` a cuda view of the same values) and compares
    every buffer with the truth.  Returns the status row and the call."""
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
        ids = [v for r in rows for v in r]
    if max_target is None:
        max_target = max(len(r) for r in rows)
    em_device = em_host.cuda() if em_device is None else em_device
    call = _Call(em_device, lengths, offsets, ids, max_target, blank, candidates, posteriors)
    call.run()
    got = call.buffers()
    truth = U.score_batch(em_host.numpy(), lengths, offsets, ids, max_target, blank, candidates, posteriors)
    _compare(got, truth, lengths, candidates, yard)
    return got[5], call


def test_the_pool(amd, pool, yard):
    """Every row of the pool the yardsticks were measured on, one launch per class count: the device within 4x torch's own
    fp32 error, rows without a path flagged -1."""
    for Cn in (2, 5, 37, 201):
        members = [row for row in pool if row.lp.shape[1] == Cn]
        T = max(row.lp.shape[0] for row in members)
        em = torch.zeros(len(members), T, Cn)
        for n, row in enumerate(members):
            em[n, :row.lp.shape[0]] = row.lp
        lengths = [row.lp.shape[0] for row in members]
        rows = [row.targets for row in members]
        call = _Call(em.cuda(), lengths, np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist(), [v for r in rows for v in r], 100)
        call.run()
        _compare(call.buffers(), [row.truth for row in members], lengths, 1, yard, where=f"C={Cn}")
    print(f"\npool: worst device error / yardstick: ll {WORST['ll']:.3f} x E_ll, g {WORST['g']:.3f} x E_post (bound 4)")


STRIP_LENGTHS = (0, 1, 31, 32, 63, 64, 100)


def test_strip_edges(amd, yard):
    """S = 2L + 1 of 1, 3, 63, 65, 127, 129 and 201 states, each row with T = 2L + 5 frames, C = 37."""
    rng = np.random.default_rng(1)
    T = 2 * max(STRIP_LENGTHS) + 5
    em = _emissions(len(STRIP_LENGTHS), T, 37, seed=1)
    status, _ = _check(yard, em, [2 * L + 5 for L in STRIP_LENGTHS], [_targets(rng, L, 37) for L in STRIP_LENGTHS])
    assert (status == 0).all()


def test_frame_edges(amd, yard):
    """T of 1, 2, 3, 63, 64, 65 and around the prefetch depth (one below, at, one above), with no, one and several targets."""
    rng = np.random.default_rng(2)
    frames = sorted({1, 2, 3, 63, 64, 65, PREFETCH - 1, PREFETCH, PREFETCH + 1})
    lengths = [T for T in frames for _ in range(3)]
    rows = [_targets(rng, L, 9) for T in frames for L in (0, 1, min(T, 7))]
    status, _ = _check(yard, _emissions(len(lengths), 65, 9, seed=2), lengths, rows)
    assert (status >= -1).all() and (status == 0).sum() >= 2 * len(frames)


@pytest.mark.parametrize("Cn,blank", [(2, 0), (2, 1), (3, 2), (37, 5), (1025, 0), (1025, 1024)])
def test_ragged_lengths_class_counts_and_blank(amd, yard, Cn, blank):
    """frame_lengths below T: the tails of `posteriors` keep their sentinel."""
    T = 24
    rng = np.random.default_rng(Cn + blank)
    em = _emissions(4, T, Cn, seed=Cn + blank)
    status, _ = _check(yard, em, [T, 0, 1, T - 5], [_targets(rng, 6, Cn, blank), _targets(rng, 2, Cn, blank),
                                                   _targets(rng, 1, Cn, blank), _targets(rng, 9, Cn, blank)], blank=blank)
    assert status.tolist() == [0, -1, 0, 0]


def test_rows_without_frames_or_targets(amd, yard):
    em = _emissions(4, 9, 5, seed=4)
    status, call = _check(yard, em, [0, 9, 0, 1], [[], [], [3], []], max_target=3)
    assert status.tolist() == [0, 0, -1, 0]
    assert call.log_likelihood.cpu().tolist()[0] == 0.0
    status, _ = _check(yard, em, [0, 9, 1, 4], [[], [], [], []])  # max_target = 0
    assert status.tolist() == [0, 0, 0, 0]


def test_feasibility_boundary_and_repeated_targets(amd, yard):
    """For every row T equal to targets + repeats (a single path) and one frame fewer (-1); half of the rows are runs of one
    repeated id."""
    rng = np.random.default_rng(9)
    rows, lengths = [], []
    for k, L in enumerate((1, 2, 5, 31, 32, 33, 40, 70)):
        y = [3] * L if k % 2 else _targets(rng, L, 6, repeat=0.4)
        rows += [y, y]
        lengths += [U.minimum_frames(y), U.minimum_frames(y) - 1]
    em = _emissions(len(rows), max(lengths), 6, seed=9)
    status, call = _check(yard, em, lengths, rows)
    assert status.tolist() == [0, -1] * 8
    assert call.buffers()[1][0, 0] == 1.0  # one frame, one target: g = exp(e + e - e - e)
    # runs of repeated ids with room to spare
    rows = [[2] * 40, [1] * 10 + [2] * 10 + [1] * 13, [4] * 64]
    status, _ = _check(yard, _emissions(3, 140, 5, seed=10), [140, 90, 127], rows)
    assert status.tolist() == [0, 0, 0]


def test_minus_infinity_emissions(amd, yard):
    """Scattered -inf (rows stay feasible or not, as the truth says), and one row with -inf in every frame of the class of
    one of its targets (-1)."""
    T, Cn = 60, 7
    em = _emissions(5, T, Cn, seed=13)
    g = torch.Generator().manual_seed(13)
    em[:4][torch.rand(4, T, Cn, generator=g) < torch.tensor([0.05, 0.2, 0.4, 0.7]).view(4, 1, 1)] = -float("inf")
    rng = np.random.default_rng(13)
    rows = [_targets(rng, 12, Cn) for _ in range(4)] + [[1, 2, 3, 4, 5, 6]]
    em[4, :, 4] = -float("inf")
    status, _ = _check(yard, em, [T] * 5, rows)
    assert status[4] == -1 and 0 in status.tolist() and status.tolist().count(-1) >= 2
    # a blocked row next to the same targets unblocked
    em = _emissions(2, 20, 4, seed=14)
    em[0, :, 0] = -float("inf")  # no blank at all: the repeat cannot be separated
    status, _ = _check(yard, em, [20, 20], [[1, 1, 2], [1, 1, 2]])
    assert status.tolist() == [-1, 0]
    # feasible rows with -inf emissions of their own targets in most frames: g is exactly 0 there and no sum is NaN
    em = _emissions(2, 12, 4, seed=15)
    em[:, :5, 1] = -float("inf")
    em[:, 8:, 2] = -float("inf")
    status, call = _check(yard, em, [12, 12], [[1, 2], [2, 1, 2]])
    assert status[0] == 0
    got = call.buffers()
    assert (got[4][0, :5, 1] == 0.0).all() and not np.isnan(got[3][0, :2]).any()


def test_nan_emissions_terminate_and_stay_in_range(amd):
    """The values on NaN emissions are unspecified; the kernel terminates and the fences around every buffer (and what lies
    past each row's frames, targets and states) stay intact."""
    N, T, Cn, L = 8, 150, 6, 50
    em = _emissions(N, T, Cn, seed=22)
    g = torch.Generator().manual_seed(22)
    em[torch.rand(N, T, Cn, generator=g) < torch.tensor([0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 0.6, 1.0]).view(N, 1, 1)] = float("nan")
    rng = np.random.default_rng(22)
    rows = [_targets(rng, L - n, Cn) for n in range(N)]
    lengths = [T, T, T - 1, T, 77, T, T, T]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
    call = _Call(em.cuda(), lengths, offsets, [v for r in rows for v in r], L)
    call.run()
    torch.cuda.synchronize()
    ll, occupancy, position_sums, score_sums, posteriors, status = call.buffers()  # (checks the fences)
    assert set(status.tolist()) <= {0, -1}
    for n in range(N):
        k, count = (lengths[n], len(rows[n])) if status[n] == 0 else (0, 0)
        assert _untouched(posteriors[n, k:]) and _untouched(posteriors[n, :k, 2 * count + 1:])
        for buffer in (occupancy, position_sums, score_sums):
            assert _untouched(buffer[n, count:])


def test_transposed_view_is_read_in_place(amd, yard):
    out = _emissions(30, 5, 41, seed=11)  # [T, N, C]
    view = out.cuda().transpose(0, 1)
    assert not view.is_contiguous()
    rng = np.random.default_rng(11)
    lengths = [30, 12, 0, 29, 1]
    rows = [_targets(rng, L, 41) for L in (9, 4, 0, 11, 1)]
    host = out.transpose(0, 1).contiguous()
    _, call = _check(yard, host, lengths, rows, em_device=view)
    # and through the Python entry point, bit for bit the same call
    scored = amd.ctc_score(view, torch.tensor(lengths), rows, posteriors=True)
    assert scored.log_likelihood.shape == (5, 1) and scored.posteriors.shape == (5, 1, 30, 23) and scored.names is None
    status = call.buffers()[5]
    assert scored.status.cpu().view(-1).tolist() == status.tolist()
    got = scored.scores()
    ll = call.buffers()[0]
    for n in range(5):
        if status[n] != 0:
            assert got[n][0] is None
            continue
        assert np.float32(got[n][0].log_likelihood) == ll[n]
        assert got[n][0].posteriors.shape == (lengths[n], 2 * len(rows[n]) + 1)
        want = U.score_row(host[n, :lengths[n]].numpy(), rows[n])
        assert np.allclose(got[n][0].positions.numpy(), want.position_sums / want.occupancy, rtol=1e-3, atol=1e-3)
    # padded targets with their lengths give the same rows
    width = max(len(t) for t in rows)
    padded = torch.tensor([t + [0] * (width - len(t)) for t in rows])
    again = amd.ctc_score(view, torch.tensor(lengths), (padded, torch.tensor([len(t) for t in rows])))
    assert torch.equal(again.log_likelihood[scored.status == 0], scored.log_likelihood[scored.status == 0]) and again.posteriors is None


def test_malformed_rows_are_flagged_and_write_nothing(amd, yard):
    """A target equal to the blank, a target >= C, a negative target, decreasing offsets, offsets past the id count, L >
    max_target and frame lengths outside [0, T]: -2 and sentinels everywhere, next to valid rows that stay correct."""
    T, Cn, blank = 20, 6, 2
    em = _emissions(9, T, Cn, seed=15)
    #       row: 0 ok     1 blank    2 >= C     3 ok  4 negative  5 too long        6 ok  7 length > T   8 length < 0
    rows = [[1, 3, 4], [1, 2, 3], [1, 6, 3], [5], [0, -1], [1, 3, 1, 3, 1], [3, 3], [1], [4]]
    status, _ = _check(yard, em, [T, T, T, 7, T, T, T, T + 1, -1], rows, blank=blank, max_target=4)
    assert status.tolist() == [0, -2, -2, 0, -2, -2, 0, -2, -2]
    ids = [1, 3, 4, 5, 1, 3, 4, 5]
    status, _ = _check(yard, em[:4], [T] * 4, None, blank=blank, max_target=4, offsets=[0, 5, 3, 9, 8], ids=ids)
    assert status.tolist() == [-2, -2, -2, -2]  # row 0 holds 5 > max_target ids
    status, _ = _check(yard, em[:4], [T] * 4, None, blank=blank, max_target=5, offsets=[0, 4, 2, 6, 8], ids=ids)
    assert status.tolist() == [0, -2, 0, 0]
    status, _ = _check(yard, em[:3], [T] * 3, None, blank=blank, max_target=5, offsets=[-1, 2, 4, 3], ids=ids)
    assert status.tolist() == [-2, -2, -2]
    with pytest.raises(ValueError, match="row 1"):
        amd.ctc_score(em[:3].cuda(), torch.tensor([T] * 3), [[1], [2], [3]], blank_index=blank).scores()


def test_three_candidates_equal_three_calls(amd, yard):
    """candidates = 3 (row r reads utterance r // 3) against the truth, and bitwise equal to three calls of one candidate."""
    N, T, Cn, G = 4, 50, 11, 3
    rng = np.random.default_rng(23)
    em = _emissions(N, T, Cn, seed=23)
    lengths = [T, 45, 0, T - 1]
    rows = [_targets(rng, int(rng.integers(0, 20)), Cn) for _ in range(N * G)]  # (at most 19 targets: 38 frames suffice)
    status, call = _check(yard, em, lengths, rows, candidates=G)
    assert (status[:6] == 0).all()
    together = call.buffers()
    width = max(len(r) for r in rows)
    for g in range(G):
        single = _Call(em.cuda(), lengths, np.concatenate(([0], np.cumsum([len(r) for r in rows[g::G]]))).tolist(),
                       [v for r in rows[g::G] for v in r], width)
        single.run()
        for name, a, b in zip(NAMES, together, single.buffers()):
            assert np.array_equal(_bits(np.ascontiguousarray(a[g::G])), _bits(b)), (g, name)


@pytest.mark.parametrize("L", [1023, 1024, 2047, 2048, 4095])
def test_strips_per_wave_variants(amd, yard, L):
    """The kernel is instantiated for 1, 2, 4 and 8 strips per wave: max_target around 1024 and 2048 switches between them,
    and 4095 targets (8191 states) fill the LDS rows.  T is the smallest feasible one (a single path); posteriors = NULL.  A
    short row shares each launch."""
    rng = np.random.default_rng(L)
    y = _targets(rng, L, 5, repeat=0.002)
    T = U.minimum_frames(y)
    em = _emissions(2, T, 5, seed=L)
    status, call = _check(yard, em, [T, 40], [y, _targets(rng, 7, 5)], posteriors=False)
    assert status.tolist() == [0, 0]
    # every target holds its one frame (fp32 rounding of a + b - e - ll at |ll| near 8000 is about 1e-3)
    assert np.abs(call.buffers()[1][0] - 1.0).max() < 0.05


def test_long_row(amd, yard):
    """T = 3000 with 600 targets (19 strips: every wave of the block, two strips each) next to a 17-frame row."""
    rng = np.random.default_rng(16)
    em = _emissions(2, 3000, 37, seed=16, scale=3.0)
    status, _ = _check(yard, em, [3000, 17], [_targets(rng, 600, 37), _targets(rng, 5, 37)])
    assert status.tolist() == [0, 0]


def _graph_case():
    rng = np.random.default_rng(19)
    em = _emissions(3, 150, 9, seed=19).cuda()
    lengths = [150, 77, 0]
    rows = [_targets(rng, L, 9) for L in (70, 20, 0)] * 2
    rows = [rows[0], rows[3][:40], rows[1], rows[4][:5], rows[2], [1]]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
    return em, lengths, offsets, [v for r in rows for v in r]


def test_two_runs_are_bitwise_equal(amd):
    em, lengths, offsets, ids = _graph_case()
    first, second = _Call(em, lengths, offsets, ids, 70, candidates=2), _Call(em, lengths, offsets, ids, 70, candidates=2)
    first.run()
    second.run()
    second.refill()
    second.run()
    for name, a, b in zip(NAMES, first.buffers(), second.buffers()):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert first.buffers()[5].tolist() == [0, 0, 0, 0, 0, -1]


def test_graph_capture(amd):
    """One amx_ctc_score_emissions call captured on a single stream and replayed twice equals the eager result bit for bit."""
    em, lengths, offsets, ids = _graph_case()
    eager = _Call(em, lengths, offsets, ids, 70, candidates=2)
    eager.run()
    torch.cuda.synchronize()
    want = eager.buffers()
    captured = _Call(em, lengths, offsets, ids, 70, candidates=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.run()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.run()
    for _ in range(2):
        captured.refill()
        graph.replay()
        torch.cuda.synchronize()
        for name, g, w in zip(NAMES, captured.buffers(), want):
            assert np.array_equal(_bits(g), _bits(w)), name


def _table():
    from allophant_amd.phonetic import AttributeTable

    return AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])


@pytest.mark.parametrize("kind", ["multitask", "hierarchical"])
def test_through_the_estimator(amd, yard, kind):
    """predict -> label_targets -> Estimator.score against the truth on predictions.outputs copied to the host, for every
    output; Scored.ctc_loss against upstream's CTCWrapper arithmetic; log_likelihood >= the best path's total from
    Estimator.align; rescore_device of beam 8 / n_best 4 against the truth of every hypothesis."""
    from allophant_amd import spec as S, synthetic
    from allophant_amd.alignment import label_targets
    from allophant_amd.evaluation import EvaluationMaps

    table = _table()
    attributes = ["syllabic", "long", "nasal"]
    make = S.multitask_spec if kind == "multitask" else S.hierarchical_spec
    spec = make(S.tiny_encoder(2), attributes, embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    names = S.output_names(spec)
    N = 5
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    rng = np.random.default_rng(31)
    labels = [[inventory[i] for i in rng.integers(0, len(inventory), rng.integers(1, 9))] for _ in range(N)]
    labels[2] = []

    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    try:
        batch = amd.Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long))
        pred = est.predict(batch, synthetic.make_inventory(spec, len(inventory), seed=2))
        targets = label_targets(EvaluationMaps(table, names, inventory, ["lg0"]), labels, ["lg0"] * N)
        frames = [int(v) for v in pred.lengths]
        host = {name: pred.outputs[name].cpu() for name in names}  # [T, N, C]

        scored = est.score_device(pred, targets, posteriors=True)
        O, T = len(names), next(iter(host.values())).shape[0]
        assert scored.names == names and scored.present == names and scored.log_likelihood.shape == (O, N, 1)
        assert scored.log_likelihood.is_cuda and scored.posteriors.shape[:4] == (O, N, 1, T)
        result = scored.scores()
        aligned = est.align(pred, targets)
        loss_bound, torch_loss, feasible = 0.0, 0.0, 0
        for name in names:
            em = host[name].transpose(0, 1).contiguous()
            for n, row in enumerate(targets[name]):
                want = U.score_row(em[n, :frames[n]].numpy(), row)
                got = result[name][n][0]
                assert (got is None) == (want.status != 0) == (aligned[name][n] is None), (name, n)
                if got is None:
                    continue
                feasible += 1
                loss_bound += U.ll_bound(yard, want.ll)
                assert abs(got.log_likelihood - want.ll) <= U.ll_bound(yard, want.ll), (name, n)
                assert np.abs(got.posteriors.numpy() - want.g).max() <= U.g_bound(yard, want.ll), (name, n)
                assert (np.abs(got.occupancy.numpy() - want.occupancy) <= U.sum_bound(yard, want.ll, frames[n], want.occupancy)).all()
                # the sum over every path holds the best path
                assert got.log_likelihood >= aligned[name][n].total - U.ll_bound(yard, want.ll), (name, n)
                seconds = got.seconds(spec)
                assert seconds.shape == (len(row),) and (len(row) < 2 or float(seconds[-1]) > float(seconds[0]) >= 0.0)
            width = max(len(row) for row in targets[name])
            padded = torch.tensor([list(row) + [0] * (width - len(row)) for row in targets[name]], dtype=torch.long).view(N, width)
            torch_loss += float(F.ctc_loss(host[name], padded, torch.tensor(frames), torch.tensor([len(row) for row in targets[name]]),
                                           blank=0, reduction="sum", zero_infinity=True))
        assert feasible >= 3 * O
        loss = scored.ctc_loss()
        assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0
        assert abs(float(loss) - torch_loss) <= loss_bound, (float(loss), torch_loss, loss_bound)
        # Estimator.score drops the candidate level; an output without targets is scored against nothing
        plain = est.score(pred, {"phoneme": targets["phoneme"]})
        assert list(plain) == ["phoneme"] and plain["phoneme"][0].posteriors is None
        assert plain["phoneme"][0].log_likelihood == result["phoneme"][0][0].log_likelihood
        with pytest.raises(ValueError):
            est.score(pred, {"nope": [[]] * N})

        beam = est.beam_decode_device(pred, 8, 4)
        rescored = est.rescore_device(pred, beam)
        assert rescored.log_likelihood.shape == (O, N, 4) and rescored.log_likelihood.is_cuda
        ll, posterior = rescored.log_likelihood.cpu(), rescored.nbest_posteriors.cpu()
        hypotheses = beam.hypotheses()
        found = beam.hyp_counts.cpu()
        several = 0
        for o, name in enumerate(names):
            em = host[name].transpose(0, 1).contiguous()
            for n in range(N):
                count = int(found[o, n])
                assert count == len(hypotheses[name][n])
                several += count > 1
                assert (ll[o, n, count:] == -float("inf")).all() and (posterior[o, n, count:] == 0.0).all()
                for h, hypothesis in enumerate(hypotheses[name][n]):
                    want = U.score_row(em[n, :frames[n]].numpy(), hypothesis.tokens.tolist())
                    assert want.status == 0 and abs(float(ll[o, n, h]) - want.ll) <= U.ll_bound(yard, want.ll), (name, n, h)
                if count:
                    assert abs(float(posterior[o, n].sum()) - 1.0) <= 1e-5
        assert several >= 1
    finally:
        est.close()


def test_report_worst_ratios(amd, yard):
    """Not a check of its own: prints the worst ratios the tests above met (run with -s), each a multiple of the yardstick
    against the bound of 4."""
    print(f"\nyardsticks E_ll = {yard.E_ll:.3e}, E_post = {yard.E_post:.3e}; device worst: ll {WORST['ll']:.3f} x E_ll, "
          f"g {WORST['g']:.3f} x E_post (bound 4), per-target sums {WORST['sums']:.3f} of their bound")
    assert WORST["ll"] <= U.MARGIN and WORST["g"] <= U.MARGIN
