"""On-device CTC scoring of every one-edit variant (amx_ctc_variants.hip) against the float64 contract
(tests/ctc_variants_util.py).  Every finite cell is held to ctc_score_util.ll_bound: 4x the error of torch's own fp32 CPU
ctc_loss against float64, measured on make_pool() at test time (never against the code under test) -- each variant is a chain
of the depth of ll itself: forward to t, one bridging state, backward from t + 1.  A cell that is -inf in the truth must be
-inf on the device.  Shapes: state counts around a 64-state strip and two strips, class counts around a 64-class strip with
the blank first, in the middle and in a partial last strip, frame counts around the emission prefetch depth, the lattice
kernel's four instantiations; all-equal targets, ragged lengths, rows below minimum_frames, -inf and NaN emissions, malformed
rows, the transposed view, a long row, determinism, graph capture, the Estimator façade and planted edits.  Every buffer is
pre-filled with a sentinel and fenced by guard elements, so what the contract leaves untouched is checked too."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_score_util as U
import ctc_variants_util as V

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F = -77, -12345.5
GUARD = 64  # sentinel elements before and after every buffer
PREFETCH = 4  # the variants kernel's prefetch depth, and the lattice kernel's deepest (frames)
INF = float("inf")


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


@pytest.fixture(scope="module")
def yard():
    y = U.yardsticks(U.make_pool())
    print(f"\nyardstick: E_ll = {y.E_ll:.3e}")
    return y


WORST = {"cell": 0.0, "ll": 0.0, "own": 0.0}  # the device's worst errors as multiples of E_ll * max(1, |truth|) (bound: 4)


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
    """One amx_ctc_variants_emissions call on sentinel-filled, fenced buffers; `run` may be repeated (graph capture)."""

    def __init__(self, em, lengths, offsets, ids, max_target, blank=0):
        from allophant_amd import lib as L

        self.lib, self.handle = L, L.load()
        self.em = em  # [N, T, C] cuda view, unit class stride
        N, T, Cn = em.shape
        self.shape, self.blank, self.max_target = (N, T, Cn), blank, max_target
        dev = em.device
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
        self.ids = torch.tensor(list(ids) + [0], dtype=torch.int32, device=dev)
        size = C.c_size_t()
        assert self.handle.amx_ctc_variants_workspace(N, T, max_target, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.fences = {}
        self.fences["workspace"], self.workspace = _fenced(size.value, torch.uint8, 0x5A, dev)
        self.fences["log_likelihood"], self.log_likelihood = _fenced(N, torch.float32, SENTINEL_F, dev)
        self.fences["substitutions"], self.substitutions = _fenced(N * max_target * Cn, torch.float32, SENTINEL_F, dev)
        self.fences["insertions"], self.insertions = _fenced(N * (max_target + 1) * Cn, torch.float32, SENTINEL_F, dev)
        self.fences["status"], self.status = _fenced(N, torch.int32, SENTINEL_I, dev)

    def refill(self):
        for name, whole in self.fences.items():
            whole.fill_(0x5A if name == "workspace" else SENTINEL_I if name == "status" else SENTINEL_F)

    def run(self):
        N, T, Cn = self.shape
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        code = self.handle.amx_ctc_variants_emissions(
            self.em.device.index or 0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), N, T, Cn, self.blank,
            p(self.offsets), p(self.ids), self.max_target, p(self.workspace), self.size, p(self.log_likelihood),
            p(self.substitutions), p(self.insertions), p(self.status), C.c_void_p(torch.cuda.current_stream(self.em.device).cuda_stream))
        assert code == self.lib.AMX_OK, self.handle.amx_last_error(None)

    def buffers(self):
        """ll, substitutions, insertions, status as numpy; the fences are checked."""
        for name, whole in self.fences.items():
            host = whole.cpu()
            sentinel = 0x5A if name == "workspace" else SENTINEL_I if name == "status" else SENTINEL_F
            assert bool((host[:GUARD] == sentinel).all()) and bool((host[-GUARD:] == sentinel).all()), f"write outside {name}"
        N, _, Cn = self.shape
        return (self.log_likelihood.cpu().numpy(), self.substitutions.cpu().numpy().reshape(N, self.max_target, Cn),
                self.insertions.cpu().numpy().reshape(N, self.max_target + 1, Cn), self.status.cpu().numpy())


NAMES = ("log_likelihood", "substitutions", "insertions", "status")


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _untouched(a):
    return bool((_bits(np.ascontiguousarray(a)) == _bits(np.float32(SENTINEL_F))).all())


def _truth(em, lengths, offsets, ids, max_target, blank, slots=None):
    """The batch form of the C ABI: malformed rows are refused with -2."""
    N, T, _ = em.shape
    rows = []
    for n in range(N):
        lb, le, k = int(offsets[n]), int(offsets[n + 1]), int(lengths[n])
        if k < 0 or k > T or lb < 0 or le < lb or le > int(offsets[N]) or le - lb > max_target:
            rows.append(V.VariantRow(-2, -INF, None, None))
        else:
            rows.append(V.variants_row(em[n, :k], list(ids[lb:le]), blank, None if slots is None else slots[n]))
    return rows


def _compare(got, truth, targets, yard, blank, infeasible=False, where=""):
    """Every row of one call's buffers against its truth row: the cells within the bound and -inf where the truth is,
    everything else untouched.  `infeasible`: the case is built to hold cells without a path (else more than 10 % of them make
    it vacuous).  Cells that the truth left out (NaN) are not compared."""
    ll, sub, ins, status = got
    compared = infinite = 0
    for r, want in enumerate(truth):
        tag = (where, r)
        assert status[r] == want.status, (tag, status[r], want.status)
        if want.status == -2:
            assert _untouched(ll[r:r + 1]), tag
        elif want.status == -1:
            assert ll[r] == -np.inf, (tag, ll[r])
        if want.status != 0:
            assert _untouched(sub[r]) and _untouched(ins[r]), tag
            continue
        L = want.sub.shape[0]
        assert _untouched(sub[r, L:]) and _untouched(ins[r, L + 1:]), tag
        # ll: the truth of score_row, which variants_row restates (equal to 1e-9, test_ctc_variants_contract.py)
        if want.ll == -np.inf:
            assert ll[r] == -np.inf, (tag, ll[r])
        else:
            error = abs(float(ll[r]) - want.ll) / (yard.E_ll * U.scale(want.ll))
            WORST["ll"] = max(WORST["ll"], error)
            assert error <= U.MARGIN, (tag, "ll", float(ll[r]), want.ll, error)
        for name, g, w in (("sub", sub[r, :L], want.sub), ("ins", ins[r, :L + 1], want.ins)):
            known = ~np.isnan(w)
            assert not np.isnan(g[known]).any(), (tag, name)
            lost = w == -np.inf
            assert (g[lost] == -np.inf).all(), (tag, name, "a cell without a path is not -inf")
            finite = known & ~lost
            compared += int(known.sum())
            infinite += int(lost.sum())
            if finite.any():
                error = np.abs(g[finite].astype(np.float64) - w[finite]) / (yard.E_ll * np.maximum(1.0, np.abs(w[finite])))
                WORST["cell"] = max(WORST["cell"], float(error.max()))
                assert (np.abs(g[finite].astype(np.float64) - w[finite]) <= U.ll_bound(yard, 1.0) * np.maximum(1.0, np.abs(w[finite]))).all(), \
                    (tag, name, float(error.max()))
        # the transcript's own symbol substituted for itself, and nothing inserted, are the transcript
        assert (_bits(ins[r, :L + 1, blank]) == _bits(ll[r:r + 1])).all(), tag
        for l, v in enumerate(targets[r]):
            if ll[r] == -np.inf:
                assert sub[r, l, v] == -np.inf, (tag, l)
            else:
                error = abs(float(sub[r, l, v]) - float(ll[r])) / (yard.E_ll * U.scale(float(ll[r])))
                WORST["own"] = max(WORST["own"], error)
                assert error <= U.MARGIN, (tag, l, error)
    if not infeasible:
        assert compared and infinite <= 0.1 * compared, (where, "vacuous", infinite, compared)
    return compared, infinite


def _check(yard, em_host, lengths, rows, blank=0, max_target=None, em_device=None, offsets=None, ids=None, infeasible=False,
           slots=None):
    """Runs the two kernels on `em_host` ([N, T, C] fp32 cpu tensor; `em_device` a cuda view of the same values) and compares
    every buffer with the truth.  Returns the buffers and the call."""
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
        ids = [v for r in rows for v in r]
    if max_target is None:
        max_target = max(len(r) for r in rows)
    em_device = em_host.cuda() if em_device is None else em_device
    call = _Call(em_device, lengths, offsets, ids, max_target, blank)
    call.run()
    got = call.buffers()
    truth = _truth(em_host.numpy(), lengths, offsets, ids, max_target, blank, slots)
    N = em_host.shape[0]
    targets = [list(ids[int(offsets[n]):int(offsets[n + 1])]) if truth[n].status == 0 else [] for n in range(N)]
    _compare(got, truth, targets, yard, blank, infeasible)
    return got, call


STRIP_LENGTHS = (0, 1, 2, 31, 32, 33, 64)  # 1, 3, 5, 63, 65, 67 and 129 states


@pytest.mark.parametrize("Cn,blank", [(2, 0), (2, 1), (5, 2), (63, 0), (64, 63), (65, 64), (130, 64), (130, 129)])
def test_strip_edges_class_counts_and_blank(amd, yard, Cn, blank):
    """Rows of 0 to 64 targets with T = 2L + 2 frames each (every variant has a path) under 2 to 130 classes: one class strip,
    a full one, one lane more, and three strips with the blank in a full and in the partial last one."""
    rng = np.random.default_rng(100 * Cn + blank)
    lengths = [2 * L + 2 for L in STRIP_LENGTHS]
    em = _emissions(len(STRIP_LENGTHS), max(lengths), Cn, seed=Cn + blank)
    rows = [_targets(rng, L, Cn, blank) for L in STRIP_LENGTHS]
    (_, _, _, status), _ = _check(yard, em, lengths, rows, blank=blank)
    assert (status == 0).all()


def test_frame_edges(amd, yard):
    """T of 1, 2, 3, around the prefetch depth and around 64, with no, one and several targets: short rows hold variants
    without a path."""
    rng = np.random.default_rng(2)
    frames = sorted({1, 2, 3, PREFETCH - 1, PREFETCH, PREFETCH + 1, 2 * PREFETCH, 2 * PREFETCH + 1, 63, 64, 65})
    lengths = [T for T in frames for _ in range(3)]
    rows = [_targets(rng, L, 9) for T in frames for L in (0, 1, min(T, 7))]
    (_, _, _, status), _ = _check(yard, _emissions(len(lengths), 65, 9, seed=2), lengths, rows, infeasible=True)
    assert (status == 0).all()


def test_all_equal_targets_and_substitutes_equal_to_a_neighbour(amd, yard):
    """Runs of one id (every substitute but the id itself breaks a repeat, every insertion of the id makes one), alternating
    ids (a substitute equal to both neighbours) and a non-zero blank."""
    rows = [[3] * 10, [1, 2] * 6, [4, 4, 1, 1, 4, 4], [2]]
    lengths = [2 * len(r) + 2 for r in rows]
    (ll, sub, ins, status), _ = _check(yard, _emissions(4, max(lengths), 5, seed=3), lengths, rows)
    assert (status == 0).all()
    rows = [[0] * 7, [0, 1, 0, 1], [3, 3]]
    _check(yard, _emissions(3, 16, 4, seed=4), [16, 10, 6], rows, blank=2)


def test_ragged_lengths_and_rows_without_frames_or_targets(amd, yard):
    T = 24
    rng = np.random.default_rng(5)
    em = _emissions(6, T, 7, seed=5)
    rows = [_targets(rng, 6, 7), _targets(rng, 2, 7), _targets(rng, 1, 7), _targets(rng, 9, 7), [], []]
    (ll, sub, ins, status), _ = _check(yard, em, [T, 0, 4, T - 4, 0, 5], rows)
    assert status.tolist() == [0, -1, 0, 0, 0, 0]
    assert ll[4] == 0.0 and ins[4, 0].tolist() == [0.0] + [-INF] * 6  # no frames, no targets: only "nothing" has a path
    (_, _, _, status), _ = _check(yard, em[:3], [0, 9, 1], [[], [], []], infeasible=True)  # max_target = 0: no substitution rows at all
    assert status.tolist() == [0, 0, 0]


def test_rows_below_minimum_frames_keep_their_deletions(amd, yard):
    """One and two frames too few for the transcript: ll is -inf under status 0, while a deletion that removes a repeat (or
    any symbol, one frame short) has a path."""
    rows, lengths = [], []
    for y in ([3] * 6, [1, 1, 2, 2, 1], [2, 4, 1], [3] * 33):
        for short in (1, 2):
            rows.append(y)
            lengths.append(U.minimum_frames(y) - short)
    (ll, sub, ins, status), _ = _check(yard, _emissions(len(rows), max(lengths), 5, seed=6), lengths, rows, infeasible=True)
    assert (status == 0).all() and (ll == -np.inf).all()
    for r in range(0, len(rows), 2):  # one frame short: every deletion of a repeated symbol fits
        assert np.isfinite(sub[r, 0, 0]), r
    assert np.isfinite(sub[1, :6, 0]).all()  # [3] * 6 two frames short: a deletion saves the symbol and its blank


def test_minus_infinity_emissions(amd, yard):
    """A whole class at -inf (its column of every row of variants is -inf, 1 of 37), and scattered -inf."""
    T, Cn = 40, 37
    rng = np.random.default_rng(7)
    em = _emissions(3, T, Cn, seed=7)
    em[:, :, 11] = -INF
    rows = [[c for c in _targets(rng, 14, Cn) if c != 11] for _ in range(3)]
    (ll, sub, ins, status), _ = _check(yard, em, [T, T - 3, T - 9], rows)
    assert (sub[0, :len(rows[0]), 11] == -np.inf).all() and (ins[0, :len(rows[0]) + 1, 11] == -np.inf).all() and np.isfinite(ll).all()
    em = _emissions(4, 30, 6, seed=8)
    g = torch.Generator().manual_seed(8)
    em[torch.rand(4, 30, 6, generator=g) < torch.tensor([0.05, 0.2, 0.4, 0.7]).view(4, 1, 1)] = -INF
    _check(yard, em, [30] * 4, [_targets(rng, 8, 6) for _ in range(4)], infeasible=True)


def test_nan_emissions_terminate_and_stay_in_range(amd):
    """The values on NaN emissions are unspecified; the kernels terminate and the fences around every buffer (and what lies
    past each row's targets) stay intact."""
    N, T, Cn, L = 6, 90, 70, 40
    em = _emissions(N, T, Cn, seed=22)
    g = torch.Generator().manual_seed(22)
    em[torch.rand(N, T, Cn, generator=g) < torch.tensor([0.001, 0.01, 0.1, 0.3, 0.6, 1.0]).view(N, 1, 1)] = float("nan")
    rng = np.random.default_rng(22)
    rows = [_targets(rng, L - 3 * n, Cn) for n in range(N)]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
    call = _Call(em.cuda(), [T, T, T - 1, 77, T, T], offsets, [v for r in rows for v in r], L)
    call.run()
    torch.cuda.synchronize()
    ll, sub, ins, status = call.buffers()  # (checks the fences)
    assert status.tolist() == [0] * N
    for n in range(N):
        assert _untouched(sub[n, len(rows[n]):]) and _untouched(ins[n, len(rows[n]) + 1:])


def test_malformed_rows_are_flagged_and_write_nothing(amd, yard):
    """A target equal to the blank, a target >= C, a negative target, decreasing offsets, offsets past the id count, L >
    max_target and frame lengths outside [0, T]: -2 and sentinels everywhere, next to valid rows that stay correct."""
    T, Cn, blank = 14, 6, 2
    em = _emissions(9, T, Cn, seed=15)
    #       row: 0 ok     1 blank    2 >= C     3 ok  4 negative  5 too long        6 ok  7 length > T   8 length < 0
    rows = [[1, 3, 4], [1, 2, 3], [1, 6, 3], [5], [0, -1], [1, 3, 1, 3, 1], [3, 3], [1], [4]]
    (_, _, _, status), _ = _check(yard, em, [T, T, T, 7, T, T, T, T + 1, -1], rows, blank=blank, max_target=4)
    assert status.tolist() == [0, -2, -2, 0, -2, -2, 0, -2, -2]
    ids = [1, 3, 4, 5, 1, 3, 4, 5]
    (_, _, _, status), _ = _check(yard, em[:4], [T] * 4, None, blank=blank, max_target=4, offsets=[0, 5, 3, 9, 8], ids=ids, infeasible=True)
    assert status.tolist() == [-2, -2, -2, -2]  # row 0 holds 5 > max_target ids
    (_, _, _, status), _ = _check(yard, em[:4], [T] * 4, None, blank=blank, max_target=5, offsets=[0, 4, 2, 6, 8], ids=ids)
    assert status.tolist() == [0, -2, 0, 0]
    (_, _, _, status), _ = _check(yard, em[:3], [T] * 3, None, blank=blank, max_target=5, offsets=[-1, 2, 4, 3], ids=ids, infeasible=True)
    assert status.tolist() == [-2, -2, -2]
    with pytest.raises(ValueError, match="row 1"):
        bad = amd.ctc_variants(em[:3].cuda(), torch.tensor([T, T + 1, T]), [[1], [3], [3]], blank=blank)
        bad.diagnose()


def test_transposed_view_is_read_in_place(amd, yard):
    out = _emissions(30, 5, 41, seed=11)  # [T, N, C]
    view = out.cuda().transpose(0, 1)
    assert not view.is_contiguous()
    rng = np.random.default_rng(11)
    lengths = [30, 12, 0, 29, 4]
    rows = [_targets(rng, L, 41) for L in (9, 4, 0, 11, 1)]
    host = out.transpose(0, 1).contiguous()
    (ll, sub, ins, status), _ = _check(yard, host, lengths, rows, em_device=view)
    # and through the Python entry point, bit for bit the same call
    v = amd.ctc_variants(view, torch.tensor(lengths), rows)
    assert v.substitutions.shape == (5, 11, 41) and v.insertions.shape == (5, 12, 41) and v.log_likelihood.is_cuda
    assert v.status.cpu().tolist() == status.tolist() and v.lengths == lengths and v.target_counts.tolist() == [9, 4, 0, 11, 1]
    assert np.array_equal(_bits(v.log_likelihood.cpu().numpy()), _bits(ll))
    for n, row in enumerate(rows):
        assert np.array_equal(_bits(v.substitutions[n, :len(row)].cpu().numpy()), _bits(sub[n, :len(row)])), n
        assert np.array_equal(_bits(v.insertions[n, :len(row) + 1].cpu().numpy()), _bits(ins[n, :len(row) + 1])), n
        assert v.targets[n, :len(row)].tolist() == row
    # the device-side views against the truth: goodness of the transcript's symbols, and the best alternative per position
    want = V.variants_row(host[0].numpy(), rows[0])
    goodness = v.goodness().cpu().numpy()
    expected = np.array([want.sub[l, c] for l, c in enumerate(rows[0])]) - np.logaddexp.reduce(want.sub, axis=1)
    # (two device cells, each within its bound, and the fp32 rounding of their logsumexp and difference)
    slack = 2 * U.ll_bound(yard, float(np.abs(want.sub).max())) + 4 * 2.0 ** -24 * float(np.abs(want.sub).max())
    assert np.abs(goodness[0, :9] - expected).max() <= slack and np.isnan(goodness[0, 9:]).all() and np.isnan(goodness[2]).all()
    top = v.alternatives(1)
    assert top.substitution_classes[0, :9, 0].cpu().tolist() == np.argmax(want.sub, axis=1).tolist()
    assert np.abs(v.insertion_free().cpu().numpy()[0, :10] - (want.ll - np.logaddexp.reduce(want.ins, axis=1))).max() <= slack


@pytest.mark.parametrize("L", [600, 1024, 2100])
def test_lattice_kernel_variants(amd, yard, L):
    """The lattice kernel is instantiated for 1, 2, 4 and 8 strips per wave: 600, 1024 and 2100 targets take the last three
    (the tests above the first).  T = L + 8 frames; 8 slots x 5 classes are compared, and a short row shares the launch."""
    rng = np.random.default_rng(L)
    y = _targets(rng, L, 5, repeat=0.0)
    T = L + 8
    em = _emissions(2, T, 5, seed=L)
    slots = sorted({0, 1, 2 * L - 1, 2 * L, *rng.integers(0, 2 * L + 1, 4).tolist()})
    (_, _, _, status), _ = _check(yard, em, [T, 40], [y, _targets(rng, 7, 5)], slots=[slots, None])
    assert status.tolist() == [0, 0]


def test_long_row(amd, yard):
    """T = 1500, L = 300, C = 37 on 64 sampled cells: 16 slots, of each the four classes drawn for it."""
    rng = np.random.default_rng(16)
    em = _emissions(1, 1500, 37, seed=16, scale=3.0)
    y = _targets(rng, 300, 37)
    slots = sorted(rng.choice(601, 16, replace=False).tolist())
    call = _Call(em.cuda(), [1500], [0, 300], y, 300)
    call.run()
    ll, sub, ins, status = call.buffers()
    truth = V.variants_row(em[0].numpy(), y, 0, slots)
    for slot in slots:  # keep four cells of each computed row
        row = truth.sub[slot >> 1] if slot & 1 else truth.ins[slot >> 1]
        keep = rng.choice(37, 4, replace=False)
        dropped = np.setdiff1d(np.arange(37), keep)
        row[dropped] = np.nan
    compared, infinite = _compare((ll, sub, ins, status), [truth], [[]], yard, 0, where="long")
    assert compared == 64 and infinite == 0 and status[0] == 0
    assert abs(float(ll[0]) - U.score_row(em[0].numpy(), y, posteriors=False).ll) <= U.ll_bound(yard, float(ll[0]))


def _graph_case():
    rng = np.random.default_rng(19)
    em = _emissions(4, 150, 70, seed=19).cuda()
    lengths = [150, 77, 0, 9]
    rows = [_targets(rng, L, 70) for L in (70, 20, 0, 5)]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
    return em, lengths, offsets, [v for r in rows for v in r]


def test_two_runs_are_bitwise_equal(amd):
    em, lengths, offsets, ids = _graph_case()
    first, second = _Call(em, lengths, offsets, ids, 70), _Call(em, lengths, offsets, ids, 70)
    first.run()
    second.run()
    second.refill()
    second.run()
    for name, a, b in zip(NAMES, first.buffers(), second.buffers()):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert first.buffers()[3].tolist() == [0, 0, 0, 0]


def test_graph_capture(amd):
    """One amx_ctc_variants_emissions call captured on a single stream and replayed twice equals the eager result bit for bit."""
    em, lengths, offsets, ids = _graph_case()
    eager = _Call(em, lengths, offsets, ids, 70)
    eager.run()
    torch.cuda.synchronize()
    want = eager.buffers()
    captured = _Call(em, lengths, offsets, ids, 70)
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


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in ((a.log_likelihood, b.log_likelihood), (a.status, b.status), (a.targets, b.targets)))


def test_through_the_estimator(amd, yard):
    """Estimator.variants_device on the results of predict and of predict_long equals ctc_variants on the same output tensor
    bit for bit, and the cells hold the truth of the fetched log-probabilities."""
    from allophant_amd import spec as S, synthetic

    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5,
                            n_values=3)
    N = 3
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    try:
        batch = amd.Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long))
        tfi = synthetic.make_inventory(spec, 7, seed=2)
        for pred in (est.predict(batch, tfi), est.predict_long(batch, tfi, window_seconds=0.25, context_seconds=0.05, batch_windows=4)):
            frames = [int(v) for v in pred.lengths]
            classes = pred.outputs["phoneme"].shape[2]
            rng = np.random.default_rng(31)
            rows = [_targets(rng, min(5, frames[n] // 3), classes) for n in range(N)]
            got = est.variants_device(pred, {"phoneme": rows}, "phoneme")
            direct = amd.ctc_variants(pred.outputs["phoneme"].transpose(0, 1), pred.lengths, rows)
            assert got.log_likelihood.is_cuda and got.substitutions.shape == (N, max(len(r) for r in rows), classes) and _same(got, direct)
            host = pred.outputs["phoneme"].transpose(0, 1).cpu().numpy()
            status = got.status.cpu().tolist()
            for n, row in enumerate(rows):
                L = len(row)
                assert torch.equal(got.substitutions[n, :L].view(torch.int32), direct.substitutions[n, :L].view(torch.int32))
                assert torch.equal(got.insertions[n, :L + 1].view(torch.int32), direct.insertions[n, :L + 1].view(torch.int32))
                want = V.variants_row(host[n, :frames[n]], row)
                assert status[n] == want.status == 0
                _compare((got.log_likelihood.cpu().numpy()[n:n + 1], got.substitutions.cpu().numpy()[n:n + 1, :L],
                          got.insertions.cpu().numpy()[n:n + 1, :L + 1], np.array([0])), [want], [row], yard, 0, infeasible=True)
            found = est.variants(pred, rows, "phoneme", threshold=0.5)
            assert found == got.diagnose(0.5) and all(row is not None for row in found)
        with pytest.raises(ValueError, match="unknown output"):
            est.variants_device(pred, rows, "nope")
    finally:
        est.close()


def test_diagnose_recovers_planted_edits(amd):
    """Peaky emissions spell thirteen symbols, one frame each with a blank frame between (the peak 10 nats above the rest);
    the transcript has one of them substituted, one deleted and one inserted.  Each planted edit, undone, wins back one frame's
    peak (10 nats); an edit that undoes nothing moves the likelihood by path counts only (well under a nat).  At a threshold of
    half the peak exactly the three are reported, at their positions and with the spoken class."""
    from allophant_amd.evaluation import Action

    Cn = 12
    spoken = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 3, 5]
    T = 2 * len(spoken) + 1
    logits = torch.zeros(2, T, Cn)
    for f in range(T):
        logits[:, f, spoken[f // 2] if f % 2 else 0] = 10.0
    em = torch.log_softmax(logits, -1)
    transcript = list(spoken)
    transcript[2] = 9         # spoken 3
    del transcript[6]         # spoken 7, which now belongs into gap 6
    transcript.insert(10, 2)  # not spoken
    v = amd.ctc_variants(em.cuda(), None, [transcript, spoken])
    found = v.diagnose(threshold=5.0)
    assert [(kind, at, c) for kind, at, c, _ in found[0]] == [(Action.SUBSTITUTION, 2, 3), (Action.INSERTION, 6, 7),
                                                              (Action.DELETION, 10, 2)], found[0]
    assert all(9.0 < ratio < 11.0 for *_, ratio in found[0])
    assert found[1] == []  # the spoken sequence itself: nothing to report
    assert float(v.goodness()[1, :13].min()) > -0.01 and float(v.goodness()[0, 2]) < -5.0
    assert float(v.insertion_free()[1, :14].min()) > -0.01 and float(v.insertion_free()[0, 6]) < -5.0


def test_report_worst_ratios(amd, yard):
    """Not a check of its own: prints the worst ratios the tests above met (run with -s), each a multiple of the yardstick
    against the bound of 4."""
    print(f"\nyardstick E_ll = {yard.E_ll:.3e}; device worst: variant cells {WORST['cell']:.3f} x E_ll, ll {WORST['ll']:.3f} x E_ll "
          f"(bound 4), sub[l][y[l]] against the device's ll {WORST['own']:.3f} x E_ll")
    assert WORST["cell"] <= U.MARGIN and WORST["ll"] <= U.MARGIN
