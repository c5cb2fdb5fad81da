"""Inputs on which equal scores decide a CTC beam search (tie rule), shared by the host tests
(test_ctc_beam_ties.py) and the device tests (test_gpu_beam_ties.py), and the restatement's answer on each of them, computed
once per process.

Two kinds of input.  *Tied families* are continuous random emissions in which whole columns are duplicated (or are -inf, or
underflow to one exponential), so that equal scores come from the same sequence of operations and a comparison with the
restatement can be exact; a case names its family, sizes, beam, mode, language-model set-up and seed.  *Dyadic rows* are
tiny rows over {0, -0.25, -0.5, -1} for brute force over every alignment, where mathematically equal sums are computed in
different ways and only scores and sets are compared."""
import functools
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from ctc_beam_util import search

# 1000 x the 1e-9 score tolerance: no decision of a case rests on a difference two implementations could order differently
GAP = 1e-6
WEIGHTS = ((1.3, -0.4), (1.0, 0.0))


class Case(NamedTuple):
    family: str        # "columns", "constant", "dead", "dead_blank", "underflow", "sharp"
    C: int
    beam: int
    exp: bool
    seed: int
    T: int = 24
    arg: int = 0       # columns: largest group; dead: live classes
    lm: str = ""       # "", "addk", "groups", "flat", "forbid", "end", "rows"
    weights: int = 0   # index into WEIGHTS

    @property
    def id(self) -> str:
        parts = [self.family, f"C{self.C}", f"B{self.beam}", "exp" if self.exp else "log"]
        if self.arg:
            parts.insert(2, f"a{self.arg}")
        if self.lm:
            parts += [self.lm, f"w{self.weights}"]
        return "-".join(parts)

    @property
    def n_best(self) -> int:
        return self.beam if self.beam in (5, 64) else min(self.beam, 3)


def _log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def _groups(rng, C: int, largest: int) -> np.ndarray:
    """Class -> group, groups of 1 to ``largest`` classes scattered over the class indices."""
    sizes = []
    while sum(sizes) < C:
        sizes.append(min(int(rng.integers(1, largest + 1)), C - sum(sizes)))
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes))


def duplicated_columns(rng, layout, T: int, C: int, largest: int, scale: float = 2.0) -> Tuple[np.ndarray, np.ndarray]:
    """[T, C] fp32 log-probabilities over the groups, every class of a group with the group's column; and class -> group.
    ``layout`` is the generator that places the groups, ``rng`` the one that draws the values."""
    group = _groups(layout, C, largest)
    base = _log_softmax(rng.standard_normal((T, int(group.max()) + 1)) * scale).astype(np.float32)
    return base[:, group], group


def _one_exponential_pair(rng) -> Tuple[np.float32, np.float32]:
    """Two fp32 neighbours (one ulp apart, the lower first) with one fp32 exponential."""
    while True:
        x = np.float32(rng.uniform(-0.7, -0.05))
        y = np.nextafter(x, np.float32(0.0))
        if np.float32(np.exp(np.float64(x))) == np.float32(np.exp(np.float64(y))):
            return x, y


def _row(case: Case, rng, layout) -> Tuple[np.ndarray, np.ndarray]:
    """One utterance [T, C] and its class -> group map (classes of one group have equal columns as added; -1: a class of
    no group).  ``layout`` draws which classes are grouped, live or tied, ``rng`` the values."""
    T, C = case.T, case.C
    if case.family == "columns":
        return duplicated_columns(rng, layout, T, C, case.arg)
    if case.family == "constant":  # every third frame has all C emissions equal (the others: duplicated columns)
        em, group = duplicated_columns(rng, layout, T, C, max(1, C // 8))
        em[2::3] = np.float32(-np.log(C))
        return em, group
    if case.family in ("dead", "dead_blank"):  # a restricted union block: the blank and live - 1 others finite, the rest -inf
        live = np.concatenate([[0], 1 + np.sort(layout.permutation(C - 1)[:case.arg - 1])])
        columns, group = duplicated_columns(rng, layout, T, len(live), 2)
        em = np.full((T, C), -np.inf, dtype=np.float32)
        em[:, live] = columns
        full = np.full(C, -1)
        full[live] = group
        if case.family == "dead_blank":
            em[1::4, 0] = -np.inf
            full[0] = int(group.max()) + 1
        return em, full
    if case.family == "sharp":
        # log mode.  Every other frame is sharp: the blank at 0, ``arg`` classes at -40 (inside the threshold of 50, and so
        # far below that log1p(exp(-40)) vanishes in a merge), the rest at -60 (outside).  The frames between are constant.
        # After a sharp frame the beam holds the empty prefix and single tokens 40 below it; in the constant frame the
        # empty prefix's extensions onto those states merge to exactly the score of its other extensions and of its blank.
        em = np.full((T, C), np.float32(-np.log(C)), dtype=np.float32)
        low = 1 + np.sort(layout.permutation(C - 1)[:case.arg])
        em[0::2] = np.float32(-60.0)
        em[0::2, 0] = 0.0
        for c in low:
            em[0::2, c] = np.float32(-40.0)
        group = np.full(C, 1)
        group[0] = 0
        group[low] = 2
        return em, group
    assert case.family == "underflow" and case.exp
    # fewer than beam + 2 classes above the tied ones: a few ordinary classes (the blank among them), pairs one ulp apart
    # with one exponential (the lower raw value at the lower index), and distinct values in [-150, -104] that all add 0.0f
    ordinary, pairs = max(2, case.beam // 2), max(1, case.beam // 5)
    assert ordinary + 2 * pairs < case.beam + 2 < C
    places = 1 + layout.permutation(C - 1)
    em = rng.uniform(-150.0, -104.0, size=(T, C)).astype(np.float32)
    plain = np.concatenate([[0], places[:ordinary - 1]])
    em[:, plain] = _log_softmax(rng.standard_normal((T, ordinary)) * 2.0).astype(np.float32)
    group = np.full(C, -1)
    group[plain] = np.arange(ordinary)
    for p in range(pairs):
        lo, hi = sorted(places[ordinary - 1 + 2 * p:ordinary + 1 + 2 * p])
        for t in range(T):
            em[t, lo], em[t, hi] = _one_exponential_pair(rng)
        group[[lo, hi]] = ordinary + p
    assert np.all(np.exp(em[:, group < 0].astype(np.float64)).astype(np.float32) == 0.0)
    return em, group


def _group_table(rng, group: np.ndarray, scale: float = 3.0) -> np.ndarray:
    """A [C + 1, C + 1] fp32 table whose rows and columns repeat with the emission columns: classes of one group are one
    token to it (classes outside every group share one more)."""
    g = np.where(group < 0, group.max() + 1, group)
    G = int(g.max()) + 1
    base = _log_softmax(rng.standard_normal((G + 1, G + 1)) * scale).astype(np.float32)
    index = np.append(g, G)
    return base[index][:, index]


def _addk_table(C: int) -> np.ndarray:
    """PhonotacticLM's own add-k estimate from a handful of words: every unseen bigram of a row has one value."""
    from allophant_amd.phonotactics import PhonotacticLM

    words = [[1, 2, 3], [2, 2, 4], [4], [3, 1, 2, 3], [5, 1], [2, 3, 5, 5]]
    return PhonotacticLM.from_sequences(words, classes=C, smoothing=1.0).table.numpy()


class Inputs(NamedTuple):
    em: np.ndarray                         # [4, T, C] fp32
    lengths: List[int]
    tables: List[Optional[np.ndarray]]     # per row
    stack: List[np.ndarray]                # the distinct tables
    ids: List[int]                         # per row: index into stack, -1 for none
    weight: float
    bonus: float


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    rng = np.random.default_rng(case.seed)
    shared = case.lm in ("groups", "forbid", "end", "flat")  # one table for the four rows: they share one layout
    rows = [_row(case, rng, np.random.default_rng([case.seed, 1 if shared else 1 + n])) for n in range(4)]
    em = np.stack([r[0] for r in rows])
    T = case.T
    lengths = [T, 0, 1, T - 5]
    weight, bonus = WEIGHTS[case.weights]
    if not case.lm:
        return Inputs(em, lengths, [None] * 4, [], [-1] * 4, weight, bonus)
    if case.lm == "addk":
        stack, ids = [_addk_table(case.C)], [0] * 4
    elif case.lm == "rows":  # per-row tables, one row without
        stack, ids = [_group_table(rng, rows[3][1]), _group_table(rng, rows[0][1])], [1, 0, -1, 0]
    elif case.lm == "flat":  # every entry equal: with a constant frame every key of a prefix's list selection is equal
        stack, ids = [np.full((case.C + 1, case.C + 1), -2.0, dtype=np.float32)], [0] * 4
    else:
        group = rows[0][1]
        table = _group_table(rng, group)
        if case.lm == "forbid":  # of otherwise identical tokens one is forbidden: the lowest class of every other group
            # after every token and at the beginning (the rule must then pass it over), the highest of the rest at the beginning
            twins = [np.flatnonzero((group == g) & (np.arange(case.C) != 0)) for g in range(int(group.max()) + 1)]
            twins = [t for t in twins if len(t) >= 2]
            assert len(twins) >= 2
            for i, t in enumerate(twins):
                if i % 2 == 0:
                    table[:, int(t[0])] = -np.inf
                else:
                    table[case.C, int(t[-1])] = -np.inf
        if case.lm == "end":
            table[:, case.C] = np.float32(-1.5)
        stack, ids = [table], [0] * 4
    return Inputs(em, lengths, [None if i < 0 else stack[i] for i in ids], stack, ids, weight, bonus)


def token_lists(which: str, beam_width: int, blank: int = 0, reverse: bool = False):
    """The candidate reduction of the kernels, as a ``restrict`` function for ``search``: extensions are enumerated only for
    the top min(beam_width + 2, C) tokens by (value as added, then lower class index; higher when reversed).  "frame": one
    list per frame over all classes by the emission as added (amx_ctc_beam.hip).  "prefix": one list per prefix over its
    permitted non-blank tokens by the emission as added plus the table term (amx_ctc_beam_lm.hip)."""
    sign = -1 if reverse else 1

    def top(value, tokens, count):
        return tokens[np.lexsort((sign * tokens, -value[tokens]))[:count]]

    def restrict(e_t, a, permitted, lead):
        S, C = permitted.shape
        count = min(beam_width + 2, C)
        classes = np.arange(C)
        listed = np.zeros((S, C), dtype=bool)
        if which == "frame":
            listed[:, top(e_t, classes, count)] = True
            return listed
        assert which == "prefix"
        for j in np.flatnonzero(lead == np.arange(S)):
            tokens = np.flatnonzero(permitted[j] & (classes != blank))
            listed[np.ix_(np.flatnonzero(lead == j), top(e_t + a[j], tokens, count))] = True
        return listed

    return restrict


def reduced_search(which: str, em, length, beam_width, n_best, *args, reverse_ties: bool = False, **kwargs):
    """``search`` over the candidates that the kernel named by ``which`` enumerates (see ``token_lists``)."""
    return search(em, length, beam_width, n_best, *args, reverse_ties=reverse_ties,
                  restrict=token_lists(which, beam_width, kwargs.get("blank", 0), reverse_ties), **kwargs)


class Reference(NamedTuple):
    rows: list            # per utterance: the restatement's hypotheses under the tie rule
    reversed_rows: list   #   and under the reversed rule
    gaps: List[float]     # per utterance: the smaller of the two runs' gap reports


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> Reference:
    data = inputs(case)
    rows, reversed_rows, gaps = [], [], []
    for n in range(4):
        a, b = {}, {}
        args = (data.em[n], data.lengths[n], case.beam, case.n_best, data.tables[n], data.weight, data.bonus)
        rows.append(search(*args, exp=case.exp, report=a))
        reversed_rows.append(search(*args, exp=case.exp, reverse_ties=True, report=b))
        gaps.append(min(a["gap"], b["gap"]))
    return Reference(rows, reversed_rows, gaps)


def check_preconditions(case: Case) -> Reference:
    """What every exact comparison asserts on the host first: no decision rests on a difference below GAP, and the tie rule
    decides the result (the reversed rule gives other n-best)."""
    ref = reference(case)
    assert min(ref.gaps) >= GAP, (case.id, ref.gaps)
    assert ref.rows != ref.reversed_rows, case.id
    return ref


def _cases() -> List[Case]:
    cases = []
    for exp in (True, False):
        for beam in (1, 2, 5, 16):
            cases.append(Case("columns", 37, beam, exp, 0, arg=6))
        for beam in (16, 64):
            cases.append(Case("columns", 300, beam, exp, 0, arg=40))
        cases.append(Case("columns", 1025, 16, exp, 0, T=12, arg=40))
        cases.append(Case("columns", 4400, 16, exp, 0, T=8, arg=40))  # more classes than the plain kernel stages at a time
        for C, beam in ((3, 5), (37, 16), (300, 64)):
            cases.append(Case("constant", C, beam, exp, 0))
        for C, live in ((30, 7), (30, 23), (300, 5)):
            for beam in (5, 16, 64):
                cases.append(Case("dead", C, beam, exp, 0, arg=live))
    cases.append(Case("dead_blank", 30, 16, False, 0, arg=7))
    for C, beam in ((20, 5), (40, 16), (100, 64)):
        cases.append(Case("underflow", C, beam, True, 0))
    # states of one beam 40 apart inside the threshold: B - 1 and B + 5 low classes, the list cut among the tied extensions
    for C, beam, low in ((10, 4, 3), (37, 5, 4), (37, 16, 21), (300, 64, 63)):
        cases.append(Case("sharp", C, beam, False, 0, T=6, arg=low))
    return cases


def _lm_cases() -> List[Case]:
    return [Case("columns", 12, 5, False, 0, arg=3, lm="addk", weights=0),
            Case("columns", 12, 16, True, 0, arg=3, lm="addk", weights=1),
            Case("columns", 37, 16, False, 0, arg=6, lm="groups", weights=0),
            Case("columns", 37, 5, True, 0, arg=6, lm="groups", weights=1),
            Case("columns", 300, 16, False, 0, arg=40, lm="groups", weights=0),
            Case("columns", 300, 64, False, 0, arg=40, lm="groups", weights=1),
            Case("constant", 300, 16, False, 0, lm="flat", weights=0),
            Case("constant", 300, 64, True, 0, lm="flat", weights=1),
            Case("columns", 37, 16, False, 0, arg=6, lm="forbid", weights=0),
            Case("columns", 37, 16, False, 0, arg=6, lm="forbid", weights=1),
            Case("columns", 37, 16, False, 0, arg=6, lm="end", weights=0),
            Case("columns", 37, 16, False, 0, arg=6, lm="rows", weights=0),
            Case("columns", 300, 16, True, 0, arg=40, lm="rows", weights=1),
            Case("dead", 30, 16, False, 0, arg=7, lm="groups", weights=0),
            Case("sharp", 37, 5, False, 0, T=6, arg=4, lm="flat", weights=0),
            Case("sharp", 37, 16, False, 0, T=6, arg=21, lm="groups", weights=1)]


# A seed that violates a precondition is replaced here, not tolerated in a test.
SEEDS = {"dead-C30-a7-B16-log-groups-w0": 2}

CASES = [c._replace(seed=SEEDS.get(c.id, 0)) for c in _cases()]
LM_CASES = [c._replace(seed=SEEDS.get(c.id, 0)) for c in _lm_cases()]


def sharp_row() -> np.ndarray:
    """C = 10, T = 2, for beam 4 in log mode: a sharp frame (the blank at 0, classes 1 to 3 at -40, the rest at -60) and a
    constant one.  In frame 1 the empty prefix's extensions by 1, 2, 3 land on beam states 40 below it, whose own member
    vanishes in the merge, so they tie exactly with its extensions by 4 to 9 and with its blank successor."""
    em = np.full((2, 10), -np.log(10.0), dtype=np.float32)
    em[0] = -60.0
    em[0, 0] = 0.0
    em[0, 1:4] = -40.0
    return em


def dyadic_rows() -> List[Tuple[str, np.ndarray]]:
    """Tiny tied rows for brute force: C in 2..4, T <= 6, emissions drawn from {0, -0.25, -0.5, -1} and from duplicated
    columns.  Sizes at which a beam of 64 drops nothing (asserted where that is relied on)."""
    values = np.array([0.0, -0.25, -0.5, -1.0], dtype=np.float32)
    rows = []
    for C, T in ((2, 6), (3, 5), (3, 4), (4, 3), (3, 3)):
        for seed in range(3):
            rng = np.random.default_rng(1000 * C + 10 * T + seed)
            em = values[rng.integers(0, 4, size=(T, C))]
            if seed == 1 and C > 2:   # two non-blank classes share a column
                em[:, C - 1] = em[:, 1]
            if seed == 2:             # one constant frame, and the blank's column shared too
                em[T // 2] = values[1]
                em[:, C - 1] = em[:, 0]
            rows.append((f"C{C}-T{T}-{seed}", em))
    return rows


def dyadic_table(C: int, seed: int) -> np.ndarray:
    """A [C + 1, C + 1] table over the same dyadic values, with one forbidden bigram when there is room for one."""
    rng = np.random.default_rng(77 + 10 * C + seed)
    table = np.array([0.0, -0.25, -0.5, -1.0], dtype=np.float32)[rng.integers(0, 4, size=(C + 1, C + 1))]
    if C > 2:
        table[1, 2] = -np.inf
    return table
