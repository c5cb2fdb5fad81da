"""Equal scores in the CTC beam-search contract, on the host (no GPU): the two float64 restatements (tests/ctc_beam_util.py,
tests/ctc_beam_lm_util.py) with the tie rule of DESIGN 9 against brute force over every alignment on tiny tied rows; the
candidate reduction of the two kernels (the top beam + 2 token lists) against full enumeration on the tied input families
of the device tests (tests/ctc_beam_ties_util.py); and, for each of those inputs, that no decision rests on a near-tie and
that the tie rule decides the result."""
import numpy as np
import pytest

import ctc_beam_ties_util as U
from ctc_beam_lm_util import beam_search_lm, brute_force_lm, lm_score
from ctc_beam_util import beam_search, brute_force, emissions_as_added, search

ROWS = U.dyadic_rows()


def _lowest_alignment(e, table_terms, hyp, blank=0):
    """The lowest total among the alignments that collapse to the hypothesis's labelling with its timesteps (each token
    first emitted in the frame it reports).  ``e``: [T, C] emissions as added; ``table_terms``: what the labelling's
    tokens and end cost under a table (0 without one)."""
    T, C = e.shape
    lowest = np.inf
    for a in np.ndindex(*([C] * T)):
        lab, ts, prev = [], [], blank
        for t, n in enumerate(a):
            if n != blank and n != prev:
                lab.append(n)
                ts.append(t + 1)
            prev = n
        if lab == hyp.tokens and ts == hyp.timesteps:
            lowest = min(lowest, float(sum(e[t, a[t]] for t in range(T))))
    assert np.isfinite(lowest), hyp
    return lowest + table_terms


def _against_brute_force(hyps, exact, report, complete, e=None, terms=lambda tokens: 0.0):
    """Labellings distinct, scores descending.  Where nothing was dropped: every score within 1e-9 relative of the exact
    one, and exactly brute force's set of labellings.  Where candidates were dropped the beam has summed a labelling over a
    subset of its alignments, so equality is not owed; the score is then bounded from both sides: at most the exact one,
    and at least the total of one alignment -- the path the hypothesis reports is among the alignments with its timesteps,
    and every merge is at least its highest member, so the lowest of those alignments bounds the score from below (a merge
    that lost its highest member, or a path traced to the wrong frames, falls outside)."""
    scores = dict(exact)
    labellings = [tuple(h.tokens) for h in hyps]
    assert len(set(labellings)) == len(labellings)
    assert [h.score for h in hyps] == sorted((h.score for h in hyps), reverse=True)
    if report["dropped"] == 0:
        for h in hyps:
            want = scores[tuple(h.tokens)]
            assert abs(h.score - want) <= 1e-9 * max(1.0, abs(want)), (h.tokens, h.score, want)
        assert set(labellings) == set(scores)
    else:
        assert not complete
        for h in hyps:
            want = scores[tuple(h.tokens)]
            assert h.score <= want + 1e-9 * max(1.0, abs(want)), h.tokens
            low = _lowest_alignment(e, terms(h.tokens), h)
            assert h.score >= low - 1e-9 * max(1.0, abs(low)), (h.tokens, h.score, low)


@pytest.mark.parametrize("reverse", [False, True], ids=["rule", "reversed"])
@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("name,em", ROWS, ids=[name for name, _ in ROWS])
def test_tied_rows_against_brute_force(name, em, exp, reverse):
    """A beam of 64 drops nothing on these rows (asserted), so every labelling appears with its exact score, under either
    tie order; beams of 3 and 8 do drop, and then each score lies between one alignment's total and the exact one (see
    ``_against_brute_force``)."""
    T = em.shape[0]
    exact = brute_force(em, T, exp=exp)
    e = emissions_as_added(em, exp)
    for beam in (64, 8, 3):
        report = {}
        hyps = beam_search(em, T, beam, beam, exp=exp, reverse_ties=reverse, report=report)
        _against_brute_force(hyps, exact, report, complete=beam == 64, e=e)


@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.5, -0.25)], ids=["w1", "w.5"])
@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("name,em", ROWS, ids=[name for name, _ in ROWS])
def test_tied_rows_with_a_table_against_brute_force(name, em, exp, weights):
    T, C = em.shape
    table = U.dyadic_table(C, T)
    exact = brute_force_lm(em, T, table, *weights, exp=exp)
    e = emissions_as_added(em, exp)

    def terms(tokens):
        return lm_score(tuple(tokens), table, *weights)

    for beam in (64, 8, 3):
        for reverse in (False, True):
            report = {}
            hyps = beam_search_lm(em, T, beam, beam, table, *weights, exp=exp, reverse_ties=reverse, report=report)
            _against_brute_force(hyps, exact, report, complete=beam == 64, e=e, terms=terms)


def test_the_tie_rule_decides_a_hand_worked_row():
    """C = 3, beam 1, both tokens equal in frame 0: the rule keeps the extension by the lower class, the reversed rule the
    higher; with the blank tied too, the extension (kind 1) comes before the blank successor (kind 2)."""
    em = np.array([[-2.0, -0.5, -0.5], [-0.1, -3.0, -3.0]], dtype=np.float32)
    assert beam_search(em, 2, 1, 1, exp=False)[0].tokens == [1]
    assert beam_search(em, 2, 1, 1, exp=False, reverse_ties=True)[0].tokens == [2]
    flat = np.zeros((1, 3), dtype=np.float32)
    assert beam_search(flat, 1, 1, 1, exp=False)[0].tokens == [1]
    assert beam_search(flat, 1, 1, 1, exp=False, reverse_ties=True)[0].tokens == []
    report = {}
    # slots follow that order, and the end step ranks equal scores by slot
    assert [h.tokens for h in beam_search(flat, 1, 3, 3, exp=False, report=report)] == [[1], [2], []]
    assert report == {"gap": 1.0, "dropped": 0}  # the only unequal comparison: a score of 0 against the threshold's -50


@pytest.mark.parametrize("case", U.CASES + U.LM_CASES, ids=[c.id for c in U.CASES + U.LM_CASES])
def test_preconditions_of_the_exact_comparison(case):
    """No decision rests on a difference below 1e-6 relative, and the reversed rule gives other n-best."""
    U.check_preconditions(case)


@pytest.mark.parametrize("case", U.CASES + U.LM_CASES, ids=[c.id for c in U.CASES + U.LM_CASES])
def test_reduced_candidates_equal_full_enumeration(case):
    """The kernels enumerate extensions only for the top beam + 2 tokens (one list per frame without a table, one per prefix
    with one): under the tie rule that gives exactly the hypotheses of full enumeration, tokens, scores and timesteps.
    Under the reversed rule too, except in the "sharp" family: there an extension onto a beam state ties exactly with
    extensions off the list, and only the rule's own order of kinds (beam states first) makes the lists exact."""
    data, ref = U.inputs(case), U.reference(case)
    for n in range(4):
        args = (data.em[n], data.lengths[n], case.beam, case.n_best, data.tables[n], data.weight, data.bonus)
        lists = ["prefix"] if data.tables[n] is not None else ["frame", "prefix"]
        for which in lists:
            assert U.reduced_search(which, *args, exp=case.exp) == ref.rows[n], (n, which)
            if case.family != "sharp":
                backwards = U.reduced_search(which, *args, exp=case.exp, reverse_ties=True)
                assert backwards == ref.reversed_rows[n], (n, which)


def test_an_extension_onto_a_far_lower_beam_state_comes_before_the_other_extensions():
    """``sharp_row`` at beam 4.  Successors of beam states come first (kind 0), so of the candidates tied in frame 1 the
    four survivors are [1], [2], [3] and the lowest other extension, [4]; and with lists of beam + 2 = 6 tokens (classes 0
    to 5 here) both reductions find the same four.  Were beam states ordered after the extensions, full enumeration would
    keep [4] to [7], of which the lists hold only [4] and [5]."""
    em = U.sharp_row()
    report = {}
    full = search(em, 2, 4, 4, exp=False, report=report)
    assert [h.tokens for h in full] == [[1], [2], [3], [4]]
    assert len({h.score for h in full}) == 1 and report["gap"] >= U.GAP
    assert [h.timesteps for h in full] == [[2]] * 4  # the path of the highest member: the extension in frame 1
    for which in ("frame", "prefix"):
        assert U.reduced_search(which, em, 2, 4, 4, exp=False) == full
    assert [h.tokens for h in search(em, 2, 4, 4, exp=False, reverse_ties=True)] == [[7], [8], [9], []]
