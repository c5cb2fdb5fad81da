"""A forward pass never depends on what the handle ran before.

Every accuracy test of the forward pass builds a fresh ``Estimator``, runs one batch and closes it; production keeps one handle for
a corpus.  Its workspaces only grow, and every pass runs on top of what earlier passes -- of another geometry, row layout, plane
stride or inventory -- left there: padding rows and columns of the Q / K / V planes that are "still zero", rows behind the packed
ones that are "read, never used", conv rows in an utterance's padding that are left unwritten, the slack behind every plane buffer,
the fold's statistics, the split-K slabs, the ``kpad`` tails of the heads' operands.  On a fresh handle a read of something the pass
did not write mostly meets zero pages and shows nowhere.

The kernels are deterministic (no atomics on the data path; replays are bitwise the eager pass: tests/test_gpu_graph.py), so the
property is held with NO tolerance: the whole flat output buffer of a pass -- the zeros of the frames beyond ``lengths``
included -- the frame lengths and the plan (``pass_info()``: ``ln_fold``, ``packed``, ``attention``, ``rows``) are those of a clean
pass of the same case (``history_util.reference``), whatever the handle ran before and whatever its workspaces hold:

* ``test_scribbled_workspaces``: every data workspace filled with finite garbage over its whole allocation
  (``Estimator._debug_scribble``: 65504 / 2.7e36 and 1.1 / 0.014, as fp16 / bf16 and fp32 read them) in front of the pass;
* ``test_history_walk``: eager passes in an order in which every case follows every other one;
* ``test_history_walk_recorded``: the same order with passes recorded and replayed between the changes;
* ``test_the_hook_scribbles``: the hook does reach a buffer a pass has just written, so the first test is not vacuous.

This is also the one sharp statement about the single-plane modes (``f16``, ``bf16``), whose accuracy bounds are 6e-2 / 5e-1.
The clean pass itself is held to float64 at these geometries by the stage tests; this file adds that nothing else can come out.
Models, cases and their ``pass_info()`` pins: tests/history_util.py; DESIGN.md, "History independence".
"""
import pytest
import torch

from tests import history_util as HU

pytestmark = pytest.mark.gpu
RUNS = pytest.mark.parametrize("name,precision", HU.RUNS, ids=[f"{m}-{p}" for m, p in HU.RUNS])


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def veteran(amd, model, precision):
    """a handle that has run the model's largest case: no later case grows a workspace, every one runs on what is there"""
    handle = HU.Handle(amd, model, precision)
    try:
        HU.assert_same(handle.run(model.cases[0], eager=True), HU.reference(amd, model, precision, model.cases[0]),
                       f"{model.name}/{precision} case {model.cases[0].name!r}, first pass of the veteran")
    except BaseException:
        handle.close()
        raise
    return handle


@RUNS
def test_scribbled_workspaces(amd, name, precision):
    model = HU.model(name)
    with veteran(amd, model, precision) as handle:
        for case in model.cases:
            want = HU.reference(amd, model, precision, case)
            for pattern in HU.PATTERNS:
                handle.scribble(pattern)
                got = handle.run(case, eager=True)
                handle.est.check_finite()
                HU.assert_same(got, want, f"{name}/{precision} case {case.name!r} on workspaces filled with {pattern:#06x}")


def walk_of(model):
    """the cases in an order in which every ordered pair of distinct cases is adjacent: n (n - 1) + 1 passes"""
    n = len(model.cases)
    walk = HU.pair_walk(n)
    assert len(walk) == n * (n - 1) + 1
    assert set(zip(walk, walk[1:])) == {(a, b) for a in range(n) for b in range(n) if a != b}
    return [model.cases[i] for i in walk]


@RUNS
def test_history_walk(amd, name, precision):
    model = HU.model(name)
    with veteran(amd, model, precision) as handle:
        before = model.cases[0]
        for case in walk_of(model):
            HU.assert_same(handle.run(case, eager=True), HU.reference(amd, model, precision, case),
                           f"{name}/{precision} case {case.name!r} behind {before.name!r}")
            before = case


@RUNS
def test_history_walk_recorded(amd, name, precision):
    """default flags, each case three times in a row: noted, recorded and replayed between the changes of geometry"""
    model = HU.model(name)
    with veteran(amd, model, precision) as handle:
        before = model.cases[0]
        modes = set()
        for case in walk_of(model):
            want = HU.reference(amd, model, precision, case)
            for repeat in range(3):
                got = handle.run(case, eager=False)
                modes.add(got.info["graph"])
                HU.assert_same(got, want, f"{name}/{precision} case {case.name!r} behind {before.name!r}, pass {repeat + 1} of 3 "
                                          f"({('eager', 'recorded', 'replayed')[got.info['graph']]})")
            before = case
        captures, replays = handle.est.graph_info()
        assert captures > 0 and replays > 0 and modes == {0, 1, 2}, (captures, replays, modes)


@RUNS
def test_the_hook_scribbles(amd, name, precision):
    """after a ``_keep_hidden`` pass the conv output the pass kept is the pattern, word for word -- and the next pass is clean"""
    model = HU.model(name)
    case = next(c for c in model.cases if c.name in ("pk2/keep", "ragged"))
    kept = HU.Case("kept", case.audio, case.lengths, flags={"_keep_hidden": True})
    with veteran(amd, model, precision) as handle:
        handle.run(kept, eager=True)
        conv = handle.est.debug_fetch("conv")
        assert conv.isfinite().all() and conv.abs().max() > 0
        handle.scribble(0x7BFF)
        words = handle.est.debug_fetch("conv").view(torch.int16)
        assert words.numel() == 2 * conv.numel() and bool((words == 0x7BFF).all())
        HU.assert_same(handle.run(case, eager=True), HU.reference(amd, model, precision, case),
                       f"{name}/{precision} case {case.name!r} right behind the scribble")
