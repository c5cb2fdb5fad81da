"""The CTC beam-search contract on the host (no GPU): the float64 restatement (tests/ctc_beam_util.py) against brute force
over every alignment, a hand-worked case, the threshold and pruning, and the host side of the device decoder (decoder
construction, argument checks, the C ABI's limits and bindings, and a kernel compiled without scratch or spills)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ctc_beam_util import beam_search, brute_force

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("seed", range(12))
def test_restatement_is_exact_without_pruning(seed, exp):
    """With a beam above the number of states and no threshold the n-best are the top n of the exact prefix scores: the
    log-sum-exp over all C^T alignments of each labelling."""
    rng = np.random.default_rng(seed)
    T, C = int(rng.integers(0, 7)), int(rng.integers(2, 5))
    em = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32).reshape(T, C)
    exact = brute_force(em, T, exp=exp)
    n = min(len(exact), 6)
    hyps = beam_search(em, T, beam_width=10 ** 6, n_best=n, exp=exp, threshold=np.inf)
    assert [tuple(h.tokens) for h in hyps] == [lab for lab, _ in exact[:n]]
    for h, (_, score) in zip(hyps, exact):
        assert abs(h.score - score) <= 1e-12 * max(1.0, abs(score))


def test_hand_worked_three_frames():
    """C = 2 (blank, a), log-probabilities as given.  Labelling "a" collects six alignments (bba -3.4, bab -0.6, baa -2.2,
    abb -3.7, aab -2.5, aaa -4.1: log-sum-exp -0.2029), "" one (bbb -1.8), "aa" one (aba -5.3)."""
    e = np.array([[-0.1, -2.0], [-1.5, -0.3], [-0.2, -1.8]], dtype=np.float32)
    f = e.astype(np.float64)
    b0, a0, b1, a1, b2, a2 = f[0, 0], f[0, 1], f[1, 0], f[1, 1], f[2, 0], f[2, 1]
    a = np.logaddexp.reduce([b0 + b1 + a2, b0 + a1 + b2, b0 + a1 + a2, a0 + b1 + b2, a0 + a1 + b2, a0 + a1 + a2])
    empty = b0 + b1 + b2
    aa = a0 + b1 + a2
    assert abs(a - (-0.20289)) < 1e-4 and abs(empty - (-1.8)) < 1e-6 and abs(aa - (-5.3)) < 1e-6
    hyps = beam_search(e, 3, beam_width=8, n_best=3, exp=False)
    assert [h.tokens for h in hyps] == [[1], [], [1, 1]]
    assert [h.timesteps for h in hyps] == [[2], [], [1, 3]]  # "a" keeps the path of its best alignment, b a b
    np.testing.assert_allclose([h.score for h in hyps], [a, empty, aa], rtol=1e-12)
    # probabilities (the reference's call): the same alignments, exp(e) added instead of e
    p = np.exp(f).astype(np.float32).astype(np.float64)
    hyps = beam_search(e, 3, beam_width=8, n_best=3, exp=True)
    pa = np.logaddexp.reduce([p[0, 0] + p[1, 0] + p[2, 1], p[0, 0] + p[1, 1] + p[2, 0], p[0, 0] + p[1, 1] + p[2, 1],
                              p[0, 1] + p[1, 0] + p[2, 0], p[0, 1] + p[1, 1] + p[2, 0], p[0, 1] + p[1, 1] + p[2, 1]])
    assert hyps[0].tokens == [1]
    assert abs(hyps[0].score - pa) < 1e-12


def test_threshold_drops_candidates_before_merging():
    """A candidate more than 50 below the frame's best is dropped: token 2 at -60 never starts a hypothesis."""
    e = np.array([[0.0, -1.0, -60.0], [-0.5, -0.7, -60.0]], dtype=np.float32)
    with_threshold = beam_search(e, 2, beam_width=16, n_best=16, exp=False)
    without = beam_search(e, 2, beam_width=16, n_best=16, exp=False, threshold=np.inf)
    assert not any(2 in h.tokens for h in with_threshold)
    assert any(2 in h.tokens for h in without)
    # the merged score of a labelling loses exactly the dropped members
    exact = dict(brute_force(e, 2, exp=False))
    for h in with_threshold:
        assert h.score <= exact[tuple(h.tokens)] + 1e-12


def test_end_threshold_cuts_against_the_best_merged_state():
    """Frame 1 merges two paths of "a" (0 and -0.01) to 0.688; "ca" (-49.5) passes the frame cut (-50), not the end cut."""
    e = np.array([[0.0, -0.01, -100.0, -49.5], [-100.0, 0.0, -100.0, -100.0]], dtype=np.float32)
    hyps = beam_search(e, 2, 8, 8, exp=False)
    assert [h.tokens for h in hyps] == [[1]] and abs(hyps[0].score - np.logaddexp(0.0, np.float32(-0.01))) < 1e-15
    assert [h.tokens for h in beam_search(e, 2, 8, 8, exp=False, end_threshold=np.inf)] == [[1], [3, 1]]


@pytest.mark.parametrize("beam", [1, 2, 3])
def test_pruning_keeps_a_subset_of_alignments(beam):
    """A pruned beam scores each labelling over a subset of its alignments: never above the exact score, sorted descending,
    at most beam_width hypotheses."""
    rng = np.random.default_rng(beam)
    em = np.log(rng.dirichlet(np.ones(3), size=6)).astype(np.float32)
    exact = dict(brute_force(em, 6, exp=False))
    hyps = beam_search(em, 6, beam_width=beam, n_best=beam, exp=False, threshold=np.inf)
    assert 1 <= len(hyps) <= beam
    assert all(h.score <= exact[tuple(h.tokens)] + 1e-12 for h in hyps)
    assert [h.score for h in hyps] == sorted((h.score for h in hyps), reverse=True)
    assert beam_search(em, 0, beam, beam) == [beam_search(em, 0, beam, 1)[0]]
    assert beam_search(em, 0, beam, beam)[0].score == 0.0


class _Indexer:
    feature_names = ["phoneme", "syllabic"]

    @staticmethod
    def feature_categories(name):
        return ["a", "b", "c"] if name == "phoneme" else ["+", "-"]


def test_feature_decoders_types_and_errors():
    from allophant_amd import estimator as E

    greedy = E.feature_decoders(_Indexer())
    assert all(type(d) is E.GreedyCTCDecoder for d in greedy.values())
    beams = E.feature_decoders(_Indexer(), beam_width=4, n_best=2)
    assert set(beams) == {"phoneme", "syllabic"}
    assert all(type(d) is E.BeamCTCDecoder for d in beams.values())
    assert beams["phoneme"]._tokens == ["<blank>", "a", "b", "c"]
    assert beams["syllabic"]._tokens == ["<blank>", "+", "-"]
    assert (beams["phoneme"]._beam_width, beams["phoneme"]._n_best) == (4, 2)
    assert list(E.feature_decoders(_Indexer(), 3, ["syllabic"])) == ["syllabic"]
    assert type(E._ctc_decoder(["a"], 1, 1)) is E.GreedyCTCDecoder
    with pytest.raises(ValueError):
        E.feature_decoders(_Indexer(), beam_width=2, n_best=3)
    with pytest.raises(ValueError):
        E._ctc_decoder(["a"], 1, 2)
    with pytest.raises(ValueError):
        E.BeamCTCDecoder(["<blank>", "a"], 65)
    with pytest.raises(RuntimeError):
        E.BeamCTCDecoder(["<blank>", "a", "b"], 4)(torch.zeros(1, 3, 3), torch.tensor([3]))
    with pytest.raises(RuntimeError):
        E.beam_ctc_decode(torch.zeros(1, 3, 3), torch.tensor([3]), 4)
    import allophant_amd

    assert allophant_amd.BeamCTCDecoder is E.BeamCTCDecoder


def test_binding_covers_the_beam_header():
    from allophant_amd import lib

    header = open(os.path.join(ROOT, "include", "allophant_amx_beam.h")).read()
    declared = re.findall(r"^int (amx_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(lib.BEAM_EXPORTS)
    assert int(re.search(r"#define AMX_BEAM_EXP_EMISSIONS (\d+)u", header).group(1)) == lib.BEAM_EXP_EMISSIONS
    source = open(os.path.join(ROOT, "allophant_amd", "lib.py")).read()
    for name in declared:
        assert f"lib.{name}.argtypes" in source and f"lib.{name}.restype" in source
    so = os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)
    if os.path.exists(so):
        handle = lib.load()
        assert all(hasattr(handle, name) for name in declared)


def test_c_abi_limits_without_a_device():
    """The limits are checked before any device work: AMX_EINVAL with a message."""
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    import ctypes as C

    h = lib.load()
    size = C.c_size_t()
    assert h.amx_beam_ctc_workspace(64, 32 * 40, 499, C.byref(size)) == lib.AMX_OK
    assert size.value == 32 * 40 * 499 * 64 * 4
    for beam in (0, 65):
        assert h.amx_beam_ctc_workspace(beam, 1, 1, C.byref(size)) == lib.AMX_EINVAL
    null = None

    def call(beam, n_best, Cn, blank, flags=1):
        return h.amx_beam_ctc_emissions(0, null, 0, 0, null, 1, 4, Cn, blank, beam, n_best, flags, null, 0, null, null, null,
                                        null, null, null)

    assert call(4, 5, 3, 0) == lib.AMX_EINVAL
    assert b"n_best" in h.amx_last_error(None)
    assert call(4, 0, 3, 0) == lib.AMX_EINVAL
    assert call(65, 1, 3, 0) == lib.AMX_EINVAL
    assert call(4, 1, 1, 0) == lib.AMX_EINVAL
    assert call(4, 1, 65536, 0) == lib.AMX_EINVAL
    assert call(4, 1, 3, 3) == lib.AMX_EINVAL
    assert call(4, 1, 3, 0, flags=2) == lib.AMX_EINVAL
    assert call(4, 1, 3, 0) == lib.AMX_EINVAL  # null buffers
    assert b"null" in h.amx_last_error(None)


def test_kernel_has_no_scratch(tmp_path):
    """amx_ctc_beam.hip compiled for gfx950: no scratch, no spilled VGPRs, no dynamic stack (hipcc's resource-usage
    report).  SGPR spills are tolerated up to a ceiling: the frame loop keeps more wave-uniform values live than the SGPR
    file holds (the fp64 exp / log1p constants and the row's pointers, hoisted out of the loop), and the compiler parks
    55 / 60 of them in VGPR lanes (v_writelane / v_readlane, no memory traffic).  The ceiling catches growth."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_beam.hip")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                           "-o", str(tmp_path / "amx_ctc_beam.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    report = done.stderr
    assert "beam_ctc_kernel" in report and "beam_ctc_emissions_kernel" in report
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", report)]
    assert len(scratch) == 2 and len(spills) == 2, report
    assert not any(scratch) and not any(spills), report
    assert "Dynamic Stack: True" not in report
    sgpr_spills = [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", report)]
    assert len(sgpr_spills) == 2 and max(sgpr_spills) <= 72, report
