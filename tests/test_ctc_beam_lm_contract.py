"""The CTC beam-search contract with a phonotactic language model, on the host (no GPU): the float64 restatement
(tests/ctc_beam_lm_util.py) against the restatement without a language model at weight 0 and against brute force over every
alignment, a hand-worked case in which the language model flips the best hypothesis, forbidden (-inf) transitions,
``PhonotacticLM`` and its builders, and the host side of the device decoder (bindings, the C ABI's limits, and a kernel
compiled without scratch or spills inside the LDS of one CU)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ctc_beam_lm_util import beam_search_lm, brute_force_lm
from ctc_beam_util import beam_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(seed, T, C, scale=1.0):
    rng = np.random.default_rng(seed)
    em = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32).reshape(T, C)
    table = (np.log(rng.dirichlet(np.ones(C + 1), size=C + 1)) * scale).astype(np.float32)
    return em, table


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("seed", range(8))
def test_weight_zero_is_the_decoder_without_a_language_model(seed, exp):
    em, table = _inputs(seed, T=7, C=2 + seed % 4)
    for beam in (1, 3, 50):
        want = beam_search(em, 7, beam, beam, exp=exp)
        got = beam_search_lm(em, 7, beam, beam, table, 0.0, 0.0, exp=exp)
        assert got == want  # tokens, scores and timesteps, exactly
        assert beam_search_lm(em, 7, beam, beam, None, 1.0, 0.5, exp=exp) == want


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("seed", range(20))
def test_restatement_is_exact_without_pruning(seed, exp):
    """With an unbounded beam and no threshold the n-best are the top n of the exact fused scores: each labelling's
    log-sum-exp over all C^T alignments plus its language-model, bonus and end terms."""
    rng = np.random.default_rng(100 + seed)
    T, C = int(rng.integers(0, 7)), int(rng.integers(2, 5))
    em, table = _inputs(seed, T, C)
    weight, bonus = float(rng.uniform(0.2, 1.5)), float(rng.uniform(-0.5, 0.5))
    exact = brute_force_lm(em, T, table, weight, bonus, exp=exp)
    n = min(len(exact), 6)
    hyps = beam_search_lm(em, T, 10 ** 6, n, table, weight, bonus, exp=exp, threshold=np.inf)
    assert [tuple(h.tokens) for h in hyps] == [lab for lab, _ in exact[:n]]
    for h, (_, score) in zip(hyps, exact):
        assert abs(h.score - score) <= 1e-12 * max(1.0, abs(score))


def test_hand_worked_three_frames_where_the_language_model_flips_the_top():
    """C = 3 (blank, a, b), log-probabilities as given.  Frame 0 prefers a to b by 0.8 and the other frames are blank, so
    without a language model "a" wins.  The table charges begin -> a 3.0 and begin -> b 0.2 (ends alike, 0.5), so with it
    "b" wins: each labelling's six alignments (x _ _, x x _, x x x, _ x _, _ x x, _ _ x) plus its bigram and end terms."""
    e = np.array([[-2.0, -0.4, -1.2], [-0.3, -2.5, -2.5], [-0.2, -3.0, -3.0]], dtype=np.float32)
    f = e.astype(np.float64)
    table = np.zeros((4, 4), dtype=np.float32)
    table[3] = [0.0, -3.0, -0.2, -4.0]  # begin -> (blank, unused), a, b, end
    table[1] = [0.0, -1.0, -1.0, -0.5]
    table[2] = [0.0, -1.0, -1.0, -0.5]
    t64 = table.astype(np.float64)

    def acoustic(x):
        return np.logaddexp.reduce([f[0, x] + f[1, 0] + f[2, 0], f[0, x] + f[1, x] + f[2, 0], f[0, x] + f[1, x] + f[2, x],
                                    f[0, 0] + f[1, x] + f[2, 0], f[0, 0] + f[1, x] + f[2, x], f[0, 0] + f[1, 0] + f[2, x]])

    plain = beam_search(e, 3, 64, 3, exp=False)
    assert [h.tokens for h in plain[:2]] == [[1], [2]]
    np.testing.assert_allclose([h.score for h in plain[:2]], [acoustic(1), acoustic(2)], rtol=1e-12)
    fused = beam_search_lm(e, 3, 64, 3, table, 1.0, 0.0, exp=False)
    want_a = acoustic(1) + t64[3, 1] + t64[1, 3]
    want_b = acoustic(2) + t64[3, 2] + t64[2, 3]
    assert want_b > want_a and acoustic(1) > acoustic(2)  # the case really flips
    assert [h.tokens for h in fused[:2]] == [[2], [1]]
    np.testing.assert_allclose([h.score for h in fused[:2]], [want_b, want_a], rtol=1e-12)
    assert fused[0].timesteps == [1]
    # the bonus counts tokens: the empty labelling gets none
    bonus = beam_search_lm(e, 3, 64, 64, table, 1.0, 0.75, exp=False)
    by_tokens = {tuple(h.tokens): h.score for h in bonus}
    assert abs(by_tokens[(2,)] - (want_b + 0.75)) < 1e-12
    assert abs(by_tokens[()] - (f[0, 0] + f[1, 0] + f[2, 0] + t64[3, 3])) < 1e-12


@pytest.mark.parametrize("weight", [1.0, 0.0])
def test_an_infinite_entry_forbids_its_bigram_at_every_weight(weight):
    em, table = _inputs(3, T=6, C=4)
    table[1, 2] = -np.inf   # no "1 2"
    table[4, 3] = -np.inf   # nothing begins with 3
    hyps = beam_search_lm(em, 6, 10 ** 6, 10 ** 6, table, weight, 0.0, exp=False, threshold=np.inf)
    assert len(hyps) > 10
    for h in hyps:
        assert h.tokens[:1] != [3]
        assert all((p, n) != (1, 2) for p, n in zip(h.tokens, h.tokens[1:]))
        assert math.isfinite(h.score)
    assert any(3 in h.tokens for h in hyps) and any(2 in h.tokens for h in hyps)
    free = beam_search_lm(em, 6, 10 ** 6, 10 ** 6, np.zeros_like(table), weight, 0.0, exp=False, threshold=np.inf)
    assert len(free) > len(hyps)


def test_an_infinite_end_entry_drops_the_state():
    em, table = _inputs(4, T=5, C=3)
    table[2, 3] = -np.inf  # no hypothesis ends in 2
    for weight in (1.0, 0.0):
        hyps = beam_search_lm(em, 5, 10 ** 6, 10 ** 6, table, weight, 0.0, exp=False, threshold=np.inf)
        assert hyps and all(h.tokens[-1:] != [2] for h in hyps)
    table[:, 3] = -np.inf  # nothing may end
    assert beam_search_lm(em, 5, 8, 8, table, 1.0, 0.0, exp=False) == []
    assert beam_search_lm(em, 0, 8, 8, table, 1.0, 0.0, exp=False) == []


def test_from_sequences_rows_are_distributions():
    from allophant_amd.phonotactics import PhonotacticLM

    sequences = [[1, 2, 3], [2, 2, 4], [4], [], [3, 1, 2, 3]]
    for blank, smoothing in ((0, 1.0), (0, 0.25), (5, 1.0)):
        shifted = [[t if blank == 0 else t - 1 for t in s] for s in sequences]
        lm = PhonotacticLM.from_sequences(shifted, classes=6, blank=blank, smoothing=smoothing)
        assert lm.classes == 6 and lm.blank == blank and lm.table.dtype == torch.float32 and lm.table.shape == (7, 7)
        events = [c for c in range(7) if c != blank]
        rows = [p for p in range(7) if p != blank]
        sums = lm.table[rows][:, events].double().exp().sum(1)
        assert torch.allclose(sums, torch.ones_like(sums), atol=1e-6)
    lm = PhonotacticLM.from_sequences(sequences, classes=6, smoothing=1.0)
    # begin -> 2 was seen once among five beginnings, over six events
    assert abs(float(lm.table[6, 2]) - math.log((1 + 1) / (5 + 6))) < 1e-6
    assert abs(float(lm.table[2, 3]) - math.log((2 + 1) / (4 + 6))) < 1e-6
    assert abs(float(lm.table[6, 6]) - math.log((1 + 1) / (5 + 6))) < 1e-6  # the empty sequence: begin -> end
    unsmoothed = PhonotacticLM.from_sequences(sequences, classes=6, smoothing=0.0)
    assert float(unsmoothed.table[1, 4]) == -math.inf and float(unsmoothed.table[5, 1]) == -math.inf  # unseen, and a row without counts
    counts = torch.zeros(7, 7)
    counts[6, 1] = 3
    counts[1, 6] = 3
    assert abs(float(PhonotacticLM.from_counts(counts, smoothing=0.5).table[6, 1]) - math.log(3.5 / (3 + 0.5 * 6))) < 1e-6
    with pytest.raises(ValueError):
        PhonotacticLM.from_sequences([[0, 1]], classes=6)  # the blank is no phoneme
    with pytest.raises(ValueError):
        PhonotacticLM.from_sequences([[6]], classes=6)


ARPA = """\\data\\
ngram 1=5
ngram 2=3

\\1-grams:
-99 <s> -0.30
-0.70 </s>
-0.50 a -0.20
-0.40 b -0.10
-1.00 c

\\2-grams:
-0.25 <s> a
-0.15 a b
-0.35 b </s>

\\end\\
"""


def test_from_arpa_backoff_sentence_marks_and_unknown_symbols(tmp_path):
    from allophant_amd.phonotactics import PhonotacticLM

    lm = PhonotacticLM.from_arpa(ARPA, ["<blank>", "a", "b", "c", "zh"])
    ln10 = math.log(10.0)
    table = lm.table.double()
    assert lm.classes == 5 and lm.blank == 0
    assert abs(float(table[5, 1]) - -0.25 * ln10) < 1e-6                    # <s> a
    assert abs(float(table[5, 2]) - (-0.30 + -0.40) * ln10) < 1e-6         # backoff(<s>) + unigram(b)
    assert abs(float(table[1, 2]) - -0.15 * ln10) < 1e-6                    # a b
    assert abs(float(table[1, 1]) - (-0.20 + -0.50) * ln10) < 1e-6         # backoff(a) + unigram(a)
    assert abs(float(table[2, 5]) - -0.35 * ln10) < 1e-6                    # b </s>
    assert abs(float(table[3, 5]) - (0.0 + -0.70) * ln10) < 1e-6           # c has no backoff weight
    assert abs(float(table[5, 5]) - (-0.30 + -0.70) * ln10) < 1e-6
    assert bool((table[4, 1:] == -math.inf).all()) and bool((table[[1, 2, 3, 5], 4] == -math.inf).all())  # "zh" is not in the file
    path = tmp_path / "lm.arpa"
    path.write_text(ARPA)
    assert torch.equal(PhonotacticLM.from_arpa(str(path), ["<blank>", "a", "b", "c", "zh"]).table, lm.table)
    unigram = "\\data\\\nngram 1=3\n\n\\1-grams:\n-0.3 a\n-0.5 b\n-0.6 </s>\n\n\\end\\\n"
    flat = PhonotacticLM.from_arpa(unigram, ["<blank>", "a", "b"]).table
    assert abs(float(flat[1, 2]) - -0.5 * ln10) < 1e-6 and abs(float(flat[2, 3]) - -0.6 * ln10) < 1e-6
    assert float(flat[3, 1]) == -math.inf  # no <s> in the file: nothing may begin
    with pytest.raises(ValueError):
        PhonotacticLM.from_arpa(ARPA.replace("ngram 2=3", "ngram 2=3\nngram 3=1"), ["<blank>", "a", "b"])
    with pytest.raises(ValueError):
        PhonotacticLM.from_arpa(ARPA.replace("\\end\\", "\\3-grams:\n-0.1 a b c\n\n\\end\\"), ["<blank>", "a", "b"])
    with pytest.raises(ValueError):
        PhonotacticLM.from_arpa("not a language model\nat all", ["<blank>", "a", "b"])


def test_restrict_stack_and_refusals():
    import allophant_amd
    from allophant_amd import estimator as E
    from allophant_amd.phonotactics import PhonotacticLM

    assert allophant_amd.PhonotacticLM is PhonotacticLM is E.PhonotacticLM and "PhonotacticLM" in allophant_amd.__all__
    _, table = _inputs(9, T=1, C=6)
    lm = PhonotacticLM(table)
    part = lm.restrict(torch.tensor([0, 4, 2]))
    assert part.classes == 3 and part.blank == 0
    index = [0, 4, 2, 6]
    assert torch.equal(part.table, torch.from_numpy(table)[index][:, index])
    assert lm.restrict([3, 0, 5]).blank == 1
    for bad in ([1, 2], [0, 2, 2], [0, 6]):  # no blank, a class twice, begin / end is no class
        with pytest.raises(ValueError):
            lm.restrict(bad)
    other = PhonotacticLM(table * 0.5)
    stack = PhonotacticLM.stack([lm, other])
    assert stack.shape == (2, 7, 7) and stack.is_contiguous() and torch.equal(stack[1], other.table)
    with pytest.raises(ValueError):
        PhonotacticLM.stack([lm, part])  # class-count mismatch
    with pytest.raises(ValueError):
        PhonotacticLM.stack([lm, PhonotacticLM(table, blank=2)])
    with pytest.raises(ValueError):
        PhonotacticLM.stack([])
    assert lm.to("cpu").table.device.type == "cpu" and lm.to("cpu").blank == 0
    for value in (np.nan, np.inf):
        broken = table.copy()
        broken[2, 3] = value
        with pytest.raises(ValueError):
            PhonotacticLM(broken)
        with pytest.raises(ValueError):
            PhonotacticLM.from_counts(np.abs(broken))
    broken = table.copy()
    broken[2, 3] = -np.inf
    assert float(PhonotacticLM(broken).table[2, 3]) == -math.inf
    with pytest.raises(ValueError):
        PhonotacticLM(table[:, :5])
    with pytest.raises(ValueError):
        PhonotacticLM(np.zeros((2, 2), dtype=np.float32))
    # the decoders check the model against the emissions before any device work
    with pytest.raises(ValueError):
        E.BeamCTCDecoder(["<blank>", "a", "b"], 4, lm=lm)  # 6 classes against 3 tokens
    with pytest.raises(ValueError):
        E.BeamCTCDecoder(["<blank>", "a", "b", "c", "d", "e"], 4, lm=lm, lm_weight=float("nan"))
    assert E.BeamCTCDecoder(["<blank>", "a", "b", "c", "d", "e"], 4, lm=lm, lm_weight=0.5)._lm is lm
    with pytest.raises(RuntimeError):
        E.beam_ctc_decode(torch.zeros(1, 3, 6), torch.tensor([3]), 4, lm=lm)  # no CPU path


def test_binding_covers_the_beam_lm_header():
    from allophant_amd import lib

    header = open(os.path.join(ROOT, "include", "allophant_amx_beam_lm.h")).read()
    declared = re.findall(r"^int (amx_\w+)\(", header, re.M)
    assert declared == lib.BEAM_LM_EXPORTS
    assert int(re.search(r"#define AMX_BEAM_LM_MAX_CLASSES (\d+)", header).group(1)) == lib.BEAM_LM_MAX_CLASSES
    source = open(os.path.join(ROOT, "allophant_amd", "lib.py")).read()
    for name in declared:
        assert f"lib.{name}.argtypes" in source and f"lib.{name}.restype" in source
    so = os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)
    if os.path.exists(so):
        handle = lib.load()
        assert all(hasattr(handle, name) for name in declared)
    makefile = open(os.path.join(ROOT, "allophant_amd", "csrc", "Makefile")).read()
    assert "amx_ctc_beam_lm.hip" in makefile and "allophant_amx_beam_lm.h" in makefile


def test_c_abi_limits_without_a_device():
    """The limits are checked before any device work: AMX_EINVAL with a message."""
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    import ctypes as C

    h = lib.load()
    size = C.c_size_t()
    assert h.amx_beam_ctc_lm_workspace(16, 40, 499, C.byref(size)) == lib.AMX_OK
    assert size.value == 40 * 499 * 16 * 4
    assert h.amx_beam_ctc_lm_workspace(65, 1, 1, C.byref(size)) == lib.AMX_EINVAL
    null = None

    def call(Cn=3, n_lm=1, weight=1.0, bonus=0.0, beam=4, n_best=1, blank=0, flags=0):
        return h.amx_beam_ctc_lm_emissions(0, null, 0, 0, null, 1, 4, Cn, blank, beam, n_best, flags, null, n_lm, null, weight,
                                           bonus, null, 0, null, null, null, null, null, null)

    assert call(Cn=4096) == lib.AMX_EINVAL
    assert b"4095" in h.amx_last_error(None)
    assert call(Cn=1) == lib.AMX_EINVAL
    assert call(n_lm=0) == lib.AMX_EINVAL
    assert b"n_lm" in h.amx_last_error(None)
    for bad in (math.nan, math.inf, -math.inf):
        assert call(weight=bad) == lib.AMX_EINVAL
        assert b"finite" in h.amx_last_error(None)
        assert call(bonus=bad) == lib.AMX_EINVAL
    assert call(beam=4, n_best=5) == lib.AMX_EINVAL
    assert call(blank=3) == lib.AMX_EINVAL
    assert call(flags=2) == lib.AMX_EINVAL
    assert call() == lib.AMX_EINVAL  # null buffers
    assert b"null" in h.amx_last_error(None)
    assert call(Cn=4095) == lib.AMX_EINVAL and b"null" in h.amx_last_error(None)  # the largest class count passes the limits


def test_kernel_has_no_scratch_and_fits_the_lds(tmp_path):
    """amx_ctc_beam_lm.hip compiled for gfx950: one kernel with no scratch, no spilled VGPRs, no dynamic stack, and static
    LDS within the 160 KiB of a CU (hipcc's resource-usage report)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_beam_lm.hip")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                           "-o", str(tmp_path / "amx_ctc_beam_lm.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    report = done.stderr
    assert "beam_ctc_lm_kernel" in report
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", report)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", report)]
    assert len(scratch) == 1 and len(spills) == 1 and len(lds) == 1, report
    assert not any(scratch) and not any(spills), report
    assert "Dynamic Stack: True" not in report
    assert 0 < lds[0] <= 163840, report
