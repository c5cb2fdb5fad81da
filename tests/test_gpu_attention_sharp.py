"""The attention kernels under a peaked softmax, in every launch form.

Every other parity test draws its q / k projections with std ``1 / sqrt(D)``: logits of about 1 nat, a nearly uniform softmax, and
the deferred maximum of ``amx_attention.hip`` (after a query's first key tile the running maximum, the running sum and the output
accumulators are rescaled only when a tile exceeds the maximum by more than 2^8) never rescales -- nor does the merge of the two
key halves (``KS = 2``) ever see two different maxima.  Here the q projection of every layer is multiplied by 8 and by 16
(``attention_util.sharpen``): |scores| of 40 .. 140 log2 units, probabilities up to 256 in the hi / lo planes of P, accumulators
that start at ``-m_run`` in the hundreds, key halves that dominate one another by 2^50.  Each case

  * asserts through ``attention_util.rescale_rows`` that its inputs reach the rescale (layer 0: at least 2 % of the (utterance, head,
    query) rows at factor 8, 10 % at 16) before anything is launched,
  * asserts the attention form it is about through ``pass_info()["attention"]`` (on a device whose CU count routes the batch
    otherwise that fails, and is not adapted to),
  * compares hidden states 1 and 2 (the final LayerNorm's) with the fp64 evaluation of the CPU oracle and the log-probs with the
    fp32 oracle, every utterance evaluated alone, at the project's gate of 1e-3 on valid frames.  ``test_attention_util.py`` keeps
    the fp32 oracle within 1e-4 of fp64 on every case; a rescale fault mis-weights a query by 2^8 at least.

Precision f16x3 (the default and timed mode), two layers.  Measured on an MI355X (256 CUs), worst |error| on valid frames -- hidden
states against fp64, log-probs against the fp32 oracle -- next to the fp32 oracle's own distance from fp64 and the share of rows
that fire at layer 0:

    case               factor  form  hidden    log-probs  oracle    rows firing
    w4                 8       1     9.3e-06   2.6e-05    8.0e-06   11.0 %
    w4                 16      1     2.4e-05   3.5e-05    2.2e-05   35.6 %
    key_split          8       2     1.2e-05   2.8e-05    1.2e-05   12.0 %
    key_split          16      2     4.2e-05   5.3e-05    4.6e-05   42.9 %
    key_split_no_mask  8       2     1.2e-05   2.9e-05    1.3e-05   6.9 %
    key_split_no_mask  16      2     4.2e-05   5.2e-05    4.4e-05   24.6 %
    w8                 8       0     1.1e-05   2.9e-05    1.5e-05   21.4 %
    w8                 16      0     2.3e-05   7.2e-05    2.4e-05   52.1 %
    long_key           8       3     1.2e-05   3.5e-05    1.6e-05   58.5 %
    long_key           16      3     2.5e-05   9.7e-05    3.4e-05   84.5 %
    head_dim_32        8       4     6.9e-06   2.0e-05    6.6e-06   6.7 %
    head_dim_32        16      4     1.7e-05   6.2e-05    2.4e-05   27.1 %
    head_dim_80        8       5     4.7e-06   1.6e-05    6.2e-06   2.5 %
    head_dim_80        16      5     1.2e-05   3.8e-05    1.2e-05   25.1 %
    head_dim_96        8       5     1.9e-05   7.3e-05    2.6e-05   11.8 %
    head_dim_96        16      5     5.1e-05   1.4e-04    7.4e-05   34.3 %
    head_dim_120       8       5     9.1e-06   1.9e-05    1.1e-05   10.3 %
    head_dim_120       16      5     2.3e-05   5.4e-05    2.7e-05   32.2 %

Invariance (``attention_util.shift_keys``: +-8 added to every element of every k bias, on the factor-16 weights; every score of a
query moves by the same ``q . b``, the function does not change, the scores of layer 0 reach 588 / 810 log2 units; 8 is the largest
power of two at which the fp32 oracle stays within 1e-4 of fp64 -- 5.5e-5 / 3.9e-5; at 16: 1.1e-4):

    key_split          16      2     3.6e-05   1.5e-04    6.6e-05   42.9 %   (19 % of the rows start below -128 log2 units)
    long_key           16      3     3.8e-05   1.1e-04    4.3e-05   84.5 %   (17 %)

This case found a fault: a query whose FIRST tile has a maximum below -128 log2 units was re-based with ``alpha = 2^-d`` = infinity
on accumulators that are still zero -- NaN, and one layer on every frame of the batch (``check_finite`` reported all of them).  Both
kernels now keep alpha at 1 or below; every other result is the same bit for bit.

Without ``l_run *= alpha`` in ``attn_kernel`` all 16 w4, key_split, w8 and head_dim cases fail and the long_key ones pass; without
it in ``attn2_kernel`` the two long_key cases fail and the other 16 pass (checked once on scratch builds)."""
import pytest
import torch

import attention_util as A
from golden_util import max_abs_valid_tm

pytestmark = pytest.mark.gpu
CASE_FACTORS = [(case.name, factor) for case in A.CASES for factor in case.factors]


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _batch(amd, ref):
    return amd.Batch(ref.audio.cuda(), ref.lengths, torch.zeros(len(ref.lengths), dtype=torch.long))


def _logprob_error(pred, ref):
    assert torch.equal(pred.lengths.cpu(), ref.frames)
    assert list(pred.outputs) == list(ref.logprobs)
    return max(max_abs_valid_tm(pred.outputs[k].cpu(), ref.logprobs[k], ref.frames) for k in ref.logprobs)


def _check(amd, case, ref, label):
    """The batch of ``ref`` through a fresh Estimator: the debug capture (padded rows) against the fp64 hidden states and the
    fp32 log-probs, then a plain call (packed rows for a ragged batch) and one that keeps the padded layout."""
    layers = ref.spec["layers"]
    est = amd.Estimator(ref.spec, ref.state, "cuda:0", "f16x3")
    batch = _batch(amd, ref)
    pred = est.predict(batch, ref.tfi, True, _keep_hidden=True)
    est.check_finite()
    info = est.pass_info()
    assert info["attention"] == case.form and info["packed"] == 0, info
    worst_logprob = _logprob_error(pred, ref)
    worst_hidden = max(A.valid_max(est.debug_fetch("hidden", i), ref.hidden64[i], ref.frames) for i in range(1, layers + 1))
    layouts = []
    for no_pack in (False, True):
        pred = est.predict(batch, ref.tfi, True, _no_pack=no_pack)
        est.check_finite()
        info = est.pass_info()
        assert info["attention"] == case.form, info
        assert info["packed"] == 0 if no_pack else (info["packed"] > 0 or not case.packs), info
        layouts.append(info["packed"])
        worst_logprob = max(worst_logprob, _logprob_error(pred, ref))
    est.close()
    print(f"\n    {label:18s} form {case.form}  hidden {worst_hidden:.1e}  log-probs {worst_logprob:.1e}  oracle {ref.oracle_noise:.1e}  "
          f"rows firing {100 * ref.fired / ref.rows:.1f} %  max |score| {ref.top_score:.0f}  packed {layouts[0]}")
    assert worst_hidden < A.GATE, (label, worst_hidden)
    assert worst_logprob < A.GATE, (label, worst_logprob)


@pytest.mark.parametrize("name,factor", CASE_FACTORS)
def test_sharpened_attention_against_fp64(amd, name, factor):
    case = A.CASE[name]
    ref = A.reference(name, factor)
    assert ref.fired >= (0.02 if factor == case.factors[0] else 0.10) * ref.rows, (ref.fired, ref.rows)
    assert ref.oracle_noise < A.NOISE_BOUND
    _check(amd, case, ref, f"{name} x{factor}")


@pytest.mark.parametrize("name", A.SHIFT_CASES)
def test_key_shift_invariance(amd, name):
    """A constant vector on every k bias: the reference function is the one of the unshifted weights (test_attention_util.py), the
    raw scores are five times larger.  Same gate, against the fp64 evaluation of the same weights."""
    case = A.CASE[name]
    ref = A.reference(name, A.SHIFT_FACTOR, A.SHIFT)
    assert ref.fired >= 0.10 * ref.rows and ref.sunk >= 0.02 * ref.rows and ref.oracle_noise < A.NOISE_BOUND
    _check(amd, case, ref, f"{name} shift {A.SHIFT:g}")


def test_factor_one_is_the_unsharpened_model(amd):
    """Guards the helper: ``sharpen(state, spec, 1)`` in one Estimator, the checkpoint as generated in another -- equal bit for bit."""
    from allophant_amd import synthetic

    case = A.CASE["key_split"]
    ref = A.reference("key_split", 1)
    plain = synthetic.make_state_dict(ref.spec, seed=case.seed)
    flats = []
    for state in (ref.state, plain):
        est = amd.Estimator(ref.spec, state, "cuda:0", "f16x3")
        pred = est.predict(_batch(amd, ref), ref.tfi, True)
        est.check_finite()
        assert est.pass_info()["attention"] == case.form
        flats.append({k: v.cpu().clone() for k, v in pred.outputs.items()})
        est.close()
    assert all(torch.equal(flats[0][k], flats[1][k]) for k in flats[0])


def test_key_split_is_deterministic(amd):
    """Two runs of the key-split case (factor 16, packed rows): equal bit for bit -- the merge of the halves has one order."""
    case = A.CASE["key_split"]
    ref = A.reference("key_split", 16)
    est = amd.Estimator(ref.spec, ref.state, "cuda:0", "f16x3")
    runs = []
    for _ in range(2):
        pred = est.predict(_batch(amd, ref), ref.tfi, True, _no_graph=True)
        est.check_finite()
        assert est.pass_info()["attention"] == case.form
        runs.append({k: v.cpu().clone() for k, v in pred.outputs.items()})
    est.close()
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
