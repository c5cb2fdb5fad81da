"""The sinc resampling contract on the host (no GPU): the float64 restatement (tests/resample_util.py) against upstream's
length rule, the identity, the frequency response and the impulse response; the library's host-side bank builder against
the restatement, its limits, the ctypes binding, the Python surface's argument checks, and a kernel compiled without scratch
or spills."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import resample_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_VOICE = (8000, 16000, 24000, 32000, 44100, 48000)  # mozilla_common_voice.py upstream
UCLA = (44100, 48000)  # ucla_phonetic_corpus.py upstream
RATES = sorted(set(COMMON_VOICE + UCLA + (11025, 22050)))


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib.load()


@pytest.mark.parametrize("rate", RATES)
def test_output_lengths_follow_upstreams_rule(rate):
    """len' = ceil(m * len / o) equals upstream's ceil(16000 * n / source_rate) (speech_corpus.py) and the restatement's
    output length, and the binding's helper agrees."""
    from allophant_amd.resample import output_length

    rng = np.random.default_rng(rate)
    ns = list(range(0, 3000)) + [int(v) for v in rng.integers(3000, 48000 * 120, size=400)]
    for n in ns:
        expected = math.ceil(16000 * n / rate)
        assert R.output_length(n, rate, 16000) == expected == output_length(n, rate, 16000), (rate, n)
    for n in (0, 1, 5, 441, 1000, 4411):
        assert len(R.resample_row(np.ones(n), rate, 16000)) == R.output_length(n, rate, 16000)


@pytest.mark.parametrize("rates", [(16000, 16000), (44100, 44100), (32000, 32000)])
def test_identity_returns_the_input(rates):
    x = np.random.default_rng(0).standard_normal(1234)
    assert R.bank(*rates) is None
    assert np.array_equal(R.resample_row(x, *rates), x)


def _amplitude(y: np.ndarray, f: float, rate: int) -> float:
    """Least-squares amplitude of the tone f in y, away from the edges."""
    t = np.arange(len(y)) / rate
    basis = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)[2000:-2000]
    coef, *_ = np.linalg.lstsq(basis, y[2000:-2000], rcond=None)
    return float(np.hypot(*coef))


@pytest.mark.parametrize("rate", [r for r in RATES if r != 16000])
def test_passband_tone_keeps_its_amplitude(rate):
    """1 kHz, well inside the passband of every rate: amplitude within 1e-3 after resampling to 16 kHz."""
    t = np.arange(rate) / rate
    y = R.resample_row(np.sin(2 * np.pi * 1000.0 * t), rate, 16000)
    assert abs(_amplitude(y, 1000.0, 16000) - 1.0) <= 1e-3


@pytest.mark.parametrize("rate", [32000, 44100, 48000])
def test_tone_above_the_new_nyquist_is_attenuated(rate):
    """The default filter (lpw 6, rolloff 0.99): a 12 kHz tone comes out below 2e-3 (-54 dB), a 14 kHz tone below 1e-4
    (-80 dB).  (Their aliases would sit at 4 and 2 kHz.)"""
    t = np.arange(rate) / rate
    for f, bound in ((12000.0, 2e-3), (14000.0, 1e-4)):
        y = R.resample_row(np.sin(2 * np.pi * f * t), rate, 16000)
        assert np.abs(y[2000:-2000]).max() < bound, (rate, f)


@pytest.mark.parametrize("rates", [(44100, 16000), (48000, 16000), (8000, 16000), (16000, 44100)])
def test_impulse_reproduces_the_bank(rates):
    """x = delta at p: y[f m + j] = h_j[p + W - f o] (0 where that tap does not exist)."""
    o, m, W, h, _ = R.bank(*rates)
    n, p = 40 * o + 7, 17 * o + 3
    x = np.zeros(n)
    x[p] = 1.0
    y = R.resample_row(x, *rates)
    expected = np.zeros_like(y)
    for t in range(len(y)):
        f, j = divmod(t, m)
        i = p + W - f * o
        if 0 <= i < h.shape[1]:
            expected[t] = h[j, i]
    assert np.array_equal(y, expected)


BUILDER_CASES = [(r, 16000, 6, 0.99) for r in RATES if r != 16000] + [
    (16000, 8000, 6, 0.99), (16000, 44100, 6, 0.99), (16000, 22050, 6, 0.99), (44100, 16000, 3, 0.9),
    (48000, 16000, 16, 0.95), (22050, 16000, 6, 1.0), (96000, 16000, 6, 0.99), (1, 2, 1, 0.5)]


@pytest.mark.parametrize("orig,new,lpw,rolloff", BUILDER_CASES)
def test_host_bank_builder_matches_the_restatement(orig, new, lpw, rolloff):
    """amx_resample_bank (called through ctypes, no device): same o, m, W, tap ranges, and every kept tap is the
    restatement's float64 value rounded to fp32 (within one fp32 ulp: the host libm may differ in the last float64 bit);
    every dropped tap is below 1e-30 in the restatement."""
    _library()
    from allophant_amd.resample import host_bank

    o, m, W, h, raw = R.bank(orig, new, lpw, rolloff)
    geometry, bank, phases = host_bank(orig, new, lpw, rolloff)
    first, count = R.tap_ranges(raw, lpw)
    assert (geometry.o, geometry.m, geometry.width) == (o, m, W)
    assert geometry.taps == count.max() and geometry.bank_size == geometry.taps * m
    assert np.array_equal(phases[0].numpy(), first) and np.array_equal(phases[1].numpy(), count)
    assert geometry.window == (1023 // m + 1) * o + int(first[-1]) + geometry.taps - int(first[0])
    bank = bank.numpy().astype(np.float64)
    for j in range(m):
        kept = h[j, first[j]: first[j] + count[j]]
        np.testing.assert_allclose(bank[: count[j], j], kept.astype(np.float32), rtol=2 ** -23, atol=1e-45)
        assert not bank[count[j]:, j].any()
        dropped = np.concatenate([h[j, : first[j]], h[j, first[j] + count[j]:]])
        assert np.abs(dropped).max(initial=0.0) < 1e-30


def test_host_bank_of_the_identity_is_empty():
    _library()
    from allophant_amd.resample import host_bank

    geometry, bank, phases = host_bank(48000, 48000)
    assert (geometry.o, geometry.m, geometry.width, geometry.taps, geometry.bank_size, geometry.window) == (1, 1, 0, 0, 0, 0)
    assert bank.numel() == 0 and phases.numel() == 0


@pytest.mark.parametrize("orig,new,lpw,rolloff,message", [
    (0, 16000, 6, 0.99, b"sample rates"), (-44100, 16000, 6, 0.99, b"sample rates"), (44100, 0, 6, 0.99, b"sample rates"),
    (2 ** 31, 16000, 6, 0.99, b"sample rates"), (44100, 16000, 0, 0.99, b"lowpass_filter_width"),
    (44100, 16000, 1025, 0.99, b"lowpass_filter_width"), (44100, 16000, 6, 0.0, b"rolloff"), (44100, 16000, 6, 1.5, b"rolloff"),
    (44100, 16000, 6, float("nan"), b"rolloff"), (16000, 16001, 6, 0.99, b"reduced target rate"),
    (256000, 16000, 6, 0.99, b"window"), (44100, 16000, 6, 1e-9, b"window"), (2 ** 31 - 1, 1, 6, 0.99, b"window")])
def test_host_bank_builder_rejects_inputs_outside_its_limits(orig, new, lpw, rolloff, message):
    import ctypes as C

    from allophant_amd import lib

    h = _library()
    geometry = lib.AmxResampleGeometry()
    assert h.amx_resample_bank(orig, new, lpw, rolloff, C.byref(geometry), None, None) == lib.AMX_EINVAL
    assert message in h.amx_last_error(None)
    assert h.amx_resample_bank(44100, 16000, 6, 0.99, None, None, None) == lib.AMX_EINVAL
    assert h.amx_resample_bank(192000, 16000, 6, 0.99, C.byref(geometry), None, None) == lib.AMX_OK  # the largest ratio listed


def test_device_entry_checks_its_arguments_without_a_device():
    from allophant_amd import lib

    h = _library()
    null = None

    def call(stride=8, L_in=8, window=64, N=2, L_out=4, x=1):
        return h.amx_resample(0, x, stride, L_in, null, null, null, null, window, N, L_out, null, null)

    assert call(N=-1) == lib.AMX_EINVAL
    assert call(N=65536) == lib.AMX_EINVAL
    assert call(L_out=(1 << 40) + 1) == lib.AMX_EINVAL
    assert call(window=lib.RESAMPLE_MAX_WINDOW + 1) == lib.AMX_EINVAL
    assert call(stride=4) == lib.AMX_EINVAL
    assert call() == lib.AMX_EINVAL and b"null" in h.amx_last_error(None)
    assert call(N=0) == lib.AMX_OK and call(L_out=0) == lib.AMX_OK  # nothing to do: no device touched


def test_binding_covers_the_resample_header():
    from allophant_amd import lib

    header = open(os.path.join(ROOT, "include", "allophant_amx_resample.h")).read()
    declared = re.findall(r"^int (amx_\w+)\(", header, re.M)
    assert sorted(declared) == sorted(lib.RESAMPLE_EXPORTS)
    assert int(re.search(r"#define AMX_RESAMPLE_MAX_PHASES (\d+)", header).group(1)) == lib.RESAMPLE_MAX_PHASES
    assert int(re.search(r"#define AMX_RESAMPLE_MAX_WINDOW (\d+)", header).group(1)) == lib.RESAMPLE_MAX_WINDOW

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\}" % name, header, re.S).group(1)
        return re.findall(r"\w+", re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("int64_t", ""))

    assert fields("amx_resample_geometry") == [f for f, _ in lib.AmxResampleGeometry._fields_]
    assert fields("amx_resample_row") == list(lib.RESAMPLE_ROW_FIELDS)
    source = open(os.path.join(ROOT, "allophant_amd", "lib.py")).read()
    for name in declared:
        assert f"lib.{name}.argtypes" in source and f"lib.{name}.restype" in source
    so = os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)
    if os.path.exists(so):
        handle = lib.load()
        assert all(hasattr(handle, name) for name in declared)


def test_python_surface_argument_checks():
    """No CPU path: CPU tensors and other dtypes raise; only sinc_interp_hann exists; the estimator's rate is 16 kHz."""
    _library()
    from allophant_amd import resample as RS
    from allophant_amd.estimator import SAMPLE_RATE, Batch, Estimator

    x = torch.zeros(2, 100)
    with pytest.raises(RuntimeError, match="no CPU"):
        RS.resample(x, 44100, 16000)
    with pytest.raises(ValueError, match="sinc_interp_hann"):
        RS.resample(x, 44100, 16000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError, match="sinc_interp_hann"):
        RS.Resample(44100, 16000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError, match="positive"):
        RS.resample(x, 0, 16000)
    module = RS.Resample(44100, 16000)
    assert module.bank.numel() == 160 * module._geometry.taps and module.phases.numel() == 2 * 160
    assert not module.state_dict()  # non-persistent buffers, like upstream's kernel
    with pytest.raises(RuntimeError, match="no CPU"):
        module(x)
    with pytest.raises(RuntimeError, match="no CPU"):
        RS.resample_batch(Batch(x, torch.tensor([100, 50]), torch.zeros(2, dtype=torch.long)), 44100)
    assert SAMPLE_RATE == 16000 and isinstance(Estimator.sample_rate, property)
    assert callable(Estimator.resample)


def test_kernel_has_no_scratch_and_no_spills(tmp_path):
    """amx_resample.hip compiled for gfx950 (device ISA, -S): a private segment of 0 bytes and no spilled VGPRs."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "amx_resample.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(ROOT, "allophant_amd", "csrc", "amx_resample.hip")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    assert "resample_kernel" in isa
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] and spills == [0], isa[-3000:]


def test_restatement_against_torchaudio():
    """Only where torchaudio can be imported (it is not a dependency): torchaudio's own resampler on float64 input against
    the restatement, within 1e-5."""
    torchaudio = pytest.importorskip("torchaudio")
    rng = np.random.default_rng(5)
    for rate in (8000, 22050, 44100, 48000):
        x = rng.standard_normal(rate // 3)
        ours = R.resample_row(x, rate, 16000)
        theirs = torchaudio.functional.resample(torch.from_numpy(x), rate, 16000).numpy()
        assert ours.shape == theirs.shape
        assert np.abs(ours - theirs).max() <= 1e-5
