"""Long recordings without a GPU: the C header against the binding and the built library, amx_long_plan against the NumPy
restatement of the plan (tests/longform_util.py) and against the properties that make the stitched output a partition of the
recording's frames, its refusals, and the frame <-> sample mapping the plan rests on, on the CPU oracle's feature encoder."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import longform_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2V2 = ([10, 3, 3, 3, 3, 2, 2], [5, 2, 2, 2, 2, 2, 2])  # S = 320, RF = 400
SMALL = ([3, 2], [2, 3])                                # S = 6, RF = 5


def _library():
    from allophant_amd import lib

    return lib, lib.load()


def _plan(lengths, window, context, stack=W2V2, capacity=None, sizing=False, want_frames=True):
    """One raw amx_long_plan call: (code, n_windows, windows [capacity, 6] or None, frames or None)."""
    lib, handle = _library()
    kernels, strides = stack
    values = (C.c_int64 * max(1, len(lengths)))(*lengths)
    count = C.c_int64(-7)
    frames = (C.c_int64 * max(1, len(lengths)))(*([-7] * max(1, len(lengths))))
    k, s = (C.c_int32 * len(kernels))(*kernels), (C.c_int32 * len(strides))(*strides)
    windows = None
    if not sizing:
        if capacity is None:
            capacity = len(U.plan(lengths, window, context, kernels, strides)[0])
        windows = np.full((capacity + 1, 6), -7, dtype=np.int32)  # one guard row
    code = handle.amx_long_plan(values, len(lengths), window, context, k, s, len(kernels),
                                None if windows is None else C.c_void_p(windows.ctypes.data), capacity or 0, C.byref(count),
                                frames if want_frames else None)
    return code, count.value, windows, list(frames)[:len(lengths)]


def test_header_compiles_as_c99_and_declares_the_exports(tmp_path):
    lib, handle = _library()
    with open(os.path.join(ROOT, "include", "allophant_amx_long.h"), encoding="utf-8") as f:
        text = f.read()
    assert re.findall(r"^int (amx_\w+)\(", text, flags=re.M) == lib.LONG_EXPORTS
    assert int(re.search(r"#define AMX_LONG_MAX_BLOCKS (\d+)", text).group(1)) == lib.LONG_MAX_BLOCKS == 64
    fields = re.search(r"typedef struct amx_long_window \{ int32_t (.*?); \}", text).group(1)
    assert tuple(f.strip() for f in fields.split(",")) == lib.LONG_WINDOW_FIELDS
    for name, count in (("amx_long_plan", 11), ("amx_long_gather", 12), ("amx_long_stitch", 12)):
        prototype = re.search(rf"^int {name}\((.*?)\);", text, flags=re.M | re.S).group(1)
        assert len(prototype.split(",")) == count == len(getattr(handle, name).argtypes), name
    assert C.sizeof(lib.AmxLongBlock) == 24
    for symbol in lib.LONG_EXPORTS:
        assert hasattr(handle, symbol), symbol
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "long.c"
    src.write_text('#include "allophant_amx_long.h"\n'
                   "int main(void) {\n"
                   "    int64_t lengths[1] = {0}, n = 0, frames[1];\n"
                   "    int32_t k[1] = {1}, s[1] = {1};\n"
                   "    amx_long_window w[1];\n"
                   "    amx_long_block b = {0, 0, AMX_LONG_MAX_BLOCKS};\n"
                   "    return amx_long_plan(lengths, 1, 1, 0, k, s, 1, w, 1, &n, frames) + (int)b.classes + (int)sizeof w;\n"
                   "}\n")
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_closed_form_frames_equal_the_per_layer_formula():
    from allophant_amd import spec as S

    assert U.constants(*W2V2) == (320, 400) and U.constants(*SMALL) == (6, 5)
    tiny = S.tiny_encoder()
    assert U.constants(tiny["conv_kernel"], tiny["conv_stride"]) == (320, 400)
    for stack in (W2V2, SMALL, ([1], [1]), ([4, 4, 1], [3, 1, 2])):
        for L in range(0, 3000):
            assert U.frames(L, *stack) == U.nested_frames(L, *stack), (stack, L)
    for L in (399, 400, 719, 720, 160000, 57600000):
        assert U.frames(L, *W2V2) == U.nested_frames(L, *W2V2)
        if L >= 400:
            assert S.frame_lengths([L], tiny) == [U.frames(L, *W2V2)]


@pytest.mark.parametrize("stack", [W2V2, SMALL], ids=["wav2vec2", "k32s23"])
def test_plan_equals_the_restatement(stack):
    S, RF = U.constants(*stack)
    windows = (400, 720, 799, 4000, 160000) if stack is W2V2 else (5, 11, 16, 17, 100)
    compared = 0
    for window in windows:
        Wf = U.frames(window, *stack)
        for c in sorted({0, 1, (Wf - 1) // 2}):
            K = Wf - 2 * c
            if K < 1:
                continue
            counts = sorted({0, 1, Wf - 1, Wf, Wf + 1, Wf + K - 1, Wf + K, Wf + K + 1, 5 * K + 3} - {-1})
            singles = [[RF - 1], [RF]] + [[U.length_for(T, *stack, extra=extra)] for T in counts if T >= 1 for extra in (0, S - 1)]
            triples = [[U.length_for(5 * K + 3, *stack, 7 % S), RF - 1, U.length_for(Wf + 1, *stack)],
                       [0, U.length_for(Wf, *stack), U.length_for(Wf + K + 1, *stack, S - 1)]]
            for lengths in singles + triples:
                want, want_frames = U.plan(lengths, window, c, *stack)
                code, n, got, frames = _plan(lengths, window, c, stack)
                assert code == 0 and n == len(want) and frames == want_frames.tolist(), (window, c, lengths)
                assert np.array_equal(got[:n], want), (window, c, lengths)
                assert (got[n:] == -7).all()
                compared += 1
            assert [U.frames(l[0], *stack) for l in singles[2::2]] == [T for T in counts if T >= 1]
    assert compared > 100


def test_plan_properties_on_random_draws():
    """2 000 seeded draws: window sizes from 400 to 160 000 samples, every admissible context, lengths up to 14 windows."""
    from allophant_amd import longform, spec as S

    rng = np.random.default_rng(20)
    spec = S.tiny_encoder()
    hop, RF = 320, 400
    several = 0
    for draw in range(2000):
        window = int(rng.choice([400, 401, 719, 720, 1039, 1040, int(rng.integers(400, 8000)), int(rng.integers(400, 160001))]))
        Wf = U.frames(window, *W2V2)
        c = int(rng.integers(0, (Wf - 1) // 2 + 1))
        K = Wf - 2 * c
        lengths = [int(rng.integers(0, 14 * window)) for _ in range(int(rng.integers(1, 4)))]
        if draw % 5 == 0:
            lengths[0] = U.length_for(int(rng.integers(1, 6 * Wf)), *W2V2, extra=int(rng.integers(0, hop)))
        plan = longform.plan_windows(lengths, spec, window, c)
        assert (plan.window, plan.context, plan.hop) == (window, c, hop) and plan.windows.dtype == np.int32
        want, want_frames = U.plan(lengths, window, c, *W2V2)
        assert np.array_equal(plan.windows, want) and np.array_equal(plan.frames, want_frames)
        assert plan.windows[:, U.RECORDING].tolist() == sorted(plan.windows[:, U.RECORDING].tolist())
        for r, length in enumerate(lengths):
            T = U.frames(length, *W2V2)
            rows = plan.windows[plan.windows[:, U.RECORDING] == r]
            n = len(rows)
            assert rows[:, U.INDEX].tolist() == list(range(n)) and (n == 0) == (T == 0)
            several += n > 2
            at = 0
            for i, (_, _, a, lo, hi, samples) in enumerate(rows.tolist()):
                assert lo == at and hi > lo, "the kept ranges partition [0, T)"
                at = hi
                assert a <= lo and hi <= a + U.frames(samples, *W2V2)
                assert samples >= RF and a * hop + samples <= length
                if i < n - 1:
                    assert samples == window
                elif n > 1:
                    assert window - hop < samples <= window
                if i > 0:      # an inner seam: c frames of context on both sides of it
                    previous = rows[i - 1]
                    assert lo - a >= c and previous[U.START] + U.frames(int(previous[U.SAMPLES]), *W2V2) - lo >= c
            assert at == T
    assert several > 500


def test_refusals_and_the_sizing_call():
    lib, handle = _library()
    ok = dict(lengths=[9000, 250, 4000], window=4000, context=2)
    want, want_frames = U.plan(ok["lengths"], 4000, 2, *W2V2)
    # windows == NULL only sizes the plan
    code, n, _, frames = _plan(**ok, sizing=True)
    assert (code, n, frames) == (0, len(want), want_frames.tolist()) and n == 4
    assert _plan(**ok, sizing=True, want_frames=False)[:2] == (0, 4)
    # too little room: refused, the size still reported, nothing written
    code, n, windows, frames = _plan(**ok, capacity=3)
    assert code == lib.AMX_EINVAL and n == 4 and (windows == -7).all() and frames == want_frames.tolist()
    assert b"room" in handle.amx_last_error(None)
    assert _plan(**ok, capacity=7)[:2] == (0, 4)
    refused = [dict(ok, window=399), dict(ok, context=6), dict(ok, context=-1), dict(ok, lengths=[9000, -1]),
               dict(ok, stack=([], [])), dict(ok, stack=([3] * 9, [2] * 9)), dict(ok, stack=([10, 0], [5, 2])),
               dict(ok, stack=([10, 3], [5, 0])), dict(ok, stack=([10, 3], [-5, 2])),
               dict(lengths=[400 + 320 * (2 ** 31 - 1)], window=4000, context=2),   # 2^31 frames
               dict(lengths=[4000], window=2 ** 40, context=2)]
    for case in refused:
        code, n, _, _ = _plan(**case, capacity=8)
        assert code == lib.AMX_EINVAL and n == 0, case
    largest = [400 + 320 * (2 ** 31 - 2)]  # 2^31 - 1 frames, in the largest window
    assert _plan(largest, 2 ** 31 - 1, 0, sizing=True)[:2] == (0, len(U.plan(largest, 2 ** 31 - 1, 0, *W2V2)[0]))
    assert _plan(ok["lengths"], 4000, 5)[0] == 0 and _plan(ok["lengths"], 400, 0)[0] == 0  # K = 2; a window of one frame
    assert _plan([], 4000, 2)[:2] == (0, 0)
    # null pointers
    k, s = (C.c_int32 * 7)(*W2V2[0]), (C.c_int32 * 7)(*W2V2[1])
    one, count = (C.c_int64 * 1)(9000), C.c_int64(-7)
    assert handle.amx_long_plan(one, 1, 4000, 2, k, s, 7, None, 0, None, None) == lib.AMX_EINVAL
    assert handle.amx_long_plan(None, 1, 4000, 2, k, s, 7, None, 0, C.byref(count), None) == lib.AMX_EINVAL and count.value == 0
    assert handle.amx_long_plan(one, 1, 4000, 2, None, s, 7, None, 0, C.byref(count), None) == lib.AMX_EINVAL
    assert handle.amx_long_plan(one, -1, 4000, 2, k, s, 7, None, 0, C.byref(count), None) == lib.AMX_EINVAL
    # the Python binding raises ValueError with the library's reason
    from allophant_amd import longform, spec as S

    with pytest.raises(ValueError, match="receptive field"):
        longform.plan_windows([9000], S.tiny_encoder(), 399, 0)
    with pytest.raises(ValueError, match="keeps none"):
        longform.plan_windows([9000], S.tiny_encoder(), 4000, 6)
    # the launches refuse on the host before any device work (never-dereferenced pointers)
    p = C.c_void_p(64)
    gather = lambda n=2, R=1, stride=100, hop=320, L_out=50, audio=p: handle.amx_long_gather(  # noqa: E731
        0, audio, stride, p, R, p, n, hop, L_out, p, p, None)
    assert gather(n=-1) == gather(R=-1) == gather(stride=-1) == gather(L_out=-1) == lib.AMX_EINVAL
    assert gather(hop=0) == gather(hop=2 ** 31) == gather(audio=None) == lib.AMX_EINVAL
    assert gather(R=2 ** 31 - 1, stride=2 ** 62) == lib.AMX_EINVAL and gather(n=0, audio=None) == lib.AMX_OK
    block = lambda *v: (lib.AmxLongBlock * 1)(lib.AmxLongBlock(*v))  # noqa: E731
    stitch = lambda n=2, src_T=12, blocks=block(0, 0, 5), n_blocks=1, R=1, dst_T=30, src=p: handle.amx_long_stitch(  # noqa: E731
        0, src, src_T, n, p, blocks, n_blocks, p, R, dst_T, p, None)
    assert stitch(n=-1) == stitch(src_T=-1) == stitch(R=-1) == stitch(dst_T=-1) == stitch(n_blocks=-1) == lib.AMX_EINVAL
    assert stitch(blocks=block(0, 0, 0)) == stitch(blocks=block(-4, 0, 5)) == stitch(blocks=block(0, -4, 5)) == lib.AMX_EINVAL
    assert stitch(blocks=None) == stitch(src=None) == stitch(src_T=2 ** 29) == lib.AMX_EINVAL  # (2^29 * 5 classes)
    many = (lib.AmxLongBlock * 65)(*[lib.AmxLongBlock(0, 0, 5)] * 65)
    assert stitch(blocks=many, n_blocks=65) == lib.AMX_EINVAL and b"at most 64" in handle.amx_last_error(None)
    assert stitch(n=0, src=None) == stitch(n_blocks=0, blocks=None, src=None) == lib.AMX_OK


def test_a_window_sees_the_frames_of_the_recording_at_its_start():
    """The premise of the plan, on the CPU oracle's conv stack (tiny encoder, no normalisation): the features of each planned
    window of a 9 000-sample row are the row's features at start + j.  Gate 1e-4: fp32 convolutions of other lengths differ
    by 1.7e-6 here (measured), features one frame apart by 2.95."""
    from allophant_amd import spec as S, synthetic
    from oracle import allophant_oracle as O

    encoder = S.tiny_encoder(2)
    encoder["do_normalize"] = False
    spec = S.baseline_spec(encoder, 5)
    state = synthetic.make_state_dict(spec, seed=4)
    audio, _ = synthetic.make_audio(1, 9000, seed=8)
    windows, frames = U.plan([9000], 4000, 2, spec["conv_kernel"], spec["conv_stride"])
    assert frames.tolist() == [27] and len(windows) == 3 and windows[-1].tolist() == [0, 2, 15, 18, 27, 4000]
    with torch.inference_mode():
        whole = O.feature_encoder(audio, state, spec)[0]
        assert whole.shape[0] == 27
        worst, shifted = 0.0, 0.0
        for _, _, a, lo, hi, samples in windows.tolist():
            own = O.feature_encoder(audio[:, a * 320: a * 320 + samples], state, spec)[0]
            assert own.shape[0] >= hi - a
            worst = max(worst, float((own[lo - a: hi - a] - whole[lo:hi]).abs().max()))
            shifted = max(shifted, float((own[lo - a: hi - a - 1] - whole[lo + 1: hi]).abs().max()))
    print(f"window features vs the recording's: {worst:.3g} aligned, {shifted:.3g} one frame off")
    assert worst < 1e-4 < 0.5 < shifted
