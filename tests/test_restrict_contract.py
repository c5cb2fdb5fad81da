"""Per-utterance inventories without a GPU: the C header against the binding and the built library with its host-side
refusals, the float64 restatement of the restriction (tests/restrict_util.py) against torch, LanguageInventories, and the
premise of predict_languages on the CPU oracle: the union pass restricted to a language is that language's own pass."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import restrict_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "restrict.c"
    src.write_text('#include "allophant_amx_restrict.h"\nint main(void) { return amx_restrict_outputs(0, 0, 0, 0, AMX_RESTRICT_MAX_CLASSES,'
                   ' 0, 0, 0, 1, 0, 0, AMX_RESTRICT_NORMALIZE, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_header_prototypes_are_the_exports():
    from allophant_amd import lib

    with open(os.path.join(ROOT, "include", "allophant_amx_restrict.h"), encoding="utf-8") as f:
        text = f.read()
    assert re.findall(r"^int (amx_\w+)\(", text, flags=re.M) == lib.RESTRICT_EXPORTS
    assert int(re.search(r"#define AMX_RESTRICT_NORMALIZE (\d+)u", text).group(1)) == lib.RESTRICT_NORMALIZE == U.NORMALIZE
    assert int(re.search(r"#define AMX_RESTRICT_MAX_CLASSES (\d+)", text).group(1)) == lib.RESTRICT_MAX_CLASSES == 65535
    prototype = re.search(r"^int amx_restrict_outputs\((.*?)\);", text, flags=re.M | re.S).group(1)
    assert len(prototype.split(",")) == 17


def test_exports_and_refusals():
    lib, handle = _library()
    for symbol in lib.RESTRICT_EXPORTS:
        assert hasattr(handle, symbol)
    assert len(handle.amx_restrict_outputs.argtypes) == 17

    def call(Cn=5, n_lang=2, N=2, T=8, flags=1, null=(), strides=None, out_strides=None):
        p = C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        arg = lambda name: None if name in null else p  # noqa: E731
        st, sn = strides or (N * Cn, Cn)
        ot, on = out_strides or (st, sn)
        return handle.amx_restrict_outputs(0, arg("src"), st, sn, Cn, arg("lengths"), arg("ids"), arg("bits"), n_lang, N, T, flags,
                                           arg("out"), ot, on, arg("status"), None)

    for Cn in (1, 0, -3, 65536):
        assert call(Cn=Cn) == lib.AMX_EINVAL, Cn
    assert b"classes" in handle.amx_last_error(None)
    assert call(n_lang=0) == lib.AMX_EINVAL and call(n_lang=-1) == lib.AMX_EINVAL
    assert call(flags=2) == lib.AMX_EINVAL and call(flags=3) == lib.AMX_EINVAL
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(strides=(-1, 5)) == lib.AMX_EINVAL and call(out_strides=(10, -5)) == lib.AMX_EINVAL
    for name in ("src", "lengths", "ids", "bits", "out", "status"):
        assert call(null=(name,)) == lib.AMX_EINVAL, name
    assert b"null" in handle.amx_last_error(None)
    assert call(N=2, T=2 ** 40, strides=(2 ** 40, 5)) == lib.AMX_EINVAL  # N * T
    assert call(N=2, T=2 ** 20, strides=(2 ** 50, 5)) == lib.AMX_EINVAL  # the extent of src
    assert call(N=2, T=2 ** 20, out_strides=(2 ** 50, 5)) == lib.AMX_EINVAL  # the extent of out
    # nothing to do: AMX_OK whatever the pointers are
    everything = ("src", "lengths", "ids", "bits", "out", "status")
    assert call(N=0, null=everything) == lib.AMX_OK and call(T=0, null=everything) == lib.AMX_OK
    assert call(N=0, Cn=1) == lib.AMX_EINVAL  # (the limits hold for an empty call as well)


def _pool(rng, T, N, Cn):
    return (rng.standard_normal((T, N, Cn)) * 8).astype(np.float32)


def test_restatement_equals_float64_log_softmax_of_the_gathered_columns():
    rng = np.random.default_rng(0)
    for Cn in (2, 63, 64, 65, 129, 300):
        T, N = 5, 4
        src = _pool(rng, T, N, Cn)
        members = [[0], list(range(Cn)), [0, Cn - 1], sorted(rng.choice(Cn, Cn // 2, replace=False).tolist())]
        lengths, ids = [5, 0, 3, 5], [3, 1, 2, 0]
        got, status = U.restrict(src, lengths, ids, members, U.NORMALIZE)
        raw, _ = U.restrict(src, lengths, ids, members, 0)
        assert status.tolist() == [0] * N
        for n in range(N):
            own = torch.tensor(members[ids[n]])
            rest = np.setdiff1d(np.arange(Cn), own.numpy())
            want = torch.log_softmax(torch.from_numpy(src[:lengths[n], n].astype(np.float64))[:, own], -1).numpy()
            assert np.abs(got[:lengths[n], n][:, own] - want).max(initial=0.0) < 1e-12
            assert np.array_equal(raw[:lengths[n], n][:, own], src[:lengths[n], n][:, own].astype(np.float64))
            for form in (got, raw):
                assert np.all(form[:lengths[n], n][:, rest] == -np.inf)
                assert np.all(form[lengths[n]:, n] == 0.0)


def test_restatement_gives_minus_inf_and_never_nan():
    src = np.zeros((3, 2, 6), dtype=np.float32)
    src[0, :, :] = -np.inf  # every member -inf
    src[1, :, 1] = -np.inf  # one member -inf
    src[2, :, 4] = 30.0  # a spike on a non-member
    for flags in (0, U.NORMALIZE):
        out, status = U.restrict(src, [3, 3], [0, 1], [[0, 1, 2], []], flags)
        assert not np.isnan(out).any() and status.tolist() == [0, 0]
        assert np.all(out[0] == -np.inf)
        assert np.all(out[:, 1] == -np.inf)  # a language without members
        assert out[1, 0, 1] == -np.inf and np.all(out[:, 0, 3:] == -np.inf)
        if flags:
            assert abs(out[1, 0, 0] + math.log(2)) < 1e-15 and abs(out[2, 0, 0] + math.log(3)) < 1e-15
    out, status = U.restrict(src, [3, 4], [2, 0], [[0]], U.NORMALIZE, out=np.full(src.shape, 7.0))
    assert status.tolist() == [-2, -2] and np.all(out == 7.0)


# -- LanguageInventories ----------------------------------------------------------------------------------------------
def _matrices():
    pool = torch.tensor([[0, 1], [1, 1], [2, 0], [0, 0], [1, 2]])
    return pool, {"x": pool[[0, 2, 3]], "y": pool[[3, 1]], "empty": pool[:0], "z": pool[[4]]}


def test_union_columns_and_bits_from_matrices():
    from allophant_amd.inventories import LanguageInventories

    pool, matrices = _matrices()
    inv = LanguageInventories.from_matrices(matrices)
    assert inv.languages == ["x", "y", "empty", "z"] and inv.union_symbols is None
    assert inv.union_tfi.tolist() == pool[[0, 2, 3, 1, 4]].tolist() and inv.classes == 6
    assert inv.columns("x").tolist() == [0, 1, 2, 3] and inv.columns("y").tolist() == [0, 3, 4]
    assert inv.columns("empty").tolist() == [0] and inv.columns(3).tolist() == [0, 5]
    for language, tfi in matrices.items():  # the round trip: the union's rows at a language's columns are its own matrix
        assert torch.equal(inv.union_tfi[inv.columns(language)[1:] - 1], tfi) and torch.equal(inv.tfi(language), tfi)
    assert inv.bits.dtype == np.uint64 and inv.bits.shape == (4, 1)
    for i, language in enumerate(inv.languages):
        assert [c for c in range(64) if int(inv.bits[i, 0]) >> c & 1] == inv.columns(language).tolist()
    assert np.array_equal(inv.bits, U.member_bits([inv.columns(l).tolist() for l in inv.languages], inv.classes))
    assert inv.language_ids(["z", "x", 1]).tolist() == [3, 0, 1] and inv.language_ids(torch.tensor([2, 0])).dtype == torch.int32
    with pytest.raises(ValueError):
        inv.index("q")
    with pytest.raises(IndexError):
        inv.language_ids(torch.tensor([4]))
    with pytest.raises(IndexError):
        inv.index(-1)
    with pytest.raises(ValueError):
        inv.symbols("x")


def test_bits_past_one_word():
    from allophant_amd.inventories import LanguageInventories

    pool = torch.stack([torch.arange(150) // 13, torch.arange(150) % 13], 1)
    inv = LanguageInventories.from_matrices({"all": pool, "some": pool[[0, 62, 63, 64, 127, 128, 149]]})
    assert inv.classes == 151 and inv.bits.shape == (2, 3)
    assert inv.columns("some").tolist() == [0, 1, 63, 64, 65, 128, 129, 150]
    assert np.array_equal(inv.bits, U.member_bits([inv.columns(l).tolist() for l in inv.languages], 151))
    assert int(inv.bits[0, 2]) == (1 << 23) - 1  # classes 128 .. 150


def test_index_spaces_are_inverses():
    from allophant_amd.inventories import LanguageInventories

    inv = LanguageInventories.from_matrices(_matrices()[1])
    for language in inv.languages:
        own = list(range(inv.columns(language).numel()))
        union = inv.from_language_indices(own, language)
        assert union == inv.columns(language).tolist() and inv.to_language_indices(union, language) == own
        assert torch.equal(inv.to_language_indices(torch.tensor(union), language), torch.tensor(own))
    assert inv.to_language_indices([4, 0, 3, 4], "y") == [2, 0, 1, 2] and inv.to_language_indices([], "y") == []
    for bad in ([1], [6], [-1]):
        with pytest.raises(ValueError):
            inv.to_language_indices(bad, "y")
    with pytest.raises(ValueError):
        inv.from_language_indices([3], "y")


def test_validation():
    from allophant_amd.inventories import LanguageInventories

    pool, matrices = _matrices()
    with pytest.raises(ValueError, match="twice"):
        LanguageInventories.from_matrices({"x": pool[[0, 1, 0]]})
    with pytest.raises(ValueError, match="features"):
        LanguageInventories.from_matrices({"x": pool, "y": torch.zeros(2, 3, dtype=torch.int64)})
    with pytest.raises(ValueError):
        LanguageInventories.from_matrices({})
    one = LanguageInventories.from_matrices({"only-blank": pool[:0], "one": pool[:1]})  # a one-class language is accepted
    assert one.columns("only-blank").tolist() == [0] and one.classes == 2 and int(one.bits[0, 0]) == 1


def test_from_table():
    import edit_util as E
    from allophant_amd.inventories import LanguageInventories
    from allophant_amd.phonetic import AttributeTable

    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    phonemes = table.phonemes
    assert len(phonemes) >= 4
    inventories = {"lg0": [phonemes[2], phonemes[0]], "lg1": [phonemes[0], phonemes[3], phonemes[1]], "lg2": []}
    inv = LanguageInventories.from_table(table, inventories)
    assert inv.union_symbols == [phonemes[2], phonemes[0], phonemes[3], phonemes[1]]
    assert torch.equal(inv.union_tfi, table.composition_feature_matrix(inv.union_symbols))
    for language, inventory in inventories.items():
        assert inv.symbols(language) == inventory
        assert torch.equal(inv.tfi(language), table.composition_feature_matrix(inventory))
    assert inv.columns("lg1").tolist() == [0, 2, 3, 4]
    with pytest.raises(ValueError, match="twice"):
        LanguageInventories.from_table(table, {"lg0": [phonemes[0], phonemes[0]]})
    with pytest.raises(ValueError):
        LanguageInventories.from_table(table, {"lg0": ["no such phoneme"]})


# -- the premise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_probabilities", [True, False])
def test_union_pass_restricted_is_the_language_pass_on_the_oracle(log_probabilities):
    """O.predict under the union, restricted by the restatement, against O.predict under each language's own matrix: valid
    frames within 1e-5 (fp32 oracle noise; 1.9e-6 measured), every other output bit-equal."""
    e = U.EndToEnd()
    inv = e.inventories
    assert e.pool.shape[0] == 61 and [inv.columns(l).numel() for l in "abc"] == [2, 8, 24]
    union, frames = e.oracle_union(log_probabilities)
    ids = inv.language_ids(e.LANGUAGES).tolist()
    members = [inv.columns(l).tolist() for l in inv.languages]
    restricted, status = U.restrict(union["phoneme"].numpy(), frames.tolist(), ids, members, U.NORMALIZE if log_probabilities else 0)
    assert status.tolist() == [0] * 6
    worst = 0.0
    for language in inv.languages:
        own, own_frames = e.oracle(language, log_probabilities)
        assert torch.equal(own_frames, frames)
        for name in own:
            if name != "phoneme":
                assert torch.equal(own[name], union[name]), name
        for n in (n for n, l in enumerate(e.LANGUAGES) if l == language):
            length = int(frames[n])
            got = restricted[:length, n][:, inv.columns(language).numpy()]
            worst = max(worst, float(np.abs(got - own["phoneme"][:length, n].double().numpy()).max()))
    print(f"union restricted vs per-language oracle: {worst:.3g}")
    assert worst < 1e-5
