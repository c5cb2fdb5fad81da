"""The allophone layer's structure and arithmetic on the host (no GPU): the structure ``allophant_amd.allophones`` builds from a
``LanguageAllophoneMappings`` dump against the REAL reference's ``AllophoneMapping`` buffers, and a NumPy restatement of
``map_allophones`` against the reference's outputs (tests/golden/g17_allophone_mapping.npz, tools/gen_allophone_golden.py).
The GPU kernel is held to the same restatement in test_gpu_allophones.py."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from allophant_amd.allophones import build_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G17 = os.path.join(ROOT, "tests", "golden", "g17_allophone_mapping.npz")
FINFO_MIN = np.finfo(np.float32).min


def map_allophones_np(x, matrices, mask, ids):
    """``AllophoneMapping.map_allophones`` (acoustic_model.py:142-159) in NumPy: per utterance the dense product, masked
    positions set to finfo(float32).min after the multiply, NaN-propagating max over the phones."""
    x = np.asarray(x, dtype=np.float32)
    T, N, _ = x.shape
    n_lang = matrices.shape[0]
    out = np.empty((T, N, matrices.shape[2]), dtype=np.float32)
    for n, v in enumerate(ids):
        lang = int(v)
        assert -n_lang <= lang < n_lang
        with np.errstate(invalid="ignore", over="ignore"):
            product = x[:, n, :, None] * matrices[lang][None]
        product[:, mask[lang]] = FINFO_MIN
        out[:, n] = product.max(axis=1)
    return out


@pytest.fixture(scope="module")
def g17():
    return np.load(G17)


def _mapping(g17, int_keys):
    dump = json.loads(bytes(g17["mapping_json"]).decode())
    if int_keys:
        dump["allophones"] = {int(k): {int(q): v for q, v in m.items()} for k, m in dump["allophones"].items()}
    return dump


@pytest.mark.parametrize("int_keys", [True, False])
def test_structure_is_the_references(g17, int_keys):
    mapping = _mapping(g17, int_keys)
    if int_keys:
        assert list(mapping["allophones"]) == g17["mapping_int_order"].tolist()  # keys out of order, like the generator's dict
    L, P1, Q1 = g17["matrices"].shape
    structure = build_structure(mapping, P1, Q1)
    assert structure.mask.dtype == torch.bool and structure.initialization.dtype == torch.float32
    assert np.array_equal(structure.mask.numpy(), g17["mask"])
    assert np.array_equal(structure.initialization.numpy().view(np.uint32), g17["initialization"].view(np.uint32))
    assert structure.index_map == json.loads(bytes(g17["index_map_json"]).decode())
    # matrices follow the dict's order (languages 2, 0, 3); the fourth, of the language without an entry, is masked everywhere,
    # blank included
    assert structure.index_map == {"deu": 0, "spa": 1, "fin": 2}
    assert structure.mask[3].all() and not structure.mask[:3, 0, 0].any()


def test_structure_accepts_an_object_with_attributes(g17):
    from types import SimpleNamespace

    mapping = _mapping(g17, True)
    L, P1, Q1 = g17["matrices"].shape
    structure = build_structure(SimpleNamespace(**mapping), P1, Q1)
    assert np.array_equal(structure.mask.numpy(), g17["mask"])


@pytest.mark.parametrize("change, message", [
    (lambda m: m["allophones"]["0"].update({"17": [1]}), "phoneme index"),
    (lambda m: m["allophones"]["0"].update({"-1": [1]}), "phoneme index"),
    (lambda m: m["allophones"]["0"].update({"3": [23]}), "shared phone index"),
    (lambda m: m["allophones"]["0"].update({"3": [-1]}), "shared phone index"),
    (lambda m: m["allophones"]["0"].update({"3": "ab"}), "list of shared phone indices"),
    (lambda m: m["allophones"]["0"].update({"x": [1]}), "phoneme index"),
    (lambda m: m["allophones"].update({"4": {}}), "language index"),
    (lambda m: m.update(languages=["spa", "ita"]), "maps 3 languages"),
    (lambda m: m["allophones"].update({"1": [1, 2]}), "must map phonemes"),
    (lambda m: m.pop("allophones"), "lacks 'allophones'"),
    (lambda m: m.update(allophones=[1, 2]), "must map language indices"),
])
def test_malformed_mappings_raise(g17, change, message):
    mapping = _mapping(g17, False)
    change(mapping)
    L, P1, Q1 = g17["matrices"].shape
    with pytest.raises(ValueError, match=re.escape(message)):
        build_structure(mapping, P1, Q1)


@pytest.mark.parametrize("which", ["", "_float"])
def test_numpy_restatement_reproduces_the_reference(g17, which):
    expected = g17["outputs" + which]
    got = map_allophones_np(g17["inputs"], g17["matrices"], g17["mask"], g17["ids" + which].tolist())
    assert np.array_equal(np.isnan(got), np.isnan(expected))
    assert np.isnan(expected).any() and (expected == FINFO_MIN).any()
    assert np.array_equal(got[~np.isnan(got)].view(np.uint32), expected[~np.isnan(expected)].view(np.uint32))


def test_end_to_end_case_maps_its_phone_outputs(g17):
    """The tiny-model case: the reference's mapped outputs are the restatement of its own phone log-probabilities."""
    got = map_allophones_np(g17["e2e/phone"], g17["matrices"], g17["mask"], g17["e2e/ids"].tolist())
    assert np.array_equal(got.view(np.uint32), g17["e2e/mapped"].view(np.uint32))


def test_kernel_has_no_scratch_or_spills(tmp_path):
    """amx_allophone.hip compiled for gfx950: no scratch, no spilled registers (hipcc's resource-usage report)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "allophant_amd", "csrc", "amx_allophone.hip")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                           "-o", str(tmp_path / "amx_allophone.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    report = done.stderr
    assert "allophone_map_kernel" in report
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)]
    spills = [int(v) for v in re.findall(r"[SV]GPRs Spill: (\d+)", report)]
    assert scratch and spills, report
    assert not any(scratch) and not any(spills), report
    assert "Dynamic Stack: False" in report
