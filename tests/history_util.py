"""Helpers of tests/test_gpu_history.py: the models and cases whose forward pass must give the same bits whatever the handle ran
before, the reference bits of a case, a handle with history, the walk over ordered pairs of cases, and the comparison.

A CASE is a batch plus the flags of ``Estimator.predict`` and the inventory; its ``pins`` are the entries of ``pass_info()`` that
make it the case it is meant to be.  A MODEL is a spec with synthetic weights, built by the helpers of the stage tests, and its
cases, the largest first.  Nothing here needs a GPU until a ``Handle`` is made.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from allophant_amd import synthetic
from tests import attn_adapter_util as AU, stage_util as SU

# finite in every type a workspace holds: fp16 65504 / 1.1, bf16 and (doubled) fp32 2.7e36 / 0.014, fp64 finite
PATTERNS = (0x7BFF, 0x3C66)
PLAN_KEYS = ("ln_fold", "packed", "attention", "rows")  # of ``pass_info()``: the plan may not depend on history either


@dataclasses.dataclass
class Case:
    name: str
    audio: Tensor
    lengths: Tensor
    pins: Dict[str, int] = dataclasses.field(default_factory=dict)
    flags: Dict[str, bool] = dataclasses.field(default_factory=dict)  # _no_pack / _keep_hidden
    log_probabilities: bool = True
    inventory: str = "default"


@dataclasses.dataclass
class Model:
    name: str
    spec: Dict[str, Any]
    state: Dict[str, Tensor]
    inventories: Dict[str, Optional[Tensor]]
    cases: List[Case]  # the first one is the largest: a veteran runs it first, so that no later case grows a workspace

    def case(self, name: str) -> Case:
        return next(c for c in self.cases if c.name == name)


def shaved(audio: Tensor, lengths: Tensor, by: List[int]) -> Tuple[Tensor, Tensor]:
    """the batch with utterance i shortened by ``by[i]`` samples (zeros behind its end, the padded length kept)"""
    lengths = lengths - torch.tensor(by)
    audio = audio * (torch.arange(audio.shape[1]).unsqueeze(0) < lengths.unsqueeze(1))
    return audio, lengths


def _xlsr() -> Model:
    from tests.test_gpu_parity import _custom_ragged
    from tests.test_gpu_stage_local import xlsr_model

    spec, state, tfi = xlsr_model()
    mid = synthetic.make_audio(4, 160000, seed=55)
    pk1 = shaved(synthetic.make_audio(3, 48000, seed=1234)[0], torch.tensor([48000, 48000, 48000]), [0, 16000, 28800])
    pk2 = _custom_ragged(6, 8.0, seed=77)
    longkeys = shaved(*synthetic.make_audio(6, 320000, seed=61), [0, 0, 0, 0, 0, 9000])
    cases = [
        Case("fold", *synthetic.make_audio(16, 160000, seed=778), {"ln_fold": 1, "packed": 0}),
        Case("mid", *mid, {"packed": 0, "attention": 2}),
        Case("mid_shaved", *shaved(*mid, [0, 8000, 2000, 10000]), {"packed": 0, "attention": 2, "rows": 4 * 499}),
        Case("short", *synthetic.make_audio(2, 48000, seed=1234, ragged=True)),
        Case("one", *synthetic.make_audio(1, 48000, seed=3)),
        Case("pk1", *pk1, {"packed": 1, "rows": 149 + 99 + 59}),
        Case("pk2", *pk2, {"packed": 2}),
        Case("fold_pk", *synthetic.make_audio(16, 160000, seed=4000, ragged=True), {"ln_fold": 1, "packed": 2, "rows": 6631}),
        Case("longkeys", *longkeys, {"attention": 3}),
        Case("pk2/no_pack", *pk2, {"packed": 0}, {"_no_pack": True}),
        Case("pk2/keep", *pk2, {"packed": 0}, {"_keep_hidden": True}),
        Case("mid/raw", *mid, {"packed": 0, "attention": 2}, log_probabilities=False),
        Case("mid/inv200", *mid, {"packed": 0, "attention": 2}, inventory="inv200"),
    ]
    return Model("xlsr", spec, state, {"default": tfi, "inv200": synthetic.make_inventory(spec, 200, seed=3)}, cases)


def _four_cases(equal, ragged, one) -> List[Case]:
    """what every model but the XLS-R one gets: equal lengths, ragged enough to pack, the same under ``_no_pack``, one utterance"""
    return [Case("equal", *equal, {"packed": 0}), Case("ragged", *ragged), Case("ragged/no_pack", *ragged, {"packed": 0}, {"_no_pack": True}),
            Case("one", *one, {"packed": 0})]


def _post_ln() -> Model:
    from tests.test_gpu_parity import _custom_ragged

    spec = SU.post_ln_tapped_spec()
    cases = _four_cases(synthetic.make_audio(8, 96000, seed=82), _custom_ragged(8, 6.0, seed=82), synthetic.make_audio(1, 48000, seed=3))
    cases[1].pins = {"packed": 2}
    return Model("post_ln", spec, synthetic.make_state_dict(spec, seed=23), {"default": synthetic.make_inventory(spec, 11, seed=23)}, cases)


def _heads() -> Model:
    spec = SU.heads_case_spec(True)
    cases = _four_cases(synthetic.make_audio(3, 32000, seed=41), synthetic.make_audio(3, 32000, seed=41, ragged=True),
                        synthetic.make_audio(1, 32000, seed=42))
    cases[1].pins = {"packed": 1}  # (a time-layer head keeps the rows from being packed early)
    return Model("heads", spec, synthetic.make_state_dict(spec, seed=21), {"default": synthetic.make_inventory(spec, 9, seed=5)}, cases)


def _small(name: str, spec, state, tfi, hidden: int) -> Model:
    """the tiny head-dimension models on the batch of tests/test_gpu_stage_widths.py (``head_dim_batch``)"""
    cases = _four_cases(synthetic.make_audio(5, 24000, seed=hidden), synthetic.make_audio(5, 24000, seed=hidden, ragged=True),
                        synthetic.make_audio(1, 24000, seed=hidden + 1))
    cases[1].pins = {"packed": 1}
    return Model(name, spec, state, {"default": tfi}, cases)


_BUILDERS = {
    "xlsr": _xlsr,
    "post_ln": _post_ln,
    "heads": _heads,
    "dh40": lambda: _small("dh40", *SU.head_dim_model(80, 2, 2), 80),      # rows of 64 columns, 24 of them padding
    "dh96": lambda: _small("dh96", *SU.head_dim_model(192, 2, 4), 192),    # rows of 128 columns, 32 of them padding
    "adapter": lambda: _small("adapter", *AU.small_model(80, 2, 2, 16), 80),
}
# (model, precision) of every parametrised test
RUNS = [("xlsr", "f16x3"), ("xlsr", "bf16x3"), ("xlsr", "f16"), ("xlsr", "bf16"), ("post_ln", "f16x3"), ("heads", "f16x3"),
        ("dh40", "f16x3"), ("dh96", "f16x3"), ("adapter", "f16x3")]
_models: Dict[str, Model] = {}


def model(name: str) -> Model:
    if name not in _models:
        _models[name] = _BUILDERS[name]()
    return _models[name]


def pair_walk(n: int) -> List[int]:
    """A closed walk over 0 .. n - 1 that takes every ordered pair of distinct vertices exactly once as neighbours: an Euler
    circuit of the complete directed graph (Hierholzer, out-edges in ascending order), n (n - 1) + 1 vertices long."""
    unused = {v: [w for w in range(n) if w != v] for v in range(n)}
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop(0))
        else:
            walk.append(stack.pop())
    return walk[::-1]


@dataclasses.dataclass
class Result:
    """what a pass left: the whole flat output buffer, the frame lengths and the plan, on the host"""
    flat: Tensor
    lengths: Tensor
    info: Dict[str, int]
    blocks: List[Tuple[str, int, Tuple[int, int, int]]]  # (output, offset into ``flat``, (T, N, classes))


_device_batches: Dict[Tuple[str, str], Any] = {}


class Handle:
    """An ``Estimator`` of ``model`` with one device output buffer per case: a recording is keyed on the audio and output
    addresses, so every pass of a case reads the same device batch and writes the same buffer, poisoned with NaN in front of
    the pass -- a pass has to write every element of it, the zeros of the frames beyond ``lengths`` included."""

    def __init__(self, amd, mdl: Model, precision: str):
        self.amd, self.model = amd, mdl
        self.est = amd.Estimator(mdl.spec, mdl.state, "cuda:0", precision)
        self._out: Dict[str, Tensor] = {}

    def close(self) -> None:
        self.est.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def run(self, case: Case, eager: bool) -> Result:
        key = (self.model.name, case.name)
        if key not in _device_batches:
            n = case.audio.shape[0]
            _device_batches[key] = self.amd.Batch(case.audio.cuda(), case.lengths, torch.zeros(n, dtype=torch.long))
        batch = _device_batches[key]
        tfi = self.model.inventories[case.inventory]
        if case.name not in self._out:
            self.est._select_inventory(tfi)
            total = self.est._output_layout(*case.audio.shape)[2]
            self._out[case.name] = torch.empty(total, dtype=torch.float32, device="cuda")
        out = self._out[case.name]
        out.fill_(float("nan"))
        pred = self.est.predict(batch, tfi, case.log_probabilities, _no_graph=eager, _out=out, **case.flags)
        info = self.est.pass_info()
        blocks = [(k, v.storage_offset() - pred._flat.storage_offset(), tuple(v.shape)) for k, v in pred.outputs.items()]
        return Result(pred._flat.cpu(), pred.lengths.cpu(), info, blocks)  # (the copy waits for the pass)

    def scribble(self, word16: int) -> None:
        self.est._debug_scribble(word16)


def first_difference(got: Result, want: Result) -> str:
    """where two flat buffers first differ: (output, utterance, frame, class), whether the frame is valid, and both values"""
    for name, offset, (T, N, classes) in want.blocks:
        g = got.flat[offset: offset + T * N * classes].view(T, N, classes)
        w = want.flat[offset: offset + T * N * classes].view(T, N, classes)
        # utterance-major, as the message reads (NaN != NaN: a poisoned element that was never written counts)
        differs = (g != w).permute(1, 0, 2).nonzero()
        if len(differs):
            n, t, c = differs[0].tolist()
            where = "valid" if t < int(want.lengths[n]) else "padding"
            return (f"output {name!r}, utterance {n}, frame {t} ({where}: {int(want.lengths[n])} valid frames), class {c}: "
                    f"{g[t, n, c].item()!r} != {w[t, n, c].item()!r}; {len(differs)} elements of this output differ")
    return "no element differs"


def assert_same(got: Result, want: Result, what: str) -> None:
    """no tolerance: the whole flat buffer, the frame lengths and the plan"""
    assert torch.equal(got.lengths, want.lengths), f"{what}: frame lengths {got.lengths.tolist()} != {want.lengths.tolist()}"
    plan_got, plan_want = ({k: r.info[k] for k in PLAN_KEYS} for r in (got, want))
    assert plan_got == plan_want, f"{what}: the plan depends on the history: {plan_got} != {plan_want}"
    assert got.flat.shape == want.flat.shape, f"{what}: {got.flat.shape} != {want.flat.shape}"
    if not torch.equal(got.flat, want.flat):
        raise AssertionError(f"{what}: {first_difference(got, want)}")


_references: Dict[Tuple[str, str, str], Result] = {}


def reference(amd, mdl: Model, precision: str, case: Case) -> Result:
    """The bits of a clean pass of ``case``: a new handle runs it once (which allocates), its workspaces are filled with zeros
    over their whole allocation, and it runs again -- the second pass is the reference, and the first one must equal it (else the
    pass depends on what the allocator handed out).  Asserts the case's pins.  Cached for the module's lifetime, on the host."""
    key = (mdl.name, precision, case.name)
    if key not in _references:
        with Handle(amd, mdl, precision) as fresh:
            first = fresh.run(case, eager=True)
            fresh.est.check_finite()
            fresh.scribble(0)
            second = fresh.run(case, eager=True)
            fresh.est.check_finite()
        what = f"{mdl.name}/{precision} case {case.name!r}"
        print(f"[history] {what}: pass_info {second.info}")
        for pin, value in case.pins.items():
            assert second.info[pin] == value, f"{what} is not the case it is meant to be: {pin} = {second.info[pin]}, not {value}"
        assert not torch.isnan(second.flat).any(), f"{what}: a clean pass left elements of the output buffer unwritten"
        assert_same(first, second, f"{what}, first pass of a fresh handle against the pass on zeroed workspaces")
        _references[key] = second
    return _references[key]
