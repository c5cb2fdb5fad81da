"""The stage-local method of tests/stage_util.py checked on the CPU, before tests/test_gpu_stage_local.py relies on it.

Three things per stage (conv, front, each encoder layer, heads), from the oracle's own intermediates:

* the restated stage reproduces the oracle's next intermediate to fp32 rounding (``FP32_ROUNDING``);
* the split-product emulation on fp16 planes errs against the float64 truth by at most ``EMU_OVER_FP32`` x what plain fp32 does;
* the separation condition: with ONE cross term dropped from ONE product, the stage errs by at least ``SEPARATION`` x the intact
  emulation's error ``e_emu``.  The GPU gate is 3 x e_emu, so every such loss lands >= 2.5 x above it.  A product that does not
  reach the condition is listed in ``NOT_DETECTABLE`` with its measured ratio -- the condition itself is not lowered.
  For XLS-R width the encoder layers are also taken the way a pass with the LayerNorm fold runs them (``layerN/fold``).

Cases: XLS-R width (hidden 1024, 16 heads, FFN 4096, two layers, 2 x 3 s ragged), a tiny post-LN / group-norm model, and the tiny
hierarchical model with time-layer heads that the GPU heads case runs.  For tests/test_gpu_stage_widths.py: the XLS-R 1B and 2B
widths (``xlsr_1b``, ``xlsr_2b``: hidden 1280 / 1920, heads of 80 / 120 columns, built like the XLS-R case) and the tiny models with
head dimensions 40, 8, 96 and 128 (``dh40`` ...: ``stage_util.HEAD_DIM_MODELS``, 5 ragged utterances of <= 1.5 s).  A (case, mode,
stage) whose weakest lost term is below 5.0 x e_emu -- ``LISTED_FLOOR`` plus 10 % for the summation order of the BLAS -- is not
claimed, here or on the GPU: ``stage_util.NOT_CLAIMED``.  For tests/test_gpu_stage_heads.py: the heads models of ``stage_util``
(``narrow_wide`` ... ``time_layers/dh160``), the heads stage alone, once per inventory, on the batch of ``stage_util.heads_audio``.

The same three things for the two combined stages that tests/test_gpu_stage_production.py judges a pass without the keep flag by:
``entry`` (audio -> hidden[0]) on the XLS-R and the tiny post-LN case, ``tail`` (last layer + heads of a post-LN encoder) at
wav2vec2-base width on the model of that file's post-LN case (``post_ln_base``: 3 x 3 s ragged, that stage only).
"""
import pytest
import torch

from allophant_amd import spec as S, synthetic
from tests import stage_util as SU

# Two fp32 evaluations of one stage differ by the rounding of sums of up to K = 8192 products of O(1) terms in another order:
# about sqrt(K) * 2^-24 = 5e-6 on values of rms ~1; four times that, relative to the largest value of the stage's output where
# that is beyond 1 (composed logits reach tens).
FP32_ROUNDING = 2e-5
EMU_OVER_FP32 = 8.0
SEPARATION = 7.5

# (case, mode, stage, product, dropped term) -> measured ratio (dropped error / e_emu) of a product whose lost cross term does NOT
# reach 7.5 x e_emu of its stage ("not detectable at stage level" with the full margin; DESIGN.md, "Stage-local error budget").
# The ``xlsr`` ones sit in the second layer under the LayerNorm fold on bf16 planes: there the emulation carries the fold's rounding of
# the stream to 16 bits about the pivot, which triples e_emu (1.2e-5 -> 3.7e-5) while a lost cross term costs what it did.  They
# still land at >= 2 x the GPU gate of 3 x e_emu; LISTED_FLOOR holds them above it.  The two entries at 7.5 / 7.6 are within
# rounding of the condition and are listed so that the outcome does not hang on the summation order of the host's BLAS.
NOT_DETECTABLE = {
    ("xlsr", "bf16x3", "layer1/fold", "q_proj", "lo_x"): 6.4,
    ("xlsr", "bf16x3", "layer1/fold", "q_proj", "lo_w"): 7.5,
    ("xlsr", "bf16x3", "layer1/fold", "k_proj", "lo_w"): 7.4,
    ("xlsr", "bf16x3", "layer1/fold", "qk", "lo_x"): 7.6,
    # the combined stage ``tail`` (last post-LN layer + heads, wav2vec2-base width): its e_emu is that of the heads (8e-6 on fp16
    # planes, of which the layer alone has 1.5e-6), so the attention-score products of the layer, the weakest of every layer, come
    # out lower than in a layer judged alone.  Only ``q_proj`` / ``k_proj`` / ``qk`` may be listed for a combined stage; the
    # entries at 7.7 / 7.8 are again within rounding of the condition.
    ("post_ln_base", "f16x3", "tail", "q_proj", "lo_w"): 6.9,
    ("post_ln_base", "bf16x3", "tail", "qk", "lo_x"): 6.4,
    ("post_ln_base", "bf16x3", "tail", "q_proj", "lo_x"): 7.8,
    ("post_ln_base", "bf16x3", "tail", "q_proj", "lo_w"): 7.7,
    ("post_ln_base", "bf16x3", "tail", "k_proj", "lo_x"): 7.7,
    # XLS-R 1B / 2B width (hidden 1280 / 1920, heads of 80 / 120 columns).  With K = 1280 / 1920 and an FFN of 5120 / 7680, e_emu
    # of a layer on fp16 planes is 4.2e-6 ... 6.0e-6 (hidden 1024: 2.2e-6 ... 3.0e-6) while a cross term lost from a score product
    # costs about what it did, so the attention-score products of the layers -- again only ``q_proj`` / ``k_proj`` / ``qk`` --
    # come out at 6.0 ... 7.9 instead of 8.9 and up.  On bf16 planes the unfolded layers are at >= 20; the first folded one is at
    # 6.0 ... 7.7, and the second folded one is not claimed at all (``stage_util.NOT_CLAIMED``).  Entries from 7.5 to 7.9 are
    # within rounding of the condition and are listed for the same reason as the two above.
    ("xlsr_1b", "f16x3", "layer0", "k_proj", "lo_w"): 7.6,
    ("xlsr_1b", "f16x3", "layer0/fold", "k_proj", "lo_w"): 7.8,
    ("xlsr_1b", "f16x3", "layer1", "q_proj", "lo_x"): 7.1,
    ("xlsr_1b", "f16x3", "layer1", "q_proj", "lo_w"): 7.0,
    ("xlsr_1b", "f16x3", "layer1", "k_proj", "lo_x"): 7.7,
    ("xlsr_1b", "f16x3", "layer1", "k_proj", "lo_w"): 6.5,
    ("xlsr_1b", "f16x3", "layer1", "qk", "lo_x"): 7.6,
    ("xlsr_1b", "f16x3", "layer1/fold", "q_proj", "lo_x"): 7.3,
    ("xlsr_1b", "f16x3", "layer1/fold", "q_proj", "lo_w"): 7.1,
    ("xlsr_1b", "f16x3", "layer1/fold", "k_proj", "lo_x"): 7.9,
    ("xlsr_1b", "f16x3", "layer1/fold", "k_proj", "lo_w"): 6.6,
    ("xlsr_1b", "f16x3", "layer1/fold", "qk", "lo_x"): 7.7,
    ("xlsr_1b", "bf16x3", "layer0/fold", "q_proj", "lo_x"): 7.0,
    ("xlsr_1b", "bf16x3", "layer0/fold", "q_proj", "lo_w"): 6.1,
    ("xlsr_1b", "bf16x3", "layer0/fold", "k_proj", "lo_w"): 6.7,
    ("xlsr_1b", "bf16x3", "layer0/fold", "qk", "lo_x"): 7.7,
    ("xlsr_1b", "bf16x3", "layer0/fold", "qk", "lo_w"): 7.6,
    ("xlsr_2b", "f16x3", "layer0", "q_proj", "lo_w"): 7.5,
    ("xlsr_2b", "f16x3", "layer0", "qk", "lo_x"): 7.2,
    ("xlsr_2b", "f16x3", "layer0/fold", "q_proj", "lo_w"): 7.5,
    ("xlsr_2b", "f16x3", "layer0/fold", "k_proj", "lo_x"): 7.9,
    ("xlsr_2b", "f16x3", "layer0/fold", "qk", "lo_x"): 7.1,
    ("xlsr_2b", "f16x3", "layer1", "q_proj", "lo_x"): 7.0,
    ("xlsr_2b", "f16x3", "layer1", "q_proj", "lo_w"): 6.5,
    ("xlsr_2b", "f16x3", "layer1", "k_proj", "lo_x"): 7.9,
    ("xlsr_2b", "f16x3", "layer1", "k_proj", "lo_w"): 6.2,
    ("xlsr_2b", "f16x3", "layer1", "qk", "lo_x"): 6.8,
    ("xlsr_2b", "f16x3", "layer1", "qk", "lo_w"): 7.3,
    ("xlsr_2b", "f16x3", "layer1/fold", "q_proj", "lo_x"): 6.8,
    ("xlsr_2b", "f16x3", "layer1/fold", "q_proj", "lo_w"): 6.3,
    ("xlsr_2b", "f16x3", "layer1/fold", "k_proj", "lo_x"): 7.6,
    ("xlsr_2b", "f16x3", "layer1/fold", "k_proj", "lo_w"): 6.0,
    ("xlsr_2b", "f16x3", "layer1/fold", "qk", "lo_x"): 6.8,
    ("xlsr_2b", "f16x3", "layer1/fold", "qk", "lo_w"): 7.1,
    ("xlsr_2b", "bf16x3", "layer0/fold", "q_proj", "lo_x"): 6.0,
    ("xlsr_2b", "bf16x3", "layer0/fold", "q_proj", "lo_w"): 6.2,
    ("xlsr_2b", "bf16x3", "layer0/fold", "k_proj", "lo_x"): 6.8,
    ("xlsr_2b", "bf16x3", "layer0/fold", "k_proj", "lo_w"): 6.5,
    ("xlsr_2b", "bf16x3", "layer0/fold", "qk", "lo_x"): 7.2,
    ("xlsr_2b", "bf16x3", "layer0/fold", "qk", "lo_w"): 7.4,
}
LISTABLE_IN_COMBINED = ("q_proj", "k_proj", "qk")
LISTED_FLOOR = 4.5  # 1.5 x the GPU gate's factor: a listed product's lost term is still caught there


def xlsr_case():
    enc = S.xlsr_300m_encoder()
    enc["layers"] = 2
    spec = S.multitask_spec(enc, ["syllabic", "long"], allophone_layer=True)
    spec["shared_phones"] = 80
    audio, lengths = synthetic.make_audio(2, 48000, seed=1234, ragged=True)
    return spec, synthetic.make_state_dict(spec, seed=0), synthetic.make_inventory(spec, 27, seed=0), audio, lengths


def post_ln_case():
    enc = S.tiny_encoder(2)
    enc.update(feat_extract_norm="group", conv_bias=False, stable_layer_norm=False, use_attention_mask=False)
    spec = S.multitask_spec(enc, ["syllabic", "long"], embedding_size=48, train_phonemes=12, n_features=6)
    audio, lengths = synthetic.make_audio(3, 16000, seed=99, ragged=True)
    return spec, synthetic.make_state_dict(spec, seed=11), synthetic.make_inventory(spec, 9, seed=11), audio, lengths


def heads_case():
    spec = SU.heads_case_spec(True)
    audio, lengths = synthetic.make_audio(3, 32000, seed=41, ragged=True)
    return spec, synthetic.make_state_dict(spec, seed=21), synthetic.make_inventory(spec, 9, seed=5), audio, lengths


def post_ln_base_case():
    """wav2vec2-base width, post-LN, masked, the spec of the post-LN case of tests/test_gpu_stage_production.py: the ``tail`` only"""
    spec = SU.post_ln_tapped_spec()
    audio, lengths = synthetic.make_audio(3, 48000, seed=82, ragged=True)
    return spec, synthetic.make_state_dict(spec, seed=23), synthetic.make_inventory(spec, 11, seed=23), audio, lengths


def width_case(encoder):
    """``xlsr_case`` at another released width: the encoder's own hidden / heads / FFN / positional groups on two layers"""
    enc = dict(encoder, layers=2)
    spec = S.multitask_spec(enc, ["syllabic", "long"], allophone_layer=True)
    spec["shared_phones"] = 80
    audio, lengths = synthetic.make_audio(2, 48000, seed=1234, ragged=True)
    return spec, synthetic.make_state_dict(spec, seed=0), synthetic.make_inventory(spec, 27, seed=0), audio, lengths


def head_dim_case(hidden, heads, groups):
    return lambda: SU.head_dim_model(hidden, heads, groups) + synthetic.make_audio(5, 24000, seed=hidden, ragged=True)


class Recipe:
    """a case: how it is built and which stages it gets beyond conv / front / layers / heads.  ``fold``: every layer also the way
    a pass with the LayerNorm fold runs it; ``entry``: audio -> hidden[0] in one; ``tail_only``: that combined stage alone;
    ``heads_only``: a heads model (``build`` gives (spec, state, inventories)): the heads stage alone, once per inventory"""

    def __init__(self, build, fold=False, entry=False, tail_only=False, heads_only=False):
        self.build, self.fold, self.entry, self.tail_only, self.heads_only = build, fold, entry, tail_only, heads_only


CASES = {"xlsr": Recipe(xlsr_case, fold=True, entry=True), "post_ln": Recipe(post_ln_case, entry=True), "heads": Recipe(heads_case),
         "post_ln_base": Recipe(post_ln_base_case, tail_only=True),
         "xlsr_1b": Recipe(lambda: width_case(S.xlsr_1b_encoder()), fold=True, entry=True),
         "xlsr_2b": Recipe(lambda: width_case(S.xlsr_2b_encoder()), fold=True, entry=True),
         **{f"dh{hidden // heads}": Recipe(head_dim_case(hidden, heads, groups)) for hidden, heads, groups in SU.HEAD_DIM_MODELS}}

# The heads models of tests/test_gpu_stage_heads.py, the heads stage alone (once per inventory).  The heads are judged jointly, as
# a maximum over outputs, so an output with a large e_emu could hide a lost term of a quiet one.  The candidate was
# ``large_inventory`` (the 1026-class log-softmax over the 640-wide composition, e_emu 2.5e-5 / 2.5e-4, next to 4-class heads): its
# weakest term, lo(W) of ``syllabic.linear`` on bf16 planes, still lands at 30 x e_emu, so no model had to be split.
HEADS_AUDIO_SEED = 97
CASES.update({name: Recipe(build, heads_only=True) for name, build in SU.HEADS_MODELS.items()})


def _named(logits, logp, transpose=False):
    """the two results of the heads as one dictionary (``transpose``: the oracle's time-major tensors)"""
    return {**{"logits:" + k: v.transpose(0, 1) if transpose else v for k, v in logits.items()},
            **{"logp:" + k: v.transpose(0, 1) if transpose else v for k, v in logp.items()}}


class Stage:
    """one stage with a fixed input: ``run(ev)`` evaluates it, ``want`` is the oracle's own next intermediate"""

    def __init__(self, name, run, want, frames):
        self.name, self.run, self.want, self.frames = name, run, want, frames

    def run_dropped(self, mode, drop):
        return self.run(SU.Evaluation(mode, drop))


class ConvStage(Stage):
    """the conv stack: a cross term dropped in layer i changes nothing below it, so the intact emulation's output of layer
    i - 1 is computed once per mode and the evaluation restarts there"""

    def __init__(self, x, state, spec, want, frames):
        super().__init__("conv", lambda ev: SU.conv_stage(x, state, spec, ev), want, frames)
        self.x, self.state, self.spec, self.prefix = x, state, spec, {}

    def run_dropped(self, mode, drop):
        layer = int(drop[0][len("conv"):])
        if mode not in self.prefix:
            outs, h = {}, self.x
            for i in range(len(self.spec["conv_kernel"]) - 1):
                h = SU.conv_stage(h, self.state, self.spec, SU.Evaluation(mode), i, i + 1)
                outs[i] = h
            self.prefix[mode] = outs
        return SU.conv_stage(self.prefix[mode][layer - 1], self.state, self.spec, SU.Evaluation(mode, drop), layer)


class EntryStage(Stage):
    """audio -> hidden[0] (``SU.entry_stage``).  A dropped term restarts where it acts: in the conv stack as ``ConvStage`` does,
    then the intact front; in the front from the intact emulation's conv output."""

    def __init__(self, audio, lengths, frames, state, spec, want):
        super().__init__("entry", lambda ev: SU.entry_stage(audio, lengths, frames, state, spec, ev), want, frames)
        self.conv = ConvStage(SU.normalize(audio, lengths, spec, SU.Evaluation("fp32")), state, spec, None, frames)
        self.state, self.spec, self.intact = state, spec, {}

    def run_dropped(self, mode, drop):
        if drop[0].startswith("conv"):
            return SU.front_stage(self.conv.run_dropped(mode, drop), self.frames, self.state, self.spec, SU.Evaluation(mode))
        if mode not in self.intact:
            self.intact[mode] = self.conv.run(SU.Evaluation(mode))
        return SU.front_stage(self.intact[mode], self.frames, self.state, self.spec, SU.Evaluation(mode, drop))


class Case:
    def __init__(self, name):
        from oracle import allophant_oracle as O

        self.name = name
        recipe = CASES[name]
        self._measured = {}
        if recipe.heads_only:
            spec, state, inventories = recipe.build()
            audio, lengths = SU.heads_audio(HEADS_AUDIO_SEED)
            offsets = synthetic.category_offsets(spec) if spec.get("embedding_size") else None
            with torch.inference_mode():
                hidden, frames, _ = O.wav2vec2_hidden_states(audio, lengths, state, spec, False, False)
            heads_in = {i: hidden[i] for i in SU.hidden_inputs(spec)}
            self.stages = []
            for tfi in inventories:
                with torch.inference_mode():
                    raw = O.projection_forward([h.transpose(0, 1) for h in hidden], state, spec, tfi, offsets, frames)
                    ref = {k: torch.log_softmax(v, -1) for k, v in raw.items()}
                stage = "heads" if tfi is None or len(inventories) == 1 else f"heads/{tfi.shape[0]}"
                self.stages.append(Stage(stage, lambda ev, tfi=tfi: _named(*SU.heads_stage(heads_in, frames, state, spec, tfi, offsets, ev)),
                                         _named(raw, ref, transpose=True), frames))
            return
        spec, state, tfi, audio, lengths = recipe.build()
        offsets = synthetic.category_offsets(spec)
        if recipe.tail_only:
            with torch.inference_mode():
                ref, frames, inter = O.predict(audio, lengths, state, spec, tfi, offsets, keep_intermediates=True)
                hidden = inter["hidden_states"]
                raw = O.projection_forward([h.transpose(0, 1) for h in hidden], state, spec, tfi, offsets, frames)
            last = spec["layers"]
            taps = {i: hidden[i] for i in SU.hidden_inputs(spec) if i != last}

            def tail(ev):
                return _named(*SU.tail_stage(hidden[last - 1], taps, frames, state, spec, tfi, offsets, ev))

            self.stages = [Stage("tail", tail, _named(raw, ref, transpose=True), frames)]
            return
        with torch.inference_mode():
            ref, frames, inter = O.predict(audio, lengths, state, spec, tfi, offsets, keep_intermediates=True)
            hidden = inter["hidden_states"]
            raw = O.projection_forward([h.transpose(0, 1) for h in hidden], state, spec, tfi, offsets, frames)
        # the layer-norm extractor is local in time (frame t reads samples 320 t .. 320 t + 399, no mask, no statistics over time):
        # its first second stands for the rest, and keeps the 12 dropped-term evaluations of a 512-wide stack to seconds
        x, conv_frames = inter["normed_audio"], frames
        if spec.get("feat_extract_norm", "layer") == "layer" and x.shape[1] > 16000:
            x = x[:, :16000]
            conv_frames = torch.minimum(frames, O.downsampled_lengths(torch.tensor(16000), spec["conv_kernel"], spec["conv_stride"]))
        self.stages = [ConvStage(x, state, spec, inter["conv_out"], conv_frames),
                       Stage("front", lambda ev: SU.front_stage(inter["conv_out"], frames, state, spec, ev), hidden[0], frames)]
        for i in range(spec["layers"]):
            self.stages.append(Stage(f"layer{i}", lambda ev, i=i: SU.layer_stage(hidden[i], frames, state, spec, ev, i), hidden[i + 1], frames))
            if recipe.fold:  # the same layer as a pass with the LayerNorm fold runs it: the stream rounded to planes
                self.stages.append(Stage(f"layer{i}/fold", lambda ev, i=i: SU.layer_stage(hidden[i], frames, state, spec, ev, i, fold=True),
                                         hidden[i + 1], frames))
        heads_in = {i: hidden[i] for i in SU.hidden_inputs(spec)}
        self.stages.append(Stage("heads", lambda ev: _named(*SU.heads_stage(heads_in, frames, state, spec, tfi, offsets, ev)),
                                 _named(raw, ref, transpose=True), frames))
        if recipe.entry:
            # audio -> hidden[0] in one.  The positional convolution reaches 64 frames either way, so the truncated audio of the
            # conv stage needs an oracle run of its own: the first second of every utterance as a batch
            cut = x.shape[1]
            if cut < audio.shape[1]:
                audio, lengths = audio[:, :cut].contiguous(), lengths.clamp(max=cut)
                with torch.inference_mode():
                    _, frames0, inter0 = O.predict(audio, lengths, state, spec, tfi, offsets, keep_intermediates=True)
            else:
                frames0, inter0 = frames, inter
            self.stages.append(EntryStage(audio, lengths, frames0, state, spec, inter0["hidden_states"][0]))

    def measured(self, stage, modes=("fp32", "f16x3", "bf16x3")):
        """(truth, {mode: error against truth}, products of the stage), computed once per stage"""
        if stage.name not in self._measured:
            with torch.inference_mode():
                truth = stage.run(SU.Evaluation("truth"))
                errors, products = {}, []
                for mode in modes:
                    ev = SU.Evaluation(mode)
                    errors[mode] = SU.against(stage.run(ev), truth, stage.frames)
                    products = ev.seen
            self._measured[stage.name] = (truth, errors, products)
        return self._measured[stage.name]


_cases = {}


@pytest.fixture(params=list(CASES))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def test_evaluation_splits_and_drops():
    """the product hook itself: planes, the three products, one term left out"""
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(5, 64, generator=g), torch.randn(64, 7, generator=g)
    exact = x.double() @ w.double()
    full = SU.Evaluation("f16x3").matmul("p", x, w)
    assert (full.double() - exact).abs().max() < 2e-5          # 64 terms of O(1) at 2^-22 each
    for side in ("lo_x", "lo_w"):
        ev = SU.Evaluation("f16x3", ("p", side))
        lost = ev.matmul("p", x, w)
        assert 1e-4 < (lost.double() - exact).abs().max() < 2e-2  # one operand at 2^-11
        assert torch.equal(ev.matmul("other", x, w), full) and ev.seen == ["p", "other"]
    assert SU.Evaluation("truth").matmul("p", x.double(), w.double()).dtype == torch.float64
    with pytest.raises(ValueError):
        SU.Evaluation("fp32", ("p", "lo_x"))


def test_shortest_longest_and():
    lengths = torch.tensor([50, 10, 40, 90, 20, 70])
    assert SU.shortest_longest_and(lengths, 1) == [1, 2, 3] and SU.shortest_longest_and(lengths, 2) == [0, 1, 3, 4]


def test_stages_restate_the_oracle(case):
    """each stage fed the oracle's intermediate gives the oracle's next intermediate, to fp32 rounding"""
    with torch.inference_mode():
        for stage in case.stages:
            worst = SU.against(stage.run(SU.Evaluation("fp32")), stage.want, stage.frames)
            print(f"[stage_util] {case.name} {stage.name}: restated fp32 vs oracle {worst:.3g}")
            wants = stage.want.values() if isinstance(stage.want, dict) else [stage.want]
            scale = max(1.0, max(float(w.abs().max()) for w in wants))
            assert worst < FP32_ROUNDING * scale, (case.name, stage.name, worst, scale)


def test_emulation_is_fp32_grade(case):
    """e_emu (fp16 planes) within 8 x of the fp32 evaluation's own error, both against float64"""
    for stage in case.stages:
        _, errors, _ = case.measured(stage)
        print(f"[stage_util] {case.name} {stage.name}: vs fp64: fp32 {errors['fp32']:.3g}  f16x3 {errors['f16x3']:.3g}  bf16x3 {errors['bf16x3']:.3g}")
        assert errors["f16x3"] <= EMU_OVER_FP32 * errors["fp32"], (case.name, stage.name, errors)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_every_lost_cross_term_is_separated(case, mode):
    """the separation condition, for every product of every stage and each of its two cross terms"""
    failures, listed = [], set()
    with torch.inference_mode():
        for stage in case.stages:
            if (case.name, mode, stage.name) in SU.NOT_CLAIMED:
                continue
            truth, errors, products = case.measured(stage)
            e_emu = errors[mode]
            for product in products:
                for term in ("lo_x", "lo_w"):
                    ratio = SU.against(stage.run_dropped(mode, (product, term)), truth, stage.frames) / e_emu
                    key = (case.name, mode, stage.name, product, term)
                    print(f"[stage_util] {case.name} {mode} {stage.name}: {product} without {term}: {ratio:.1f} x e_emu ({e_emu:.3g})")
                    if key in NOT_DETECTABLE:
                        listed.add(key)
                        if ratio < LISTED_FLOOR:
                            failures.append((key, ratio, "listed, and below the floor of the listed ones"))
                    elif ratio < SEPARATION:
                        failures.append((key, ratio, "below the separation condition"))
    assert not failures, failures
    assert all(k[3] in LISTABLE_IN_COMBINED for k in listed if k[2] in ("entry", "tail")), listed
    assert listed == {k for k in NOT_DETECTABLE if k[0] == case.name and k[1] == mode}
