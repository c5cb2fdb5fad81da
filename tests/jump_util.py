"""Residual-jump checkpoints of the LayerNorm-fold tests (CPU only: the GPU tests in test_gpu_fold_range.py and the emulation in
diagnostics/emulate_ln_fold.py use the same definition of sigma).

One channel of the bias of ``attention.out_proj`` or ``feed_forward.output_dense`` of an encoder layer is raised by ``m x sigma``,
with sigma the smallest standard deviation of a valid row of the CPU oracle's hidden state at that layer on the 2 x 3 s batch
``short_batch``: every valid row of that batch sees at most m of its own sigmas."""
import torch

from allophant_amd import spec as S, synthetic

AM = "_acoustic_model._model."
SUBLAYERS = {"out_proj": "attention.out_proj", "ffn2": "feed_forward.output_dense"}
CHANNEL = 7


def xlsr_spec():
    spec = S.multitask_spec(S.xlsr_300m_encoder(), allophone_layer=True)
    spec["shared_phones"] = 80
    return spec


def short_batch():
    """2 ragged 3 s utterances: below the fold's threshold, and the batch sigma is measured on"""
    return synthetic.make_audio(2, 48000, seed=777, ragged=True)


def row_sigma(state, spec, layer):
    """the smallest standard deviation of a valid row of the oracle's hidden state `layer` (the input of encoder layer `layer`)"""
    from oracle import allophant_oracle as O

    audio, lengths = short_batch()
    with torch.inference_mode():
        hidden, frames, _ = O.wav2vec2_hidden_states(audio, lengths, state, spec)
    h = hidden[layer]
    rows = torch.cat([h[n, :int(frames[n])] for n in range(h.shape[0])])
    return float(rows.std(-1, unbiased=False).min())


def add_jump(state, spec, layer, sublayer, multiple, channel=CHANNEL):
    """raises one channel of the sublayer's bias by `multiple` x row_sigma(layer); returns the increment"""
    step = multiple * row_sigma(state, spec, layer)
    key = f"{AM}encoder.layers.{layer}.{SUBLAYERS[sublayer]}.bias"
    state[key] = state[key].clone()
    state[key][channel] += step
    return step


def jump_state(layer, sublayer, multiple):
    """the XLS-R-shape synthetic checkpoint (seed 0) with one jump"""
    spec = xlsr_spec()
    state = synthetic.make_state_dict(spec, seed=0)
    add_jump(state, spec, layer, sublayer, multiple)
    return spec, state
