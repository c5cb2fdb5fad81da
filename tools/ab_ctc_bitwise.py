"""Developer check: SHA-256 of every output buffer of the CTC entry points, for comparing two builds of the library bit for
bit (``tools/ab_bitwise.py`` does the same for ``predict()``):

    tools/ab_build.sh HEAD head
    AMX_LIB_PATH=$PWD/build/ab/head.so python tools/ab_ctc_bitwise.py > a.txt
    python tools/ab_ctc_bitwise.py > b.txt; diff a.txt b.txt    # the working tree's library

A tiny model predicts two utterances of 1.5 s and 3 s.  Greedy and beam decoding, alignment and scoring (with and without
posteriors, and with 3 candidates) run in the handle form over the ``Predictions`` and in the emissions form over the
transposed view of each output; the search (with curves) has the emissions form only.  The target rows hold 0, 1, 31, 32, 33
and 130 symbols (one strip, the strip's edge, several waves; 130 symbols do not fit the frames of the short utterance), and the
last row of each call is malformed (it names the blank).  Rows without a result leave their buffers unwritten, so every buffer
is filled with a sentinel before its call."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from allophant_amd import alignment, ctc, lib as L, scoring, spec as S, synthetic
from allophant_amd.estimator import Batch, Estimator

COUNTS = (0, 1, 31, 32, 33, 130, 130)  # (an odd cycle: over rows n, n + 1, ... every count meets either utterance)
lib = L.load()
device = torch.device("cuda", 0)
stream = torch.cuda.current_stream(device).cuda_stream
rng = np.random.default_rng(7)


def target_rows(rows: int, classes: int):
    """``rows`` rows of COUNTS symbols in turn, no symbol twice in a row (each needs exactly its length in frames); the last
    row names the blank."""
    out = []
    for r in range(rows):
        row = []
        while len(row) < COUNTS[r % len(COUNTS)]:
            v = int(rng.integers(1, classes))
            if not row or v != row[-1] or classes == 2:
                row.append(v)
        out.append(row)
    out[-1] = [1, 0]
    return out


def fill(*tensors):
    for t in tensors:
        if t is not None:
            t.view(torch.uint8).fill_(0xA5)  # the sentinel: -1515870811 / about -2.87e-16


def report(label: str, code: int, handle, **buffers):
    assert code == L.AMX_OK, (label, lib.amx_last_error(handle))
    torch.cuda.synchronize()
    for name, t in buffers.items():
        if t is not None:
            print(f"{label} {name}: {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


def packed(rows):
    offsets, ids, counts = ctc.pack_targets(rows)
    meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(device)
    return meta.data_ptr(), meta.data_ptr() + 4 * (len(rows) + 1), max(counts), meta


def decode_buffers(*leading, T, n_best=None, score=torch.float32):
    shape = leading if n_best is None else (*leading, n_best)
    tokens = torch.empty(*shape, T, dtype=torch.int64, device=device)
    out = dict(tokens=tokens, timesteps=torch.empty_like(tokens), counts=torch.empty(*shape, dtype=torch.int32, device=device),
               scores=torch.empty(*shape, dtype=score, device=device))
    if n_best is not None:
        out["hyp_counts"] = torch.empty(*leading, dtype=torch.int32, device=device)
    fill(*out.values())
    return out


def pointers(buffers):
    return [t.data_ptr() for t in buffers.values()]


def beam_workspace(rows, T, beam):
    size = C.c_size_t()
    L.check(lib, None, lib.amx_beam_ctc_workspace(beam, rows, T, C.byref(size)))
    return torch.empty(max(1, size.value), dtype=torch.uint8, device=device), size.value


def align_buffers(rows, T, max_target):
    b = alignment.allocate(lib, rows, T, max_target, device)
    fill(b.paths, b.frame_scores, b.spans, b.span_scores, b.totals, b.status)
    return b, dict(paths=b.paths, frame_scores=b.frame_scores, spans=b.spans, span_scores=b.span_scores, totals=b.totals,
                   status=b.status)


def score_buffers(rows, T, max_target, posteriors):
    b = scoring.allocate(lib, rows, T, max_target, device, posteriors)
    fill(b.log_likelihood, b.occupancy, b.position_sums, b.score_sums, b.posteriors, b.status)
    return b, dict(log_likelihood=b.log_likelihood, occupancy=b.occupancy, position_sums=b.position_sums,
                   score_sums=b.score_sums, posteriors=b.posteriors, status=b.status)


spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5,
                        n_values=3, allophone_layer=True)
spec["shared_phones"] = 11
est = Estimator(spec, synthetic.make_state_dict(spec, seed=1), device, "f16x3")
audio, _ = synthetic.make_audio(2, 48000, seed=99)
pred = est.predict(Batch(audio.cuda(), torch.tensor([24000, 48000]), torch.zeros(2, dtype=torch.long)),
                   synthetic.make_inventory(spec, 7, seed=1))
names = list(pred.outputs)
T, N = next(iter(pred.outputs.values())).shape[:2]
O, length = len(names), pred._geometry[1]
classes = min(t.shape[2] for t in pred.outputs.values())  # ids every output knows
host_lengths = pred.lengths.detach().to("cpu", torch.int64).contiguous()
fl, out = C.cast(host_lengths.data_ptr(), C.POINTER(C.c_int64)), pred._flat.data_ptr()
print(f"outputs {names}, frames {T}, lengths {host_lengths.tolist()}, classes {[t.shape[2] for t in pred.outputs.values()]}")

# ---- the handle form: every output block of the predictions, rows o * N + n ----
d = decode_buffers(O, N, T=T)
report("greedy", lib.amx_greedy_ctc(est._handle, out, fl, N, length, *pointers(d), stream), est._handle, **d)
d = decode_buffers(O, N, T=T, n_best=3, score=torch.float64)
workspace, size = beam_workspace(O * N, T, 8)
report("beam", lib.amx_beam_ctc(est._handle, out, fl, N, length, 8, 3, L.BEAM_EXP_EMISSIONS, workspace.data_ptr(), size,
                                *pointers(d), stream), est._handle, **d)
offsets, ids, max_target, _meta = packed(target_rows(O * N, classes))
b, named = align_buffers(O * N, T, max_target)
report("align", lib.amx_ctc_align(est._handle, out, fl, N, length, offsets, ids, max_target, *b.pointers(), stream),
       est._handle, **named)
for candidates, posteriors in ((1, False), (1, True), (3, False)):
    offsets, ids, max_target, _meta = packed(target_rows(O * N * candidates, classes))
    b, named = score_buffers(O * N * candidates, T, max_target, posteriors)
    report(f"score G={candidates}{' posteriors' if posteriors else ''}",
           lib.amx_ctc_score(est._handle, out, fl, N, length, candidates, offsets, ids, max_target, *b.pointers(), stream),
           est._handle, **named)

# ---- the emissions form: each output's [T, N, C] block through its transposed view ----
lengths_dev = host_lengths.to(device=device, dtype=torch.int32)
for name in names:
    em = pred.outputs[name].transpose(0, 1)
    Cn = em.shape[2]
    source = (0, em.data_ptr(), em.stride(0), em.stride(1), lengths_dev.data_ptr(), N, T, Cn, 0)
    d = decode_buffers(N, T=T)
    report(f"{name} greedy", lib.amx_greedy_ctc_emissions(*source, *pointers(d), stream), None, **d)
    d = decode_buffers(N, T=T, n_best=3, score=torch.float64)
    workspace, size = beam_workspace(N, T, 8)
    report(f"{name} beam", lib.amx_beam_ctc_emissions(*source, 8, 3, L.BEAM_EXP_EMISSIONS, workspace.data_ptr(), size,
                                                       *pointers(d), stream), None, **d)
    for candidates, posteriors in ((0, False), (1, False), (1, True), (3, False)):  # (0 candidates: the alignment)
        per_call = N * max(1, candidates)
        rows = target_rows(len(COUNTS) * per_call, Cn)
        for first in range(0, len(rows), per_call):  # (a call with each count in each place)
            offsets, ids, max_target, _meta = packed(rows[first:first + per_call])
            if candidates == 0:
                b, named = align_buffers(N, T, max_target)
                code = lib.amx_ctc_align_emissions(*source, offsets, ids, max_target, *b.pointers(), stream)
                label = f"{name} align rows {first}.."
            else:
                b, named = score_buffers(per_call, T, max_target, posteriors)
                code = lib.amx_ctc_score_emissions(*source, candidates, offsets, ids, max_target, *b.pointers(), stream)
                label = f"{name} score G={candidates}{' posteriors' if posteriors else ''} rows {first}.."
            report(label, code, None, **named)
    queries = [row for row in target_rows(12, Cn)[:-1] if row] + [[1, 0]]
    q_offsets, q_ids, max_query, _meta = packed(queries)
    Q = len(queries)
    size = C.c_size_t()
    L.check(lib, None, lib.amx_ctc_search_workspace(N, Q, T, max_query, C.byref(size)))
    workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    found = dict(scores=torch.empty(N, Q, device=device), spans=torch.empty(N, Q, 2, dtype=torch.int32, device=device),
                 status=torch.empty(N, Q, dtype=torch.int32, device=device), end_scores=torch.empty(N, Q, T, device=device),
                 end_starts=torch.empty(N, Q, T, dtype=torch.int32, device=device))
    fill(*found.values())
    report(f"{name} search", lib.amx_ctc_search_emissions(*source, q_offsets, q_ids, Q, max_query, workspace.data_ptr(), size.value,
                                                          *pointers(found), stream), None, **found)
est.close()
