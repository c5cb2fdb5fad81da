"""The cases of tests/test_gpu_stage_row_edges.py: batches whose encoder row count ``M`` ends a chosen number of rows into the last
row tile of each product of a layer, and what every case is there for.  tests/test_gemm_routes.py proves the table on the CPU
(``route_dump rows``: the route of each product at that ``M``), the GPU cases pin ``rows``, ``packed`` and ``ln_fold``.

Batch recipe (rows are packed in utterance order, so the tail lies in the last partial tile and on the boundary before it):

  body    fixed utterances of 10 s (499 frames) that set the order of magnitude of ``M``: ``("equal", n)``, the ragged 16 of
          ``test_fold_on_packed_rows`` (``("ragged16",)``, 6631 rows) or none
  filler  one utterance of ``filler`` frames that steers ``M`` to the wanted value
  tail    the same short utterances in every case of a family: ``TAIL`` (294 rows, more than the tallest tile; the last one has a
          single frame) or, for products of fewer than 256 rows, ``SHORT_TAIL`` (98 rows).  Only the tail is judged.

``("padded", n)`` is ``n`` utterances of ``T`` frames each and nothing else: equal lengths, hence the padded layout.

Per product the table names the kernel (``PP`` ping-pong, ``DMA`` LDS-DMA tiles, ``TILE`` register-staged tiles), the tile
(rows x columns), the residue ``r = M mod tile rows``, the LayerNorm-fold role and the K chunks.  XLS-R 300M on 256 CUs:

  fold256    all four products on 256-row ping-pong tiles under the fold exist between about 13.6 k and 16.3 k rows only, so the
             body is 27 x 10 s.  r in {1, 8, 9, 32, 33, 127, 128, 129, 255}: one valid row, a lane's 8-row run, the 32-row
             staging round, HALF - 1, HALF, HALF + 1 (HALF = 128), one missing row.
  fold128    at the row count of ``test_fold_on_packed_rows`` (about 6.6 k .. 7.2 k) the fold holds, but only FFN1 takes 256-row
             tiles: QKV and both producers run 128-row tiles (HALF = 64).  r in {1, 63, 64, 65, 127} of those.
  plain128   no fold, about 2.3 k packed rows: 128-row tiles for QKV (256 columns: the fast scatter on whole wave groups), the
             out-projection and FFN2 (192 columns, NI = 3: the generic epilogue throughout; FFN2 with 2 K chunks), 256-row
             192-column tiles for FFN1.  r in {1, 8, 9, 33, 63, 64, 65, 127}.
  threshold  both sides of 384 (``PP_MIN_ROWS``), 768 (``dma_preferred_shape``) and 4096 (``DMA_MAX_ROWS``).  Of the three only
             768 moves a layer product here (FFN2: LDS-DMA 64 x 32 -> ping-pong with 8 K chunks): below 768 rows the LDS-DMA
             tiles are preferred wherever they fit one round, which they do at 383 .. 385 for every product, so
             ``PP_MIN_ROWS`` decides nothing; and from 2049 rows on no N = 1024 product fits one round of 128 x 64 tiles, so
             neither does ``DMA_MAX_ROWS``.  At 4097 the plan changes for another reason (tile widths and FFN2's K chunks).
             384, 768 and 4096 end on a whole tile: the control.
  short      LDS-DMA tiles with K chunks (FFN2: 4 chunks up to 128 rows, 2 up to 256, none beyond), whose partial slabs go through
             ``splitk_fixup_rownorm_kernel`` (4 rows per workgroup) or ``splitk_fixup_kernel`` (64 x 64 blocks).  M mod 64 and
             M mod 128 in {1, 63 / 127}, M mod 4 in {1, 3}.  Both DMA shapes occur in the table (128 x 64: threshold/383 .. 385);
             no layer product of this width takes the register-staged tile.  7 utterances do not fill the window positional
             convolution, so the rows are packed behind the grouped one (``packed`` 1).
  padded     T = 7, 8, 9 frames per utterance, equal lengths.  At about 2.3 k rows QKV runs 128 x 256 ping-pong tiles, whose fast
             scatter needs ``T >= 8`` and wraps ``t`` once per 8-row step (T = 8: every step, T = 9: every step but at a moving
             row); T = 7 falls to the generic epilogue.  3 utterances of the same T stay on 64 x 32 LDS-DMA tiles (FFN2: 4 K chunks).
"""
from typing import Dict, List, NamedTuple, Tuple

TAIL = (49, 49, 49, 49, 49, 24, 9, 8, 7, 1)
SHORT_TAIL = (49, 24, 9, 8, 7, 1)
BODY_FRAMES = 499  # 10 s
PRODUCTS = ("qkv", "oproj", "ffn1", "ffn2")
ROLES = ("plain", "consumer", "producer")  # GemmRoute.fold


class Route(NamedTuple):
    kernel: str
    tile_rows: int
    tile_cols: int
    residue: int
    role: str
    chunks: int


class Case(NamedTuple):
    name: str
    family: str
    precisions: Tuple[str, ...]
    body: tuple
    filler: int  # frames
    tail: Tuple[int, ...]
    M: int
    T: int  # padded family: frames per utterance
    packed: int  # pass_info()["packed"]
    ln_fold: int
    products: Dict[str, Route]


_TABLE = [
    # name, precisions, body, filler frames, tail, M, T, packed, ln_fold, routes
    # ---- fold256 ----
    ("fold256/r1", "f16x3 bf16x3", ('equal', 27), 58, TAIL, 13825, 0, 2, 1,
     "qkv PP 256x256 r1 consumer k1 | oproj PP 256x256 r1 producer k1 | ffn1 PP 256x256 r1 consumer k1 | ffn2 PP 256x256 r1 producer k1"),
    ("fold256/r8", "f16x3", ('equal', 27), 65, TAIL, 13832, 0, 2, 1,
     "qkv PP 256x256 r8 consumer k1 | oproj PP 256x256 r8 producer k1 | ffn1 PP 256x256 r8 consumer k1 | ffn2 PP 256x256 r8 producer k1"),
    ("fold256/r9", "f16x3", ('equal', 27), 66, TAIL, 13833, 0, 2, 1,
     "qkv PP 256x256 r9 consumer k1 | oproj PP 256x256 r9 producer k1 | ffn1 PP 256x256 r9 consumer k1 | ffn2 PP 256x256 r9 producer k1"),
    ("fold256/r32", "f16x3", ('equal', 27), 89, TAIL, 13856, 0, 2, 1,
     "qkv PP 256x256 r32 consumer k1 | oproj PP 256x256 r32 producer k1 | ffn1 PP 256x256 r32 consumer k1 | ffn2 PP 256x256 r32 producer k1"),
    ("fold256/r33", "f16x3", ('equal', 27), 90, TAIL, 13857, 0, 2, 1,
     "qkv PP 256x256 r33 consumer k1 | oproj PP 256x256 r33 producer k1 | ffn1 PP 256x256 r33 consumer k1 | ffn2 PP 256x256 r33 producer k1"),
    ("fold256/r127", "f16x3", ('equal', 27), 184, TAIL, 13951, 0, 2, 1,
     "qkv PP 256x256 r127 consumer k1 | oproj PP 256x256 r127 producer k1 | ffn1 PP 256x256 r127 consumer k1 | ffn2 PP 256x256 r127 producer k1"),
    ("fold256/r128", "f16x3", ('equal', 27), 185, TAIL, 13952, 0, 2, 1,
     "qkv PP 256x256 r128 consumer k1 | oproj PP 256x256 r128 producer k1 | ffn1 PP 256x256 r128 consumer k1 | ffn2 PP 256x256 r128 producer k1"),
    ("fold256/r129", "f16x3 bf16x3", ('equal', 27), 186, TAIL, 13953, 0, 2, 1,
     "qkv PP 256x256 r129 consumer k1 | oproj PP 256x256 r129 producer k1 | ffn1 PP 256x256 r129 consumer k1 | ffn2 PP 256x256 r129 producer k1"),
    ("fold256/r255", "f16x3 bf16x3", ('equal', 27), 56, TAIL, 13823, 0, 2, 1,
     "qkv PP 256x256 r255 consumer k1 | oproj PP 256x256 r255 producer k1 | ffn1 PP 256x256 r255 consumer k1 | ffn2 PP 256x256 r255 producer k1"),
    # ---- fold128 ----
    ("fold128/r1", "f16x3", ('ragged16',), 116, TAIL, 7041, 0, 2, 1,
     "qkv PP 128x256 r1 consumer k1 | oproj PP 128x256 r1 producer k1 | ffn1 PP 256x256 r129 consumer k1 | ffn2 PP 128x256 r1 producer k1"),
    ("fold128/r63", "f16x3", ('ragged16',), 50, TAIL, 6975, 0, 2, 1,
     "qkv PP 128x256 r63 consumer k1 | oproj PP 128x256 r63 producer k1 | ffn1 PP 256x256 r63 consumer k1 | ffn2 PP 128x256 r63 producer k1"),
    ("fold128/r64", "f16x3", ('ragged16',), 51, TAIL, 6976, 0, 2, 1,
     "qkv PP 128x256 r64 consumer k1 | oproj PP 128x256 r64 producer k1 | ffn1 PP 256x256 r64 consumer k1 | ffn2 PP 128x256 r64 producer k1"),
    ("fold128/r65", "f16x3", ('ragged16',), 52, TAIL, 6977, 0, 2, 1,
     "qkv PP 128x256 r65 consumer k1 | oproj PP 128x256 r65 producer k1 | ffn1 PP 256x256 r65 consumer k1 | ffn2 PP 128x256 r65 producer k1"),
    ("fold128/r127", "f16x3", ('ragged16',), 114, TAIL, 7039, 0, 2, 1,
     "qkv PP 128x256 r127 consumer k1 | oproj PP 128x256 r127 producer k1 | ffn1 PP 256x256 r127 consumer k1 | ffn2 PP 128x256 r127 producer k1"),
    # ---- plain128 ----
    ("plain128/r1", "f16x3 bf16x3", ('equal', 4), 15, TAIL, 2305, 0, 2, 0,
     "qkv PP 128x256 r1 plain k1 | oproj PP 128x192 r1 plain k1 | ffn1 PP 256x192 r1 plain k1 | ffn2 PP 128x192 r1 plain k2"),
    ("plain128/r8", "f16x3", ('equal', 4), 22, TAIL, 2312, 0, 2, 0,
     "qkv PP 128x256 r8 plain k1 | oproj PP 128x192 r8 plain k1 | ffn1 PP 256x192 r8 plain k1 | ffn2 PP 128x192 r8 plain k2"),
    ("plain128/r9", "f16x3", ('equal', 4), 23, TAIL, 2313, 0, 2, 0,
     "qkv PP 128x256 r9 plain k1 | oproj PP 128x192 r9 plain k1 | ffn1 PP 256x192 r9 plain k1 | ffn2 PP 128x192 r9 plain k2"),
    ("plain128/r33", "f16x3", ('equal', 4), 47, TAIL, 2337, 0, 2, 0,
     "qkv PP 128x256 r33 plain k1 | oproj PP 128x192 r33 plain k1 | ffn1 PP 256x192 r33 plain k1 | ffn2 PP 128x192 r33 plain k2"),
    ("plain128/r63", "f16x3", ('equal', 4), 77, TAIL, 2367, 0, 2, 0,
     "qkv PP 128x256 r63 plain k1 | oproj PP 128x192 r63 plain k1 | ffn1 PP 256x192 r63 plain k1 | ffn2 PP 128x192 r63 plain k2"),
    ("plain128/r64", "f16x3", ('equal', 4), 78, TAIL, 2368, 0, 2, 0,
     "qkv PP 128x256 r64 plain k1 | oproj PP 128x192 r64 plain k1 | ffn1 PP 256x192 r64 plain k1 | ffn2 PP 128x192 r64 plain k2"),
    ("plain128/r65", "f16x3 bf16x3", ('equal', 4), 79, TAIL, 2369, 0, 2, 0,
     "qkv PP 128x256 r65 plain k1 | oproj PP 128x192 r65 plain k1 | ffn1 PP 256x192 r65 plain k1 | ffn2 PP 128x192 r65 plain k2"),
    ("plain128/r127", "f16x3", ('equal', 4), 13, TAIL, 2303, 0, 2, 0,
     "qkv PP 128x256 r127 plain k1 | oproj PP 128x192 r127 plain k1 | ffn1 PP 256x192 r255 plain k1 | ffn2 PP 128x192 r127 plain k2"),
    # ---- threshold ----
    ("threshold/383", "f16x3", ('none',), 89, TAIL, 383, 0, 2, 0,
     "qkv DMA 128x64 r127 plain k1 | oproj DMA 64x32 r63 plain k1 | ffn1 DMA 128x64 r127 plain k1 | ffn2 DMA 64x32 r63 plain k1"),
    ("threshold/384", "f16x3", ('none',), 90, TAIL, 384, 0, 2, 0,
     "qkv DMA 128x64 r0 plain k1 | oproj DMA 64x32 r0 plain k1 | ffn1 DMA 128x64 r0 plain k1 | ffn2 DMA 64x32 r0 plain k1"),
    ("threshold/385", "f16x3", ('none',), 91, TAIL, 385, 0, 2, 0,
     "qkv DMA 128x64 r1 plain k1 | oproj DMA 64x32 r1 plain k1 | ffn1 DMA 128x64 r1 plain k1 | ffn2 DMA 64x32 r1 plain k1"),
    ("threshold/767", "f16x3", ('none',), 473, TAIL, 767, 0, 2, 0,
     "qkv PP 128x192 r127 plain k1 | oproj DMA 64x32 r63 plain k1 | ffn1 PP 128x192 r127 plain k1 | ffn2 DMA 64x32 r63 plain k1"),
    ("threshold/768", "f16x3", ('none',), 474, TAIL, 768, 0, 2, 0,
     "qkv PP 128x192 r0 plain k1 | oproj DMA 64x32 r0 plain k1 | ffn1 PP 128x192 r0 plain k1 | ffn2 PP 128x256 r0 plain k8"),
    ("threshold/769", "f16x3", ('none',), 475, TAIL, 769, 0, 2, 0,
     "qkv PP 128x192 r1 plain k1 | oproj DMA 64x32 r1 plain k1 | ffn1 PP 128x192 r1 plain k1 | ffn2 PP 128x256 r1 plain k8"),
    ("threshold/4095", "f16x3", ('equal', 7), 308, TAIL, 4095, 0, 2, 0,
     "qkv PP 256x192 r255 plain k1 | oproj PP 128x192 r127 plain k1 | ffn1 PP 256x256 r255 plain k1 | ffn2 PP 128x256 r127 plain k2"),
    ("threshold/4096", "f16x3", ('equal', 7), 309, TAIL, 4096, 0, 2, 0,
     "qkv PP 256x192 r0 plain k1 | oproj PP 128x192 r0 plain k1 | ffn1 PP 256x256 r0 plain k1 | ffn2 PP 128x256 r0 plain k2"),
    ("threshold/4097", "f16x3", ('equal', 7), 310, TAIL, 4097, 0, 2, 0,
     "qkv PP 256x256 r1 plain k1 | oproj PP 128x192 r1 plain k1 | ffn1 PP 128x192 r1 plain k1 | ffn2 PP 128x192 r1 plain k1"),
    # ---- short ----
    ("short/127", "f16x3 bf16x3", ('none',), 29, SHORT_TAIL, 127, 0, 1, 0,
     "qkv DMA 64x32 r63 plain k1 | oproj DMA 64x32 r63 plain k1 | ffn1 DMA 64x32 r63 plain k1 | ffn2 DMA 64x32 r63 plain k4"),
    ("short/129", "f16x3 bf16x3", ('none',), 31, SHORT_TAIL, 129, 0, 1, 0,
     "qkv DMA 64x32 r1 plain k1 | oproj DMA 64x32 r1 plain k1 | ffn1 DMA 64x32 r1 plain k1 | ffn2 DMA 64x32 r1 plain k2"),
    ("short/193", "f16x3 bf16x3", ('none',), 95, SHORT_TAIL, 193, 0, 1, 0,
     "qkv DMA 64x32 r1 plain k1 | oproj DMA 64x32 r1 plain k1 | ffn1 DMA 64x32 r1 plain k1 | ffn2 DMA 64x32 r1 plain k2"),
    ("short/255", "f16x3 bf16x3", ('none',), 157, SHORT_TAIL, 255, 0, 1, 0,
     "qkv DMA 64x32 r63 plain k1 | oproj DMA 64x32 r63 plain k1 | ffn1 DMA 64x32 r63 plain k1 | ffn2 DMA 64x32 r63 plain k2"),
    # ---- padded ----
    ("padded/T7x330", "f16x3", ('padded', 330), 0, (), 2310, 7, 0, 0,
     "qkv PP 128x256 r6 plain k1 | oproj PP 128x192 r6 plain k1 | ffn1 PP 256x192 r6 plain k1 | ffn2 PP 128x192 r6 plain k2"),
    ("padded/T7x3", "f16x3", ('padded', 3), 0, (), 21, 7, 0, 0,
     "qkv DMA 64x32 r21 plain k1 | oproj DMA 64x32 r21 plain k1 | ffn1 DMA 64x32 r21 plain k1 | ffn2 DMA 64x32 r21 plain k4"),
    ("padded/T8x289", "f16x3", ('padded', 289), 0, (), 2312, 8, 0, 0,
     "qkv PP 128x256 r8 plain k1 | oproj PP 128x192 r8 plain k1 | ffn1 PP 256x192 r8 plain k1 | ffn2 PP 128x192 r8 plain k2"),
    ("padded/T8x3", "f16x3", ('padded', 3), 0, (), 24, 8, 0, 0,
     "qkv DMA 64x32 r24 plain k1 | oproj DMA 64x32 r24 plain k1 | ffn1 DMA 64x32 r24 plain k1 | ffn2 DMA 64x32 r24 plain k4"),
    ("padded/T9x257", "f16x3", ('padded', 257), 0, (), 2313, 9, 0, 0,
     "qkv PP 128x256 r9 plain k1 | oproj PP 128x192 r9 plain k1 | ffn1 PP 256x192 r9 plain k1 | ffn2 PP 128x192 r9 plain k2"),
    ("padded/T9x3", "f16x3", ('padded', 3), 0, (), 27, 9, 0, 0,
     "qkv DMA 64x32 r27 plain k1 | oproj DMA 64x32 r27 plain k1 | ffn1 DMA 64x32 r27 plain k1 | ffn2 DMA 64x32 r27 plain k4"),
]


def _routes(text: str) -> Dict[str, Route]:
    out = {}
    for part in text.split(" | "):
        product, kernel, tile, residue, role, chunks = part.split()
        rows, cols = tile.split("x")
        assert product in PRODUCTS and role in ROLES and residue[0] == "r" and chunks[0] == "k", part
        out[product] = Route(kernel, int(rows), int(cols), int(residue[1:]), role, int(chunks[1:]))
    assert tuple(out) == PRODUCTS, text
    return out


CASES: Dict[str, Case] = {
    name: Case(name, name.split("/")[0], tuple(precisions.split()), body, filler, tuple(tail), M, T, packed, ln_fold, _routes(routes))
    for name, precisions, body, filler, tail, M, T, packed, ln_fold, routes in _TABLE}
assert len(CASES) == len(_TABLE)

GPU_CASES: List[Tuple[str, str]] = [(name, precision) for name, case in CASES.items() for precision in case.precisions]


def samples(frames: int) -> int:
    """the shortest utterance of ``frames`` frames: the extractor's receptive field is 400 samples, its stride 320"""
    return 400 + 320 * (frames - 1)


def utterance_frames(case: Case) -> List[int]:
    """the frame count of every utterance of the case's batch, in batch order (body, filler, tail)"""
    kind = case.body[0]
    if kind == "padded":
        return [case.T] * case.body[1]
    if kind == "equal":
        body = [BODY_FRAMES] * case.body[1]
    elif kind == "ragged16":
        from allophant_amd import spec as S
        body = S.frame_lengths(_ragged16()[1].tolist(), S.xlsr_300m_encoder())
    else:
        assert kind == "none", kind
        body = []
    return list(body) + [case.filler] + list(case.tail)


def _ragged16():
    from allophant_amd import synthetic
    return synthetic.make_audio(16, 160000, seed=4000, ragged=True)  # ``fold_batch`` of tests/test_gpu_stage_production.py


def batch(case: Case):
    """(audio [N, L], lengths [N], the indices of the judged utterances): the tail, or for the padded family the first utterance
    and the last two, which lie in and in front of the last 128-row tile.  An utterance's samples do not depend on the case: the tail
    of a family is the same audio whatever stands in front of it."""
    import torch
    from allophant_amd import synthetic

    if case.body[0] == "padded":
        n = case.body[1]
        audio, lengths = synthetic.make_audio(n, samples(case.T), seed=7000 + case.T)
        # (the last tile holds 6 .. 9 rows here, i.e. the last utterance or part of it: the one before it ends on the boundary)
        return audio, lengths, sorted({0, n - 2, n - 1})
    parts = []
    if case.body[0] == "equal":
        parts.append(synthetic.make_audio(case.body[1], samples(BODY_FRAMES), seed=7100))
    elif case.body[0] == "ragged16":
        parts.append(_ragged16())
    parts.append(synthetic.make_audio(1, samples(case.filler), seed=7200))
    parts += [synthetic.make_audio(1, samples(f), seed=7300 + i) for i, f in enumerate(case.tail)]
    longest = max(a.shape[1] for a, _ in parts)
    audio = torch.cat([torch.nn.functional.pad(a, (0, longest - a.shape[1])) for a, _ in parts])
    lengths = torch.cat([l for _, l in parts])
    n = audio.shape[0]
    return audio, lengths, list(range(n - len(case.tail), n))
