"""The contract of amx_restrict_outputs (include/allophant_amx_restrict.h) restated in float64 as a plain loop, the fp32
yardstick its error is measured against, the membership bit table, and the set-up of the end-to-end tests."""
import math

import numpy as np
import torch

NORMALIZE = 1  # AMX_RESTRICT_NORMALIZE


def restrict(src, frame_lengths, language_ids, members, flags, out=None):
    """``src`` [T, N, C] (numpy), ``members[l]`` the classes of language l.  Returns (out float64 [T, N, C], status [N]); a
    malformed utterance keeps what ``out`` held (NaN where none is given)."""
    src = np.asarray(src)
    T, N, C = src.shape
    out = np.full((T, N, C), np.nan) if out is None else np.array(out, dtype=np.float64)
    status = np.zeros(N, dtype=np.int32)
    for n in range(N):
        l, length = int(language_ids[n]), int(frame_lengths[n])
        if not 0 <= l < len(members) or not 0 <= length <= T:
            status[n] = -2
            continue
        own = [int(c) for c in members[l]]
        for t in range(T):
            if t >= length:
                out[t, n, :] = 0.0
                continue
            row = [float(src[t, n, c]) for c in own]
            m = max(row, default=-math.inf)
            if m == -math.inf:
                lse = -math.inf
            else:
                lse = m + math.log(sum(math.exp(x - m) for x in row))
            out[t, n, :] = -math.inf
            for c, x in zip(own, row):
                if flags & NORMALIZE:
                    out[t, n, c] = -math.inf if lse == -math.inf else x - lse
                else:
                    out[t, n, c] = x
    return out, status


def yardstick(src, frame_lengths, language_ids, members):
    """torch's CPU fp32 ``log_softmax`` over the gathered member columns, scattered back ([T, N, C] float32; NaN wherever the
    restatement does not put a normalised member)."""
    src = torch.as_tensor(np.asarray(src), dtype=torch.float32)
    T, N, C = src.shape
    out = torch.full((T, N, C), float("nan"))
    for n in range(N):
        own = torch.tensor([int(c) for c in members[int(language_ids[n])]], dtype=torch.int64)
        length = int(frame_lengths[n])
        if own.numel() and length:
            out[:length, n, own] = torch.log_softmax(src[:length, n][:, own], dim=-1)
    return out.numpy()


def member_bits(members, classes):
    """uint64 [languages, (classes + 63) // 64]: bit c % 64 of word c // 64 is set where class c belongs to the language."""
    bits = np.zeros((len(members), (classes + 63) // 64), dtype=np.uint64)
    for l, own in enumerate(members):
        for c in own:
            bits[l, int(c) // 64] |= np.uint64(1) << np.uint64(int(c) % 64)
    return bits


class EndToEnd:
    """The mixed-language batch of the end-to-end tests: a tiny composition model, six ragged utterances, a pool of 61
    distinct phonemes and the languages a, b, c of 1, 7 and 23 of them; utterance languages a b c c a b."""

    LANGUAGES = ("a", "b", "c", "c", "a", "b")

    def __init__(self):
        from allophant_amd import spec as S, synthetic
        from allophant_amd.inventories import LanguageInventories

        self.spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9,
                                     n_features=5)
        self.state = synthetic.make_state_dict(self.spec, seed=21)
        self.audio, self.lengths = synthetic.make_audio(6, 9000, seed=77, ragged=True)
        self.offsets = synthetic.category_offsets(self.spec)
        rows = synthetic.make_inventory(self.spec, 70, seed=3)
        seen, distinct = set(), []
        for row in rows.tolist():
            if tuple(row) not in seen:
                seen.add(tuple(row))
                distinct.append(row)
        self.pool = torch.tensor(distinct, dtype=torch.int64)
        g = torch.Generator().manual_seed(5)
        self.picks = {}
        for language, count in (("a", 1), ("b", 7), ("c", 23)):
            self.picks[language] = torch.randperm(self.pool.shape[0], generator=g)[:count].sort().values
        self.matrices = {language: self.pool[index] for language, index in self.picks.items()}
        self.inventories = LanguageInventories.from_matrices(self.matrices)
        self._oracle = {}

    def oracle(self, language, log_probabilities=True):
        """``O.predict`` of the whole batch under the language's own matrix: (outputs, frame lengths), computed once."""
        from oracle import allophant_oracle as O

        key = (language, log_probabilities)
        if key not in self._oracle:
            self._oracle[key] = O.predict(self.audio, self.lengths, self.state, self.spec, self.matrices[language], self.offsets,
                                          log_probabilities=log_probabilities)
        return self._oracle[key]

    def oracle_union(self, log_probabilities=True):
        from oracle import allophant_oracle as O

        key = ("<union>", log_probabilities)
        if key not in self._oracle:
            self._oracle[key] = O.predict(self.audio, self.lengths, self.state, self.spec, self.inventories.union_tfi,
                                          self.offsets, log_probabilities=log_probabilities)
        return self._oracle[key]
