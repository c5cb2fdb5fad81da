"""The call frame that the CTC entry points share (``allophant_amd/ctc.py``): one packer behind ``alignment.pack_targets``,
``scoring.pack_targets`` and ``search.pack_queries``, and one emission prelude that keeps each entry point's own messages."""
import pytest
import torch

from allophant_amd import alignment, scoring, search
from allophant_amd.estimator import beam_ctc_decode, greedy_ctc_decode


@pytest.mark.parametrize("rows", [[], [[]], [[], [3]], [[1, 2], [], [3], [4, 4]], [[2] * 256, [1]]])
def test_one_packer(rows):
    offsets, ids, counts = alignment.pack_targets(rows)
    assert offsets.dtype == ids.dtype == torch.int32
    assert counts == [len(row) for row in rows]
    assert offsets.tolist() == [sum(counts[:r]) for r in range(len(rows) + 1)]
    assert ids.tolist() == [v for row in rows for v in row]
    scored = scoring.pack_targets(rows)
    assert torch.equal(scored[0], offsets) and torch.equal(scored[1], ids) and scored[2] == counts
    queries = [row for row in rows if row]  # (a query has at least one symbol)
    got = search.pack_queries(queries, 5, 0)
    want = alignment.pack_targets(queries)
    assert len(got) == 2 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].dtype == got[1].dtype == torch.int32


CALLS = {
    "greedy": (lambda e: greedy_ctc_decode(e, torch.tensor([4, 4])), "decodes"),
    "beam": (lambda e: beam_ctc_decode(e, None, 4), "decodes"),
    "align": (lambda e: alignment.ctc_forced_align(e, None, [[1], [2]]), "aligns"),
    "score": (lambda e: scoring.ctc_score(e, None, [[1], [2]]), "scores"),
    "search": (lambda e: search.ctc_search(e, None, [[1]]), "searches"),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_each_call_keeps_its_messages(name):
    call, verb = CALLS[name]
    with pytest.raises(RuntimeError) as cpu:
        call(torch.zeros(2, 4, 3))
    assert str(cpu.value) == (f"allophant_amd {verb} on an MI355X only (log_emissions must be a cuda tensor); "
                              "there is no CPU fallback")
    with pytest.raises(ValueError) as flat:
        call(torch.zeros(4, 3))
    assert str(flat.value) == "log_emissions must be [N, T, C]"
