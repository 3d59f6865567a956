"""GPU parity of the head object at a real vocabulary: 50257 columns (odd: every second row of the head's own logits
buffer starts off a 16-byte boundary), d_model 128, an untied weight with a bias, max_rows 64.  next_tokens takes the
split argmax -- two launches through the head's own workspace -- at every row count, and equal logits sit in different
parts of every plan (batch_cases.head_model plants them; tests/test_batch_plans_host.py shows it on the oracle alone).
Everything is compared bit for bit with oracle.linear and head_oracle.argmax_rows_ref on the CPU."""
import numpy as np
import pytest
import torch

import batch_cases as C
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


@pytest.fixture(scope="module")
def wide_head(qg, oracle, device):
    """(head, packed W, bias on the device, the 64 hidden rows on the device)"""
    W, bias = C.head_model()
    Wp, bd = qg.pack_b(_dev(W, device)), _dev(bias, device)
    head = qg.Head(Wp, C.VOCAB, bd, max_rows=C.HEAD_MAX_ROWS)
    yield head, Wp, bd, _dev(C.head_hidden(), device)
    head.close()


@pytest.mark.parametrize("rows", C.HEAD_ROWS)
def test_logits_at_a_real_vocabulary(qg, device, wide_head, rows):
    head, Wp, bd, Hd = wide_head
    want = qg.linear(Hd[:rows], Wp, bd)
    got = head.logits(Hd[:rows])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "logits() is linear(), bit for bit"
    assert_bits_equal(got.cpu().numpy(), C.head_logits()[:rows], "logits against the oracle")
    # a column window of a wider buffer: an odd row stride and a base off a 16-byte boundary
    wide = torch.full((rows, C.VOCAB + 12), float("nan"), device=device)
    head.logits(Hd[:rows], out=wide[:, 5:5 + C.VOCAB])
    assert torch.equal(wide[:, 5:5 + C.VOCAB].view(torch.int32), want.view(torch.int32))
    assert bool(torch.isnan(wide[:, :5]).all()) and bool(torch.isnan(wide[:, 5 + C.VOCAB:]).all())


@pytest.mark.parametrize("rows", C.HEAD_ROWS)
def test_next_tokens_with_ties_across_parts(qg, device, wide_head, rows):
    """The lowest of the tied columns wins, whichever parts of the row's plan hold them."""
    head, _, _, Hd = wide_head
    parts = qg.argmax_rows_plan(rows, C.VOCAB)
    assert parts > 1, "the split argmax"
    tied = [r for r in C.rows_tied_across_parts(C.head_logits(), parts) if r < rows]
    assert len(tied) >= min(rows, 8), "a test bug: the planted ties are not ties across this plan's parts"
    tok = torch.full((rows,), -1, dtype=torch.int32, device=device)
    assert head.next_tokens(Hd[:rows], tok) is tok
    got, want = tok.cpu().numpy(), C.head_tokens()[:rows]
    assert np.array_equal(got, want), f"{rows} rows: rows {np.flatnonzero(got != want)[:8]} differ: {got} vs {want}"


def test_every_row_count_fits_the_heads_workspaces(qg, device, wide_head):
    """1 .. 64 rows on one head: the argmax workspace's need is largest below max_rows (12 parts x 46 rows)."""
    head, _, _, Hd = wide_head
    assert len(C.rows_tied_across_parts(C.head_logits(), 12)) >= 8
    want = C.head_tokens()
    toks = [torch.full((rows,), -1, dtype=torch.int32, device=device) for rows in range(1, C.HEAD_MAX_ROWS + 1)]
    for rows, tok in enumerate(toks, 1):
        head.next_tokens(Hd[64 - rows:], tok)          # the LAST rows: every call starts on another row
    for rows, tok in enumerate(toks, 1):
        assert np.array_equal(tok.cpu().numpy(), want[64 - rows:]), f"{rows} rows"
    with pytest.raises(qg.QGemmError):
        head.next_tokens(torch.zeros((C.HEAD_MAX_ROWS + 1, C.D), device=device))


@pytest.mark.parametrize("vocab,max_rows", [(C.VOCAB_TWO_PARTS, 3), (C.VOCAB_MANY_PARTS, 2)])
def test_few_rows_and_many_parts(qg, oracle, device, vocab, max_rows):
    """vocab 8195 with 3 rows: a two-part plan behind the 32-tile GEMM.  vocab 262147 with 2 rows: more than 32 parts,
    so the combine kernel's upper half-wave holds real candidates -- and a winner."""
    W, bias, H, logits, tokens = C.small_head(vocab, max_rows)
    parts = qg.argmax_rows_plan(1, vocab)
    if vocab == C.VOCAB_MANY_PARTS:
        assert parts > 32 and max(int(t) // C.argmax_chunk(vocab, parts) for t in tokens) >= 32
    else:
        assert [qg.argmax_rows_plan(r, vocab) for r in (1, 2, 3)] == [2, 2, 2]
    Hd = _dev(H, device)
    head = qg.Head(qg.pack_b(_dev(W, device)), vocab, _dev(bias, device), max_rows=max_rows)
    try:
        for rows in range(1, max_rows + 1):
            assert_bits_equal(head.logits(Hd[:rows]).cpu().numpy(), logits[:rows], f"vocab {vocab}, {rows} rows: logits")
            tok = torch.full((rows,), -1, dtype=torch.int32, device=device)
            head.next_tokens(Hd[:rows], tok)
            assert np.array_equal(tok.cpu().numpy(), tokens[:rows]), f"vocab {vocab}, {rows} rows"
            assert np.array_equal(head.next_tokens(Hd[rows - 1:rows]).cpu().numpy(), tokens[rows - 1:rows])
    finally:
        head.close()
