"""GPU parity of qgemm_embed_rows against head_oracle.embed_rows_ref, bit for bit: with and without a position table,
rows_per_seq 1 and 3, row-strided E, P and Y (Y NaN-filled outside its rows), d_model 1, 5 and 64, the first and the
last token, and tokens outside the vocabulary, which give rows of quiet NaNs beside untouched neighbours."""
import numpy as np
import pytest
import torch

import head_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

VOCAB, MAX_POS = 37, 11


def _strided(a, pad, device, offset=0):
    """a as a row-strided window (row stride = width + pad, `offset` floats into a NaN-filled parent)."""
    n, d = a.shape
    parent = torch.full((offset + n * (d + pad),), float("nan"), device=device)
    view = torch.as_strided(parent, (n, d), (d + pad, 1), offset)
    view.copy_(torch.from_numpy(np.array(a)).to(device))
    return parent, view


def _tables(d):
    return O.uniform((VOCAB, d), 811 + d), O.uniform((MAX_POS, d), 812 + d)


@pytest.mark.parametrize("d", [1, 5, 64])
@pytest.mark.parametrize("rows_per_seq", [1, 3])
@pytest.mark.parametrize("with_p", [False, True])
def test_gather(qg, oracle, device, d, rows_per_seq, with_p):
    E, P = _tables(d)
    n_seqs = 4
    pos = [0, MAX_POS - rows_per_seq, 3, 5]
    tokens = np.array(([0, VOCAB - 1, 7, VOCAB - 1, 0, 20, 7, 7, 1, 36, 35, 2])[:n_seqs * rows_per_seq], np.int32)
    want = head_oracle.embed_rows_ref(E, tokens, P if with_p else None, pos, rows_per_seq)
    tok_d = torch.from_numpy(tokens).to(device)
    # contiguous tables (16-byte rows where d allows) and a contiguous output
    got = qg.embed_rows(torch.from_numpy(E).to(device), tok_d, torch.from_numpy(P).to(device) if with_p else None,
                        pos if with_p else None, rows_per_seq)
    assert_bits_equal(got.cpu().numpy(), want, "contiguous")
    # row-strided views of E, P and Y; Y stays NaN outside its rows
    for pad, offset in ((4, 0), (3, 1)):
        _, Ev = _strided(E, pad, device, offset)
        _, Pv = _strided(P, pad + 4, device, offset)
        Yp, Yv = _strided(np.full(want.shape, np.nan, np.float32), pad, device, offset)
        out = qg.embed_rows(Ev, tok_d, Pv if with_p else None, pos if with_p else None, rows_per_seq, Y=Yv)
        assert out is Yv
        assert_bits_equal(Yv.cpu().numpy(), want, f"strided, pad {pad}")
        mask = torch.ones_like(Yp, dtype=torch.bool)
        torch.as_strided(mask, Yv.shape, Yv.stride(), offset).fill_(False)
        assert torch.isnan(Yp[mask]).all(), "Y was written outside its rows"


@pytest.mark.parametrize("d", [5, 64])
@pytest.mark.parametrize("with_p", [False, True])
def test_tokens_outside_the_vocabulary(qg, oracle, device, d, with_p):
    E, P = _tables(d)
    tokens = np.array([3, -1, 4, VOCAB, 5, 2 ** 31 - 1, -2 ** 31, 6], np.int32)
    pos = [2] * 8
    want = head_oracle.embed_rows_ref(E, tokens, P if with_p else None, pos)
    got = qg.embed_rows(torch.from_numpy(E).to(device), torch.from_numpy(tokens).to(device),
                        torch.from_numpy(P).to(device) if with_p else None, pos if with_p else None).cpu().numpy()
    bad = [1, 3, 5, 6]
    assert (got[bad].view(np.uint32) == head_oracle.QUIET_NAN).all(), "the exact quiet-NaN pattern"
    good = [0, 2, 4, 7]
    assert_bits_equal(got[good], want[good], "the neighbouring rows")


def test_refusals(qg, oracle, device):
    d = 5
    E, P = _tables(d)
    Ed, Pd = torch.from_numpy(E).to(device), torch.from_numpy(P).to(device)
    tok = torch.zeros(6, dtype=torch.int32, device=device)
    Y = torch.full((6, d), float("nan"), device=device)
    for pos, rps in (([MAX_POS] * 6, 1), ([0, MAX_POS - 2], 3), ([-1] * 6, 1)):
        with pytest.raises(qg.QGemmError) as e:
            qg.embed_rows(Ed, tok, Pd, pos, rps, Y=Y)
        assert e.value.code == qg.HIP_ERROR_INVALID_VALUE
    assert qg.embed_rows(Ed, tok, Pd, [MAX_POS - 1] * 6, 1, Y=Y) is Y       # the last position is fine
    torch.cuda.synchronize()
    Y.fill_(float("nan"))
    L = qg.load()
    assert L.qgemm_embed_rows(Ed.data_ptr(), d, VOCAB, d, tok.data_ptr(), Pd.data_ptr(), d, MAX_POS, None, 6, 1,
                              Y.data_ptr(), d, None) == 1                    # a position table without pos
    assert L.qgemm_embed_rows(Ed.data_ptr(), d - 1, VOCAB, d, tok.data_ptr(), None, 0, 0, None, 6, 1, Y.data_ptr(), d,
                              None) == 1                                     # a row stride below d_model
    assert L.qgemm_embed_rows(Ed.data_ptr(), d, VOCAB, d, tok.data_ptr(), None, 0, 0, None, 0, 1, Y.data_ptr(), d,
                              None) == 0                                     # no sequences: nothing to do
    torch.cuda.synchronize()
    assert torch.isnan(Y).all()
