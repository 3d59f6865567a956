"""GPU parity of Encoder.forward_batch (qgemm_encoder_forward_batch): the rows of every sequence of a batch against
attn_oracle.encoder_forward_ref on that sequence alone, on the CPU, and against Encoder.forward on it, on the GPU, bit
for bit.  Every call writes into a NaN-filled output.  Dimensions: d_model 64, 2 heads, d_ff 128, 2 blocks unless a
test says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

import attn_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

DIMS = (64, 2, 128, 2)
SEED = 31
INVALID = 1
LENS = (33, 1, 40, 32, 7)


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _ints(v):
    return (ctypes.c_int * max(1, len(v)))(*v)


def _rows(lens, d, seed):
    return [O.uniform((n, d), seed + b) for b, n in enumerate(lens)]


def _split(Y, lens):
    out, at = [], 0
    for n in lens:
        out.append(Y[at:at + n])
        at += n
    return out


def _check(qg, enc, seqs, device, what, dims=DIMS, cpu=True):
    """forward_batch on the sequences (numpy) into a NaN-filled output; each one against the oracle and forward."""
    lens = [s.shape[0] for s in seqs]
    X = _dev(np.concatenate(seqs), device)
    Y = _nan(X.shape, device)
    assert enc.forward_batch(X, lens, Y=Y) is Y
    got = _split(Y.cpu().numpy(), lens)
    for b, s in enumerate(seqs):
        if cpu:
            assert_bits_equal(got[b], attn_oracle.encoder_forward_ref(s, *dims, SEED), f"{what}: sequence {b} against the oracle")
        one = _nan(s.shape, device)
        enc.forward(_dev(s, device), Y=one)
        assert_bits_equal(got[b], one.cpu().numpy(), f"{what}: sequence {b} against forward")
    return got


def test_batch_of_unequal_lengths(qg, oracle, device):
    """(33, 1, 40, 32, 7): one row past a query tile, a single row, exactly one tile -- against the oracle per
    sequence and against forward per sequence on the GPU."""
    assert qg.attention_varlen_plan(LENS, LENS, DIMS[1], DIMS[0] // DIMS[1]) == "attention_fused_kernel<many>"
    enc = qg.Encoder(*DIMS, max_seq=40, seed=SEED, max_rows=sum(LENS))
    try:
        got = _check(qg, enc, _rows(LENS, DIMS[0], 400), device, "unequal lengths")
        assert all(np.isfinite(g).all() for g in got)
    finally:
        enc.close()


def test_one_sequence_equals_forward(qg, oracle, device):
    enc = qg.Encoder(*DIMS, max_seq=40, seed=SEED)
    try:
        _check(qg, enc, _rows((37,), DIMS[0], 420), device, "one sequence")
    finally:
        enc.close()


def test_a_513_row_sequence_takes_the_scores_path(qg, oracle, device):
    """d_model 16: a 513-row sequence between two short ones leaves the table launch's envelope, so the attention runs
    sequence by sequence -- fused, three launches through the stack's scores, decode."""
    dims = (16, 2, 128, 2)
    lens = (33, 513, 5)
    assert qg.attention_varlen_plan(lens, lens, dims[1], dims[0] // dims[1]) == "per_sequence"
    assert [qg.attention_plan(n, n, dims[1], 8).split("_kernel")[0] for n in lens] == \
        ["attention_fused", "three_launches", "attention_decode"]
    enc = qg.Encoder(*dims, max_seq=513, seed=SEED, max_rows=sum(lens))
    try:
        _check(qg, enc, _rows(lens, dims[0], 440), device, "513 rows", dims=dims)
    finally:
        enc.close()


def test_row_budget(qg, device):
    """sum = max_rows passes and sum = max_rows + 1 is refused; an encoder created without max_rows takes a batch of
    up to max_seq rows; max_rows below max_seq changes nothing."""
    d = DIMS[0]
    L = qg.load()

    def rc(enc, lens):
        n = sum(lens)
        X, Y = torch.rand((n, d), device=device) * 2 - 1, _nan((n, d), device)
        r = L.qgemm_encoder_forward_batch(enc._h, X.data_ptr(), Y.data_ptr(), len(lens), _ints(lens), None)
        torch.cuda.synchronize()
        return r, Y

    enc = qg.Encoder(*DIMS, max_seq=40, seed=SEED, max_rows=100)
    try:
        r, Y = rc(enc, (40, 40, 20))
        assert r == 0 and bool(torch.isfinite(Y).all())
        r, Y = rc(enc, (40, 40, 21))
        assert r == INVALID and bool(torch.isnan(Y).all()), "a refused batch launches nothing"
    finally:
        enc.close()
    for kw in (dict(), dict(max_rows=0), dict(max_rows=17)):
        enc = qg.Encoder(*DIMS, max_seq=40, seed=SEED, **kw)
        try:
            assert rc(enc, (20, 13, 7))[0] == 0, kw
            assert rc(enc, (20, 13, 8))[0] == INVALID, kw
            assert rc(enc, (40,))[0] == 0 and rc(enc, (41,))[0] == INVALID, kw
        finally:
            enc.close()


def test_graph_capture_and_replay(qg, oracle, device):
    """forward_batch allocates nothing, copies nothing to the device and does not synchronize: captured once, replayed
    with new contents of X."""
    d = DIMS[0]
    lens = (33, 1, 40)
    enc = qg.Encoder(*DIMS, max_seq=40, seed=SEED, max_rows=sum(lens))
    L = qg.load()
    try:
        X, Y = torch.zeros((sum(lens), d), device=device), _nan((sum(lens), d), device)

        def call(stream):
            assert L.qgemm_encoder_forward_batch(enc._h, X.data_ptr(), Y.data_ptr(), len(lens), _ints(lens), stream) == 0

        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            call(s.cuda_stream)      # warm-up: module load, first launches
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                call(s.cuda_stream)
        for i in range(2):
            seqs = _rows(lens, d, 460 + 10 * i)
            X.copy_(_dev(np.concatenate(seqs), device))
            Y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for b, (got, s_) in enumerate(zip(_split(Y.cpu().numpy(), lens), seqs)):
                assert_bits_equal(got, attn_oracle.encoder_forward_ref(s_, *DIMS, SEED), f"graph replay {i}, sequence {b}")
    finally:
        enc.close()


def test_every_error_case(qg, device):
    d = DIMS[0]
    L = qg.load()
    enc = qg.Encoder(*DIMS, max_seq=40, seed=SEED, max_rows=4000)
    dec = qg.Decoder(*DIMS, max_seq=40, max_enc_seq=8, seed=SEED)
    try:
        X, Y = torch.rand((4000, d), device=device) * 2 - 1, _nan((4000, d), device)
        f = L.qgemm_encoder_forward_batch
        ok = (enc._h, X.data_ptr(), Y.data_ptr(), 2, _ints((3, 4)), None)
        assert f(*ok) == 0
        torch.cuda.synchronize()
        Y.fill_(float("nan"))
        for i, v in ((0, None), (1, None), (2, None), (4, None), (3, 0), (3, -1), (3, 65), (0, dec._h)):
            bad = list(ok)
            bad[i] = v
            if i == 3 and v == 65:
                bad[4] = _ints([1] * 65)
            assert f(*bad) == INVALID, (i, v)
        for lens in ((3, 0), (0,), (-1, 4), (41,), (3, 41), [40] * 64 + [1]):
            assert f(enc._h, X.data_ptr(), Y.data_ptr(), len(lens), _ints(lens), None) == INVALID, lens
        assert f(enc._h, X.data_ptr(), Y.data_ptr(), 64, _ints([40] * 64), None) == 0      # 2560 rows, 64 sequences
        torch.cuda.synchronize()
        assert bool(torch.isfinite(Y[:2560]).all()) and bool(torch.isnan(Y[2560:]).all())
        got = Y[:2560].cpu().numpy()
        for b in (0, 31, 63):                                                              # first, middle, last
            one = _nan((40, d), device)
            enc.forward(X[40 * b:40 * b + 40], Y=one)
            assert_bits_equal(got[40 * b:40 * b + 40], one.cpu().numpy(), f"sequence {b} of 64 against forward")
        with pytest.raises(qg.QGemmError):
            qg.Encoder(*DIMS, max_seq=40, seed=SEED, max_rows=-1)
    finally:
        enc.close()
        dec.close()
