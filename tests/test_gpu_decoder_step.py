"""GPU parity of incremental decoding (QGEMM_DECODER_KV_CACHE, qgemm_decoder_begin, qgemm_decoder_step) against
tests/causal_oracle.decoder_expected and against Decoder(causal=True).forward on the GPU, bit for bit: the stacked
outputs of the steps are the rows of the causal forward on the whole sequence.  Every step writes into a NaN-filled
output."""
import ctypes

import numpy as np
import pytest
import torch

import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

FUSED, FALLBACK = causal_oracle.DECODER_FUSED, causal_oracle.DECODER_FALLBACK
INVALID = 1


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _decoder(qg, shape, kv_cache=True, max_seq=None, max_enc_seq=None):
    seq, enc_seq, d, H, dff, blocks = shape
    return qg.Decoder(d, H, dff, blocks, max_seq=max_seq or seq, max_enc_seq=max_enc_seq or enc_seq,
                      seed=causal_oracle.DECODER_SEED, causal=True, kv_cache=kv_cache)


def _steps(dec, Xd, sizes, device, pos=0):
    """step() over consecutive row groups of Xd starting at `pos`; the stacked outputs."""
    outs = []
    for n in sizes:
        Y = _nan((n, Xd.shape[1]), device)
        assert dec.step(Xd[pos:pos + n], Y=Y) is Y
        outs.append(Y)
        pos += n
        assert dec.filled == pos
    return torch.cat(outs).cpu().numpy()


def _forward(dec, X, enc, device):
    Y = _nan(X.shape, device)
    dec.forward(_dev(X, device), _dev(enc, device), Y=Y)
    return Y.cpu().numpy()


@pytest.mark.parametrize("sizes", [(1,) * 40, (17, 3, 1, 8, 3, 8)], ids=["40x1", "17+3+1+8+3+8"])
def test_steps_stack_to_the_causal_forward(qg, oracle, device, sizes):
    X, enc = causal_oracle.decoder_inputs(FUSED)
    assert sum(sizes) == X.shape[0]
    dec, ref = _decoder(qg, FUSED), _decoder(qg, FUSED, kv_cache=False)
    try:
        dec.begin(_dev(enc, device))
        got = _steps(dec, _dev(X, device), sizes, device)
        fwd = _forward(ref, X, enc, device)
    finally:
        dec.close()
        ref.close()
    assert_bits_equal(got, causal_oracle.decoder_expected(FUSED), f"steps {sizes} against the oracle")
    assert_bits_equal(got, fwd, f"steps {sizes} against Decoder(causal=True).forward")


def test_steps_across_512_keys(qg, oracle, device):
    """DECODER_FALLBACK: one step of 500 rows (the fused launch), then 13 steps of one row whose key count goes from
    501 to 513 -- past the fused envelope, where forward runs the three launches."""
    X, enc = causal_oracle.decoder_inputs(FALLBACK)
    d, H = FALLBACK[2], FALLBACK[3]
    assert qg.attention_plan(1, 513, H, d // H).startswith("attention_decode")
    assert qg.attention_plan(513, 513, H, d // H).startswith("three_launches")
    dec, ref = _decoder(qg, FALLBACK), _decoder(qg, FALLBACK, kv_cache=False)
    try:
        dec.begin(_dev(enc, device))
        got = _steps(dec, _dev(X, device), (500,) + (1,) * 13, device)
        fwd = _forward(ref, X, enc, device)
    finally:
        dec.close()
        ref.close()
    assert_bits_equal(got, causal_oracle.decoder_expected(FALLBACK), "steps 500 + 13 x 1 against the oracle")
    assert_bits_equal(got, fwd, "steps 500 + 13 x 1 against Decoder(causal=True).forward")


def test_rewind_to_an_earlier_position(qg, oracle, device):
    """30 rows, then back to pos = 20 with different rows: the forward of the altered prefix, rows 20 .."""
    X, enc = causal_oracle.decoder_inputs(FUSED)
    alt = X.copy()
    alt[20:] = O.uniform((20, FUSED[2]), 401)
    dec, ref = _decoder(qg, FUSED), _decoder(qg, FUSED, kv_cache=False)
    try:
        dec.begin(_dev(enc, device))
        _steps(dec, _dev(X, device), (30,), device)
        Y = _nan((5, FUSED[2]), device)
        dec.step(_dev(alt[20:25], device), pos=20, Y=Y)
        assert dec.filled == 25
        tail = _steps(dec, _dev(alt, device), (1,) * 15, device, pos=25)
        fwd = _forward(ref, alt, enc, device)
    finally:
        dec.close()
        ref.close()
    assert (bits(fwd[20:]) != bits(causal_oracle.decoder_expected(FUSED)[20:])).any(axis=1).all()
    assert_bits_equal(Y.cpu().numpy(), fwd[20:25], "the rewound step")
    assert_bits_equal(tail, fwd[25:], "the steps after the rewind")


def test_second_begin_with_a_shorter_enc_out_and_stale_caches(qg, oracle, device):
    """A first sequence fills every cache row (with NaN-producing inputs: both caches end up non-finite), then begin
    with a shorter enc_out and fewer steps: nothing of the first sequence leaks."""
    X, enc = causal_oracle.decoder_inputs(FUSED)
    seq, enc_seq, d = FUSED[:3]
    dec = _decoder(qg, FUSED, max_seq=64, max_enc_seq=50)
    try:
        bad = torch.full((64, d), float("nan"), device=device)
        dec.begin(torch.full((50, d), float("nan"), device=device))
        poisoned = dec.step(bad)
        assert bool(torch.isnan(poisoned).all()), "the poisoning sequence did not reach the caches"
        dec.begin(_dev(enc, device))
        assert dec.filled == 0
        got = _steps(dec, _dev(X, device), (8,) * 5, device)
        # a shorter enc_out on the same object
        dec.begin(_dev(enc[:20], device))
        short = _steps(dec, _dev(X, device), (1,) * 12, device)
    finally:
        dec.close()
    assert_bits_equal(got, causal_oracle.decoder_expected(FUSED), "after a poisoned first sequence")
    want = causal_oracle.decoder_forward_causal_ref(X[:12], enc[:20], *FUSED[2:], causal_oracle.DECODER_SEED)
    assert (bits(want) != bits(causal_oracle.decoder_expected(FUSED)[:12])).any()
    assert_bits_equal(short, want, "a second begin with 20 rows of enc_out")


def test_forward_between_two_steps_changes_nothing(qg, oracle, device):
    X, enc = causal_oracle.decoder_inputs(FUSED)
    other = O.uniform(X.shape, 409)
    dec = _decoder(qg, FUSED)
    try:
        dec.begin(_dev(enc, device))
        Xd = _dev(X, device)
        a = _steps(dec, Xd, (17, 1), device)
        fwd = _forward(dec, other, enc[:9], device)      # the cached decoder's own forward, on other inputs
        b = _steps(dec, Xd, (1,) * 22, device, pos=18)
    finally:
        dec.close()
    want_fwd = causal_oracle.decoder_forward_causal_ref(other, enc[:9], *FUSED[2:], causal_oracle.DECODER_SEED)
    assert_bits_equal(fwd, want_fwd, "forward on a cached decoder")
    assert_bits_equal(np.concatenate([a, b]), causal_oracle.decoder_expected(FUSED), "steps around a forward")


def test_graph_capture_of_one_step(qg, oracle, device):
    """begin and step allocate nothing and do not synchronize: the step at pos = 20 is captured once and replayed with
    new input rows (a graph replays one position)."""
    X, enc = causal_oracle.decoder_inputs(FUSED)
    d = FUSED[2]
    L = qg.load()
    dec, ref = _decoder(qg, FUSED), _decoder(qg, FUSED, kv_cache=False)
    try:
        xs, y = torch.zeros((1, d), device=device), _nan((1, d), device)
        Xd, Ed = _dev(X, device), _dev(enc, device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            dec.begin(Ed)
            dec.step(Xd[:20])
            dec.step(xs, pos=20, Y=y)          # warm-up of the captured call
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_step(dec._h, xs.data_ptr(), y.data_ptr(), 20, 1, s.cuda_stream)
                assert rc == 0
        for i in range(3):
            row = O.uniform((1, d), 421 + i)
            xs.copy_(_dev(row, device))
            y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            alt = np.concatenate([X[:20], row])
            assert_bits_equal(y.cpu().numpy(), _forward(ref, alt, enc, device)[20:], f"step graph replay {i}")
    finally:
        dec.close()
        ref.close()


def test_two_cached_decoders_on_two_streams(qg, oracle, device):
    X, enc = causal_oracle.decoder_inputs(FUSED)
    X2 = O.uniform(X.shape, 431)
    decs = [_decoder(qg, FUSED), _decoder(qg, FUSED)]
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    ins = [_dev(X, device), _dev(X2, device)]
    Ed = _dev(enc, device)
    outs = [_nan(X.shape, device), _nan(X.shape, device)]
    torch.cuda.synchronize()
    try:
        for dec, s in zip(decs, streams):
            with torch.cuda.stream(s):
                dec.begin(Ed)
        for p in range(0, 40, 4):   # interleaved enqueues, no synchronize between
            for dec, s, Xd, Yd in zip(decs, streams, ins, outs):
                with torch.cuda.stream(s):
                    dec.step(Xd[p:p + 4], Y=Yd[p:p + 4])
        torch.cuda.synchronize()
    finally:
        for dec in decs:
            dec.close()
    assert_bits_equal(outs[0].cpu().numpy(), causal_oracle.decoder_expected(FUSED), "stream 0")
    want2 = causal_oracle.decoder_forward_causal_ref(X2, enc, *FUSED[2:], causal_oracle.DECODER_SEED)
    assert_bits_equal(outs[1].cpu().numpy(), want2, "stream 1")


def test_begin_and_step_argument_checks(qg, oracle, device):
    """Every refused call returns hipErrorInvalidValue before any launch: the output stays NaN and the filled length
    does not move."""
    X, enc = causal_oracle.decoder_inputs(FUSED)
    seq, enc_seq, d = FUSED[:3]
    L = qg.load()
    Xd, Ed, Y = _dev(X, device), _dev(enc, device), _nan(X.shape, device)
    st = torch.cuda.current_stream(device).cuda_stream

    def begin(h, e=Ed.data_ptr(), n=enc_seq):
        return L.qgemm_decoder_begin(h, e, n, st)

    def step(h, x=Xd.data_ptr(), y=Y.data_ptr(), pos=0, n=1):
        return L.qgemm_decoder_step(h, x, y, pos, n, st)

    plain = _decoder(qg, FUSED, kv_cache=False)
    dec = _decoder(qg, FUSED)
    try:
        assert begin(plain._h) == INVALID and step(plain._h) == INVALID      # no cache flag
        assert step(dec._h) == INVALID                                        # no begin
        assert begin(dec._h, e=None) == INVALID
        assert begin(dec._h, n=0) == INVALID and begin(dec._h, n=enc_seq + 1) == INVALID
        assert step(dec._h) == INVALID                                        # the refused begins began nothing
        assert begin(dec._h) == 0
        assert step(dec._h, x=None) == INVALID and step(dec._h, y=None) == INVALID
        assert step(dec._h, n=0) == INVALID and step(dec._h, n=-1) == INVALID
        assert step(dec._h, pos=-1) == INVALID
        assert step(dec._h, pos=1) == INVALID                                 # pos > filled (0)
        assert step(dec._h, n=seq + 1) == INVALID                             # pos + n > max_seq
        assert step(dec._h, pos=0, n=2 ** 31 - 1) == INVALID
        assert step(dec._h, n=10) == 0                                        # filled = 10
        assert step(dec._h, pos=11) == INVALID
        assert step(dec._h, pos=10, n=seq - 9) == INVALID
        assert step(dec._h, pos=10, n=seq - 10) == 0                          # up to max_seq exactly
        assert step(dec._h, pos=seq, n=1) == INVALID
        torch.cuda.synchronize()
        with pytest.raises(qg.QGemmError):
            qg.Decoder(d, FUSED[3], FUSED[4], 1, seq, enc_seq, causal=False, kv_cache=True)
        rc = L.qgemm_decoder_create_ex(d, FUSED[3], FUSED[4], 1, seq, enc_seq, 1, qg.QGEMM_DECODER_KV_CACHE | 16 |
                                       qg.QGEMM_DECODER_CAUSAL, ctypes.byref(ctypes.c_void_p()))
        assert rc == INVALID
    finally:
        plain.close()
        dec.close()
    # the two accepted steps wrote rows 0 .. 9 and then rows 0 .. seq - 11 of Y (both from Y's start), nothing else
    got = Y.cpu().numpy()
    assert np.isfinite(got[:seq - 10]).all() and np.isnan(got[seq - 10:]).all()
