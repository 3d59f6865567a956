"""GPU parity of the decoder counterpart (transformer.cu:79-168 with quantized linears) against
tests/attn_oracle.decoder_forward_ref, bit for bit: shapes, lengths and limits, then every combination of the two
attention paths, split-K inside the object, zero rows, graph capture and replay of a forward, two streams."""
import numpy as np
import pytest
import torch

import attn_cases
import attn_oracle
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("seq,enc_seq,d,H,dff,blocks", [
    (6, 6, 8, 4, 8, 2),            # the reference main()'s shape
    (33, 100, 64, 2, 96, 2),       # tails in both sequence lengths
    (100, 40, 128, 4, 256, 1),     # enc_seq < seq
    (8, 520, 32, 2, 32, 1),        # cross-attention on the three-launch fallback (self-attention fused)
])
def test_decoder_forward_bit_exact(qg, oracle, device, seq, enc_seq, d, H, dff, blocks):
    X, enc = oracle.uniform((seq, d), 11), oracle.uniform((enc_seq, d), 12)
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=13)
    try:
        Y = dec.forward(_dev(X, device), _dev(enc, device))
        torch.cuda.synchronize()
        want = attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 13)
        assert_bits_equal(Y.cpu().numpy(), want,
                          f"decoder seq={seq} enc_seq={enc_seq} d={d} H={H} dff={dff} blocks={blocks}")
    finally:
        dec.close()


def test_decoder_second_forward_with_smaller_lengths(qg, oracle, device):
    """A second forward on the same object with a smaller seq and enc_seq: nothing of the first call (buffers,
    packed activations, split-K tickets) leaks into it; then the first shape again."""
    d, H, dff, blocks = 64, 2, 96, 2
    dec = qg.Decoder(d, H, dff, blocks, max_seq=33, max_enc_seq=100, seed=17)
    try:
        for seq, enc_seq in [(33, 100), (7, 21), (33, 100)]:
            X, enc = oracle.uniform((seq, d), 19), oracle.uniform((enc_seq, d), 20)
            Y = dec.forward(_dev(X, device), _dev(enc, device)).cpu().numpy()
            assert_bits_equal(Y, attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 17),
                              f"decoder forward seq={seq} enc_seq={enc_seq} on a max_seq 33 / 100 object")
    finally:
        dec.close()


def test_decoder_rejects_lengths_past_its_limits(qg, device):
    dec = qg.Decoder(8, 4, 8, 1, max_seq=6, max_enc_seq=5, seed=1)
    try:
        ok = torch.zeros((6, 8), device=device)
        for seq, enc_seq in [(7, 5), (6, 6)]:
            with pytest.raises(qg.QGemmError) as ei:
                dec.forward(torch.zeros((seq, 8), device=device), torch.zeros((enc_seq, 8), device=device))
            assert ei.value.code == qg.HIP_ERROR_INVALID_VALUE
        with pytest.raises(qg.QGemmError):
            dec.forward(ok, torch.zeros((0, 8), device=device))
    finally:
        dec.close()


# ---- attention paths, split-K, zero rows, graph replay and streams.  Every output is pre-filled with NaN ----

def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _plan(qg, m, n, k):
    import ctypes
    tile = ctypes.c_int(0)
    splits = qg.load().qgemm_gemm_plan(m, n, k, ctypes.byref(tile), None)
    return tile.value, splits


def _fused(qg, seq_q, seq_kv, H, dk):
    return qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == 0


@pytest.mark.parametrize("seq,enc_seq,d,H,dff,blocks,self_fused,cross_fused", [
    (516, 20, 16, 2, 32, 1, False, True),     # self-attention on the fallback, cross-attention fused
    (600, 600, 32, 2, 32, 1, False, False),   # both on the fallback: they share the object's scores
    # d_k 65: both fall back by width; d % 4 != 0: the general (LDS-walking) layernorm-with-pack kernel at all three
    # places of the block
    (20, 30, 130, 2, 64, 1, False, False),
])
def test_decoder_attention_paths_bit_exact(qg, oracle, device, seq, enc_seq, d, H, dff, blocks, self_fused,
                                           cross_fused):
    """The combinations of launch_attention's two paths that test_decoder_forward_bit_exact leaves out, and d_k > 64
    with d % 4 != 0 inside a decoder block."""
    assert _fused(qg, seq, seq, H, d // H) == self_fused and _fused(qg, seq, enc_seq, H, d // H) == cross_fused
    X, enc = oracle.uniform((seq, d), 23), oracle.uniform((enc_seq, d), 24)
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=25)
    try:
        Y = _nan((seq, d), device)
        dec.forward(_dev(X, device), _dev(enc, device), Y=Y)
        got = Y.cpu().numpy()
    finally:
        dec.close()
    assert_bits_equal(got, attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 25),
                      f"decoder seq={seq} enc_seq={enc_seq} d={d} H={H}")


SPLIT = (33, 100, 64, 2, 4096, 2)   # (seq, enc_seq, d, H, d_ff, blocks): FFN-down 33 x 64 x 4096 plans 2 splits


def test_decoder_split_k_inside_the_object(qg, oracle, device):
    """The split-K FFN-down runs on a scratch that the [K2 | V2] projection and every other linear are handed too,
    with tickets_zeroed = true: two blocks per forward, three forwards (A, B, A) on one object, every one bit-exact."""
    seq, enc_seq, d, H, dff, blocks = SPLIT
    assert _plan(qg, seq, d, dff) == (64, 2)
    ins = [(oracle.uniform((seq, d), 27 + i), oracle.uniform((enc_seq, d), 29 + i)) for i in range(2)]
    want = [attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 31) for X, enc in ins]
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=31)
    try:
        for i, which in enumerate((0, 1, 0)):
            Y = _nan((seq, d), device)
            dec.forward(_dev(ins[which][0], device), _dev(ins[which][1], device), Y=Y)
            assert_bits_equal(Y.cpu().numpy(), want[which], f"decoder with a split-K FFN-down, forward {i}")
    finally:
        dec.close()


def test_decoder_zero_rows(qg, oracle, device):
    """Row 3 of X and row 7 of enc_out all zero: absmax 0, scale inf, 0 * inf -> NaN -> 0 in the pack -- in the block
    input's pack and in the one-time quantization of enc_out that serves both blocks."""
    seq, enc_seq, d, H, dff, blocks = 33, 100, 64, 2, 96, 2
    X, enc = attn_cases.zero_row_decoder_inputs(seq, enc_seq, d)
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=13)
    try:
        Y = _nan((seq, d), device)
        dec.forward(_dev(X, device), _dev(enc, device), Y=Y)
        got = Y.cpu().numpy()
    finally:
        dec.close()
    assert_bits_equal(got, attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 13), "decoder, zero rows")


@pytest.mark.parametrize("seq,enc_seq,d,H,dff,blocks", [SPLIT, (8, 520, 32, 2, 32, 1)],
                         ids=["split_k", "cross_fallback"])
def test_decoder_forward_graph_capture_and_replay(qg, oracle, device, seq, enc_seq, d, H, dff, blocks):
    """Decoder.forward allocates nothing and does not synchronize: after a warm-up on the side stream one forward is
    captured into static X / enc_out / Y and replayed three times with a new X AND a new enc_out -- the packed enc_out
    is rebuilt by the replay, not remembered from the capture; on the split shape every replay finds the tickets
    zero."""
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=37)
    try:
        Xs, Es = torch.zeros((seq, d), device=device), torch.zeros((enc_seq, d), device=device)
        Y = _nan((seq, d), device)
        Xs.copy_(_dev(oracle.uniform((seq, d), 38), device))
        Es.copy_(_dev(oracle.uniform((enc_seq, d), 39), device))
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            dec.forward(Xs, Es, Y=Y)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                dec.forward(Xs, Es, Y=Y)
        for i in range(3):
            X, enc = oracle.uniform((seq, d), 41 + 2 * i), oracle.uniform((enc_seq, d), 42 + 2 * i)
            Xs.copy_(_dev(X, device))
            Es.copy_(_dev(enc, device))
            Y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_bits_equal(Y.cpu().numpy(), attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 37),
                              f"decoder graph replay {i}, enc_seq={enc_seq}")
    finally:
        torch.cuda.synchronize()
        dec.close()


def test_decoder_and_encoder_on_two_streams(qg, oracle, device):
    """One Decoder and one Encoder forward at the same time on two streams, five rounds each with different inputs,
    one synchronize at the end: the two objects share nothing."""
    seq, enc_seq, d, H, dff, blocks = 33, 100, 64, 2, 96, 2
    eseq, ed, eH, edff, eblocks = 100, 256, 8, 512, 2
    dec = enc = None
    try:
        dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=43)
        enc = qg.Encoder(ed, eH, edff, eblocks, max_seq=eseq, seed=47)
        drounds, erounds = [], []
        for r in range(5):
            X, E = oracle.uniform((seq, d), 51 + 2 * r), oracle.uniform((enc_seq, d), 52 + 2 * r)
            drounds.append((_dev(X, device), _dev(E, device), _nan((seq, d), device),
                            attn_oracle.decoder_forward_ref(X, E, d, H, dff, blocks, 43)))
            X = oracle.uniform((eseq, ed), 71 + r)
            erounds.append((_dev(X, device), _nan((eseq, ed), device),
                            oracle.encoder_forward(X, ed, eH, edff, eblocks, 47)))
        sd, se = torch.cuda.Stream(device), torch.cuda.Stream(device)
        torch.cuda.synchronize()
        for r in range(5):
            with torch.cuda.stream(sd):
                dec.forward(drounds[r][0], drounds[r][1], Y=drounds[r][2])
            with torch.cuda.stream(se):
                enc.forward(erounds[r][0], Y=erounds[r][1])
        torch.cuda.synchronize()
        for r in range(5):
            assert_bits_equal(drounds[r][2].cpu().numpy(), drounds[r][3], f"decoder on its stream, round {r}")
            assert_bits_equal(erounds[r][1].cpu().numpy(), erounds[r][2], f"encoder on its stream, round {r}")
    finally:
        torch.cuda.synchronize()
        for obj in (dec, enc):
            if obj is not None:
                obj.close()


def test_encoder_and_decoder_handles_are_not_interchangeable(qg, oracle, device):
    """Encoder and decoder handles are the same kind of object inside the library (a stack of blocks without / with
    cross-attention).  Through the raw entry points: qgemm_decoder_forward / _begin / _step on an encoder's handle and
    qgemm_encoder_forward on a decoder's return the invalid-value code and write nothing; the matching calls still work
    on the same handles afterwards.  The decoder has its caches, so begin and step are refused for the handle alone."""
    d, H, dff, blocks, seq = 32, 2, 32, 1, 8
    L = qg.load()
    enc = qg.Encoder(d, H, dff, blocks, max_seq=seq, seed=61)
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=seq, seed=61, causal=True, kv_cache=True)
    try:
        X, E = _dev(oracle.uniform((seq, d), 62), device), _dev(oracle.uniform((seq, d), 63), device)
        Y = torch.full((seq, d), -7.25, device=device)
        stream = qg._stream(device)
        refused = [
            ("decoder_forward on an encoder",
             lambda: L.qgemm_decoder_forward(enc._h, X.data_ptr(), E.data_ptr(), Y.data_ptr(), seq, seq, stream)),
            ("decoder_begin on an encoder", lambda: L.qgemm_decoder_begin(enc._h, E.data_ptr(), seq, stream)),
            ("decoder_step on an encoder",
             lambda: L.qgemm_decoder_step(enc._h, X.data_ptr(), Y.data_ptr(), 0, 1, stream)),
            ("encoder_forward on a decoder",
             lambda: L.qgemm_encoder_forward(dec._h, X.data_ptr(), Y.data_ptr(), seq, stream)),
        ]
        for what, call in refused:
            assert call() == qg.HIP_ERROR_INVALID_VALUE, what
            torch.cuda.synchronize()
            assert bool((Y == -7.25).all()), f"{what} wrote to Y"
        assert_bits_equal(enc.forward(X).cpu().numpy(),
                          oracle.encoder_forward(oracle.uniform((seq, d), 62), d, H, dff, blocks, 61),
                          "encoder forward after the refused calls")
        full = dec.forward(X, E)
        dec.begin(E)
        rows = torch.cat([dec.step(X[:5]), dec.step(X[5:])])
        assert torch.equal(rows.view(torch.int32), full.view(torch.int32)), "decoder begin + steps after the refusals"
    finally:
        enc.close()
        dec.close()
