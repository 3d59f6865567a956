"""A Llama-shaped stack at d_k 128 on the batched and generating calls: decoder-only, pre-LN + final
norm, RoPE, RMSNorm, SwiGLU; d_model 256, 2 heads, d_ff 64, 2 blocks, 3 cache slots (6 for the beam search: a slot per
beam and per prompt).  Every result is held to tests/gated_oracle.py's chain on the RoPE tables read back from the
model, never to the GPU's own forward.  Before the wide decode kernel every call here returned hipErrorInvalidValue."""
import ctypes

import numpy as np
import pytest
import torch

import beam_oracle
import gated_oracle as GO
import head_oracle
import prenorm_oracle as PO
import standard_oracle as SO
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

D, H, DFF, BLOCKS, MAX_SEQ, VOCAB = 256, 2, 64, 2, 140, 50
POS = (0, 127, 130)     # step_batch: key counts 1, 128 and 131, both sides of the kernel's 128-key chunk
BETAS = (SO.BE1, SO.BE2, SO.BE3, PO.BEF)


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _weights():
    return GO.gated_weights(D, H, DFF, BLOCKS, 23, cross=False)


def _rows(seed):
    return O.uniform((MAX_SEQ, D), seed)


def _make(qg, device, n_slots=3):
    m = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, seed=404, causal=True, kv_cache=True, decoder_only=True,
                   arch="standard", activation="silu", norm_first=True, final_norm=True, rope=True, norm="rms",
                   gated_ffn=True, n_slots=n_slots)
    assert qg.attention_plan(1, MAX_SEQ, H, D // H) == "attention_decode_wide_kernel"
    for (block, kind), a in _weights().items():
        if kind not in BETAS:
            m.set_weight(block, kind, _dev(a, device))
    return m, tuple(t.cpu().numpy() for t in m.rope_tables())


def _head(qg, device):
    """the head and its tables (E, P, W, bias)"""
    E, P, W, bias = (O.uniform((VOCAB, D), 601), O.uniform((MAX_SEQ, D), 602, -0.1, 0.1), O.uniform((D, VOCAB), 603),
                     O.uniform((VOCAB,), 604, -0.05, 0.05))
    head = qg.Head(qg.pack_b(_dev(W, device)), VOCAB, _dev(bias, device), _dev(E, device), _dev(P, device), max_rows=8)
    return head, (E, P, W, bias)


def _chain(tables):
    return lambda X, enc=None: GO.forward(X, None, _weights(), D, H, BLOCKS, GO.LLAMA, True, "silu", 1e-5, None, tables)


def _prefill(m, device, slots, pre, seed0):
    for b, n in enumerate(pre):
        m.begin_slot(slots[b])
        if n:
            m.step_slot(slots[b], _dev(_rows(seed0 + b)[:n], device))


def test_step_batch_eager_and_captured(qg, oracle, device):
    """each row is the oracle's causal forward on its sequence's prefix: the eager call and two replays of its capture"""
    m, tables = _make(qg, device)
    try:
        _prefill(m, device, (0, 1, 2), POS, 40)
        new = torch.cat([_dev(_rows(40 + b)[p:p + 1], device) for b, p in enumerate(POS)])
        Y = torch.full((3, D), float("nan"), device=device)
        slots, at = (ctypes.c_int * 3)(0, 1, 2), (ctypes.c_int * 3)(*POS)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        got = []
        with torch.cuda.stream(s):
            step = lambda: qg.load().qgemm_decoder_step_batch(m._h, 3, slots, at, 1, new.data_ptr(), Y.data_ptr(),  # noqa: E731
                                                              s.cuda_stream)
            assert step() == 0   # eager, and the warm-up
            s.synchronize()
            got.append(Y.cpu().numpy())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                assert step() == 0
        for _ in range(2):
            Y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got.append(Y.cpu().numpy())
    finally:
        m.close()
    fwd = _chain(tables)
    for b, p in enumerate(POS):
        want = fwd(_rows(40 + b)[:p + 1])[-1:]
        for i, y in enumerate(got):
            assert_bits_equal(y[b:b + 1], want, f"slot {b} at position {p}, {'eager' if i == 0 else f'replay {i}'}")


def test_generate(qg, oracle, device):
    pre, tin, n_new = (4, 0, 126), (7, 28, 49), 4   # slot 2 crosses the chunk edge while it generates
    m, tables = _make(qg, device)
    head, (E, P, Wh, bias) = _head(qg, device)
    try:
        _prefill(m, device, (0, 1, 2), pre, 60)
        out = torch.full((n_new, 3), -7, dtype=torch.int32, device=device)
        m.generate(head, [0, 1, 2], torch.tensor(tin, dtype=torch.int32, device=device), n_new, tokens_out=out)
        got = out.cpu().numpy()
    finally:
        head.close()
        m.close()
    want = np.array([head_oracle.generate_ref(_rows(60 + b)[:pre[b]], None, tin[b], n_new, E, Wh, bias, P,
                                              (D, H, DFF, BLOCKS), None, forward=_chain(tables)) for b in range(3)],
                    np.int32).T
    assert np.array_equal(got, want), f"generate against generate_ref\n{got}\n{want}"


def test_generate_beam_indirect(qg, oracle, device):
    beams, pre, tin, n_new = 2, (3, 127), (5, 31), 4
    slots, src = [0, 1, 2, 3], [4, 5]
    m, tables = _make(qg, device, n_slots=6)
    head, (E, P, Wh, bias) = _head(qg, device)
    try:
        _prefill(m, device, src, pre, 80)
        m.beam_begin(slots, src, None, beams)
        tokens = torch.tensor(np.repeat(tin, beams), dtype=torch.int32, device=device)
        got = tuple(t.cpu().numpy() for t in m.generate_beam_indirect(head, slots, src, tokens, n_new, beams))
    finally:
        head.close()
        m.close()
    want = beam_oracle.generate_beam_ref([_rows(80 + g)[:n] for g, n in enumerate(pre)], [None, None],
                                         np.repeat(np.array(tin, np.int32), beams), n_new, beams, E, Wh, bias, P,
                                         (D, H, DFF, BLOCKS), None, eos=-1, forward=_chain(tables))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"tokens, parents\n{got[:2]}\n{want[:2]}"
    assert_bits_equal(got[2], want[2], "scores")
