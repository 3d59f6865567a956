"""GPU parity of Encoder.forward_batch at real batch sizes: 32 and 64 sequences of batch_cases.WIDE (d_model 128,
d_ff 4096, 2 blocks), 1056 and 2112 rows, where the batch's linears run other int8 GEMM plans than a single sequence's
(32-tiles, the 64-tile kernel's 2-stage ring, the 256-tile kernel; tests/test_batch_plans_host.py holds the table
against the library), the row pack changes kernels at 2048 padded rows and the fused add + layernorm + pack gains
padding-row blocks.  Every sequence's rows are compared, bit for bit, with forward on that sequence on the same
encoder, with forward on a second encoder whose scratch holds one sequence, and for some with
attn_oracle.encoder_forward_ref on the CPU.  Every call writes into a NaN-filled output."""
import numpy as np
import pytest
import torch

import batch_cases as C
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)   # a copy: the cached inputs are read-only


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


@pytest.fixture(scope="module")
def encoders(qg, oracle, device):
    """(the batch encoder with a budget of 2112 rows, an encoder for one sequence of up to 64 rows)"""
    batch = qg.Encoder(*C.WIDE, max_seq=C.ENC_MAX_SEQ, seed=C.SEED, max_rows=C.MAX_ROWS)
    single = qg.Encoder(*C.WIDE, max_seq=C.ENC_MAX_SEQ, seed=C.SEED)
    yield batch, single
    batch.close()
    single.close()


def _forward_batch(enc, order, device):
    """forward_batch on the sequences `order` into a NaN-filled output: {sequence: its rows}."""
    seqs = [C.encoder_seq(b) for b in order]
    X = _dev(np.concatenate(seqs), device)
    Y = _nan(X.shape, device)
    assert enc.forward_batch(X, [s.shape[0] for s in seqs], Y=Y) is Y
    y, out, at = Y.cpu().numpy(), {}, 0
    for b, s in zip(order, seqs):
        out[b] = y[at:at + s.shape[0]]
        at += s.shape[0]
    assert at == y.shape[0]
    return out


@pytest.mark.parametrize("n_seqs", C.BATCHES)
def test_a_real_batch_against_forward_and_the_oracle(qg, device, encoders, n_seqs):
    batch, single = encoders
    assert sum(C.lens(n_seqs)) == {32: C.ROWS_32_SEQS, 64: C.ROWS_64_SEQS}[n_seqs]
    assert qg.attention_varlen_plan(C.lens(n_seqs), C.lens(n_seqs), C.N_HEADS, C.D_K) == "attention_fused_kernel<many>"
    got = _forward_batch(batch, range(n_seqs), device)
    for b in range(n_seqs):
        s = C.encoder_seq(b)
        assert got[b].shape == s.shape and np.isfinite(got[b]).all(), b
        for enc, name in ((batch, "the same encoder"), (single, "an encoder of one sequence")):
            one = _nan(s.shape, device)
            enc.forward(_dev(s, device), Y=one)
            assert_bits_equal(got[b], one.cpu().numpy(), f"{n_seqs} sequences: sequence {b} against forward on {name}")
    for b in C.oracle_checked(n_seqs):
        assert_bits_equal(got[b], C.encoder_expected(b), f"{n_seqs} sequences: sequence {b} against the oracle")


def test_a_permuted_batch_changes_no_sequence(qg, device, encoders):
    """The 64 sequences in another order: every sequence lands on other rows of the matrix -- other tiles, other
    padding -- and keeps its bits."""
    batch, _ = encoders
    first = _forward_batch(batch, range(64), device)
    again = _forward_batch(batch, C.PERMUTATION, device)
    for b in range(64):
        assert_bits_equal(again[b], first[b], f"sequence {b} at another place in the batch")
    for b in C.oracle_checked(64):
        assert_bits_equal(again[b], C.encoder_expected(b), f"permuted: sequence {b} against the oracle")
