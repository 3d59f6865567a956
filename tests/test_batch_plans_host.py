"""What the GPU tests of the batched stack, the head and generate rely on, checked without a GPU: the int8 GEMM plan of
every linear of batch_cases.WIDE at the row counts those tests run (qgemm_gemm_plan needs no device), the row pack's
threshold, the argmax plans at the real vocabularies, the attention plan of the length lists, and -- on the oracle
alone -- that the planted ties, the decoder schedule and the generate case are what they are named for.  The GPU tests
import the same constants, so a change to a dispatch threshold fails here instead of letting them pass vacuously."""
import ctypes

import numpy as np

import batch_cases as C
import head_oracle


def _plan(qg, m, n, k):
    tile = ctypes.c_int(-1)
    splits = qg.load().qgemm_gemm_plan(m, n, k, ctypes.byref(tile), None)
    return tile.value, splits


def test_every_linear_crosses_the_plans(qg):
    """The table of batch_cases.PLAN_ROWS is the library's answer.  The ring depth is not part of the query: it is
    derived from the tile count as dispatch_dequant does (batch_cases.ring_stages)."""
    for m, want in C.PLAN_ROWS.items():
        for name, (tile, splits, stages) in want.items():
            n, k = C.LINEARS[name]
            assert _plan(qg, m, n, k) == (tile, splits), (m, name)
            assert C.ring_stages(tile, m, n) == stages, (m, name)
        assert _plan(qg, m, *C.LINEARS["q2"]) == _plan(qg, m, *C.LINEARS["wo"])
    # the transitions themselves: a batched call and the per-sequence call it is compared with run different kernels
    step, seq, slots8, b32, b64 = (C.PLAN_ROWS[m] for m in (C.ROWS_STEP, C.ROWS_SEQ, C.ROWS_SLOTS8, C.ROWS_32_SEQS,
                                                            C.ROWS_64_SEQS))
    assert step["up"][0] == 64 and seq["up"][0] == 32 and b64["up"][0] == 256
    assert (slots8["up"][0], slots8["up"][2]) == (64, 3) and (b32["up"][0], b32["up"][2]) == (64, 2)
    assert seq["qkv"][0] == 64 and b32["qkv"][0] == 32
    assert b32["wo"][0] == 64 and b64["wo"][0] == 32
    assert all(p["down"][:2] == (64, 2) for p in C.PLAN_ROWS.values()), "the split-K kernel at every row count"
    # the cross keys' projection runs on one slot's enc_out alone, at most DEC_MAX_ENC rows
    assert {_plan(qg, C.enc_rows(b), *C.LINEARS["kv2"]) for b in range(C.N_SLOTS)} == {(64, 1)}


def test_every_call_of_the_gpu_tests_sits_on_a_row_of_the_table(qg):
    assert sum(C.LEN_CYCLE) == 264 and max(C.LEN_CYCLE) == C.ENC_MAX_SEQ
    assert [sum(C.lens(n)) for n in C.BATCHES] == [C.ROWS_32_SEQS, C.ROWS_64_SEQS] and C.MAX_ROWS == C.ROWS_64_SEQS
    assert sorted(C.PERMUTATION) == list(range(64)) and list(C.PERMUTATION) != list(range(64))
    # every single sequence and every one-slot step the batches are compared with: the plans of ROWS_STEP up to 32
    # rows (one row of 32-tiles), those of ROWS_SEQ from 33 on
    for m in set(C.LEN_CYCLE) | set(range(1, 10)):
        like = C.ROWS_SEQ if m > 32 else C.ROWS_STEP
        for name in ("qkv", "wo", "up", "down"):
            n, k = C.LINEARS[name]
            tile, splits = _plan(qg, m, n, k)
            assert (tile, splits, C.ring_stages(tile, m, n)) == C.PLAN_ROWS[like][name], (m, name)
    # the activation pack: pairs of rows below 2048 padded rows, the staged kernel from there on
    assert C.round_up(C.ROWS_64_SEQS, 256) >= C.PACK_STAGED_ROWS > C.round_up(C.ROWS_SLOTS, 256)
    assert C.round_up(C.ROWS_32_SEQS, 256) < C.PACK_STAGED_ROWS
    # the decoder's schedule
    calls = C.decoder_schedule()
    assert [kind for kind, *_ in calls] == ["varlen", "batch", "batch", "varlen"]
    assert [sum(n_rows) for *_, n_rows, _ in calls][:3] == [C.ROWS_64_SEQS, C.ROWS_SLOTS8, C.ROWS_SLOTS]
    assert all(sorted(slots) == list(range(64)) for _, _, slots, *_ in calls[:3])
    assert list(calls[0][2]) != sorted(calls[0][2]), "the prefill's slot order is permuted"
    rewound = [b for b, p in zip(calls[1][2], calls[1][3]) if p < C.lens(64)[b]]
    assert len(rewound) == 8 and all(C.lens(64)[b] == 64 for b in rewound)
    assert sorted(calls[3][2]) == list(range(1, 64, 2)) and set(calls[3][4]) == set(range(1, 10))
    filled = C.final_filled()
    assert max(filled) == C.DEC_MAX_SEQ and filled[5] == C.DEC_MAX_SEQ and min(filled) >= 10
    assert {0, 63, 5} <= set(C.DEC_ORACLE_SLOTS) and 4 * len(C.DEC_ORACLE_SLOTS) >= C.N_SLOTS
    assert {C.enc_rows(b) for b in range(64)} == set(range(1, 34)) and max(C.enc_rows(b) for b in range(64)) == C.DEC_MAX_ENC
    for b in (5, 8):
        exp = C.slot_expected(b)
        assert [exp[c].shape[0] for c, _, _ in C.slot_calls(b)] == [rows.shape[0] for _, _, rows in C.slot_calls(b)]
    # the attention: one table launch for every length list
    table = "attention_fused_kernel<many>"
    for n in C.BATCHES:
        assert qg.attention_varlen_plan(C.lens(n), C.lens(n), C.N_HEADS, C.D_K) == table
    for _, _, slots, pos, n_rows, _ in (calls[0], calls[3]):
        assert qg.attention_varlen_plan(n_rows, [p + n for p, n in zip(pos, n_rows)], C.N_HEADS, C.D_K) == table
        assert qg.attention_varlen_plan(n_rows, [C.enc_rows(b) for b in slots], C.N_HEADS, C.D_K) == table


def test_the_argmax_splits_at_the_real_vocabularies(qg):
    assert C.VOCAB % 4 == 1 and C.VOCAB_TWO_PARTS % 2 == 1 and C.VOCAB_MANY_PARTS % 2 == 1
    for rows in (1, 8, 64):
        assert qg.argmax_rows_plan(rows, C.VOCAB) > 1
    assert all(qg.argmax_rows_plan(rows, C.VOCAB) > 1 for rows in range(1, C.HEAD_MAX_ROWS + 1))
    assert [qg.argmax_rows_plan(rows, C.VOCAB_TWO_PARTS) for rows in (1, 2, 3)] == [2, 2, 2]
    assert qg.argmax_rows_plan(1, C.VOCAB_MANY_PARTS) > 32, "the combine kernel's upper half-wave holds candidates"
    # the head's workspace: the largest need is not the largest row count's
    L = qg.load()
    need = [L.qgemm_argmax_rows_workspace_size(rows, C.VOCAB) for rows in range(1, C.HEAD_MAX_ROWS + 1)]
    assert max(need) > need[-1]
    # the logits GEMM of the three heads: the 256-tile kernel at the real vocabularies, 32-tiles at the small one
    for rows in C.HEAD_ROWS:
        assert _plan(qg, rows, C.VOCAB, C.D) == (256, 1)
    assert _plan(qg, 3, C.VOCAB_TWO_PARTS, C.D) == (32, 1) and _plan(qg, 2, C.VOCAB_MANY_PARTS, C.D) == (256, 1)


def test_the_planted_ties_are_ties_across_parts(qg, oracle):
    """On the oracle's logits alone: in at least 8 rows the maximum is attained in columns of different parts, under
    the plan of every row count the head runs, rows 0 .. 7 (the 1-row and 8-row calls) among them; the lowest of the
    tied columns is the oracle's token."""
    parts = tuple(qg.argmax_rows_plan(rows, C.VOCAB) for rows in (1, 8, 64))
    assert (parts[0], parts[2]) == (12, 8) and parts[1] == parts[0], "batch_cases.head_model plants for these plans"
    logits, tokens = C.head_logits(), C.head_tokens()
    for p in set(qg.argmax_rows_plan(rows, C.VOCAB) for rows in range(1, C.HEAD_MAX_ROWS + 1)):
        tied = C.rows_tied_across_parts(logits, p)
        assert len(tied) >= 8 and set(range(8)) <= set(tied), (p, tied)
    for r in C.TIED_ROWS:
        cols = np.flatnonzero(logits[r] == logits[r].max())
        assert len(cols) == 4 and tokens[r] == cols[0], (r, cols)
        for p in (parts[0], parts[2]):
            chunk = C.argmax_chunk(C.VOCAB, p)
            assert any(c % chunk in (0, chunk - 1) for c in cols), f"row {r}: no tied column at a seam of {p} parts"
    assert len(set(tokens.tolist())) >= 32
    # the wide head: a winner in a part of the upper half-wave
    _, _, _, wide, wtok = C.small_head(C.VOCAB_MANY_PARTS, 2)
    chunk = C.argmax_chunk(C.VOCAB_MANY_PARTS, qg.argmax_rows_plan(1, C.VOCAB_MANY_PARTS))
    assert max(int(t) // chunk for t in wtok) >= 32


def test_the_generate_case(oracle):
    assert {C.gen_prefill_rows(b) for b in range(C.N_SLOTS)} == set(range(8))
    assert {0, C.N_SLOTS - 1} <= set(C.GEN_ORACLE_SEQS) and set(range(0, C.N_SLOTS, 4)) <= set(C.GEN_ORACLE_SEQS)
    first = C.gen_first_tokens()
    assert len(set(first.tolist())) >= 32, "the 64 sequences must not all choose the same tokens"
    for b in (0, C.N_SLOTS - 1):
        assert C.gen_expected(b)[0] == first[b], "the stacked projection against generate_ref"
    assert max(C.gen_prefill_rows(b) for b in range(C.N_SLOTS)) + 2 * C.GEN_N_NEW + 1 <= C.DEC_MAX_SEQ
