"""Cases for the batched stack, the head and generate at full tables and real sizes, built once for the host checks
(tests/test_batch_plans_host.py asserts, on the library's plan queries and on the oracle alone, that every case
produces the condition it is named for) and for the GPU tests (tests/test_gpu_batch_plans.py,
tests/test_gpu_decoder_batch_plans.py, tests/test_gpu_head_wide.py, tests/test_gpu_generate_wide.py), which then
cannot pass vacuously.  TEST INFRASTRUCTURE ONLY.

One model, WIDE: with d_ff 4096 the four linears of a block change their int8 GEMM plan between the row counts of one
slot's step, of one sequence and of a real batch (PLAN_ROWS), so "batched equals single" compares different kernels.
Every builder hands out the same read-only arrays to every test that asks; the oracle results are computed once per
process.
"""
import functools

import numpy as np

import attn_oracle
import causal_oracle
import head_oracle
from oracle import oracle as O

WIDE = (128, 2, 4096, 2)           # d_model, heads (d_k 64), d_ff, blocks
D, N_HEADS, D_FF, N_BLOCKS = WIDE
D_K = D // N_HEADS
SEED = 47                          # the stacks' weight seed

# the six linear shapes of a block as (N, K); M is the row count of the call
LINEARS = {"qkv": (3 * D, D), "wo": (D, D), "q2": (D, D), "kv2": (2 * D, D), "up": (D_FF, D), "down": (D, D_FF)}

# (tile, splits, ring stages) of qkv, wo / q2, up and down at the row counts the GPU tests run, as
# tests/test_batch_plans_host.py holds them against qgemm_gemm_plan.  The ring depth is not reported by the query; it
# is derived as dispatch_dequant (csrc/gemm_i8.hip) chooses it: 64-tiles with at most 512 of them run the 3-stage ring,
# more the 2-stage ring (ring_stages below); the 32-tile kernel has one depth, the 256-tile kernel no ring.
PLAN_ROWS = {
    1:    {"qkv": (64, 1, 3), "wo": (64, 1, 3), "up": (64, 1, 3), "down": (64, 2, 3)},     # one slot's step
    8:    {"qkv": (64, 1, 3), "wo": (64, 1, 3), "up": (64, 1, 3), "down": (64, 2, 3)},     # one slot's 8-row step
    33:   {"qkv": (64, 1, 3), "wo": (64, 1, 3), "up": (32, 1, 4), "down": (64, 2, 3)},     # one sequence
    64:   {"qkv": (64, 1, 3), "wo": (64, 1, 3), "up": (32, 1, 4), "down": (64, 2, 3)},     # 64 slots x 1 row
    512:  {"qkv": (64, 1, 3), "wo": (64, 1, 3), "up": (64, 1, 3), "down": (64, 2, 3)},     # 64 slots x 8 rows
    1056: {"qkv": (32, 1, 4), "wo": (64, 1, 3), "up": (64, 1, 2), "down": (64, 2, 3)},     # 32 sequences
    2112: {"qkv": (32, 1, 4), "wo": (32, 1, 4), "up": (256, 1, 0), "down": (64, 2, 3)},    # 64 sequences
}
ROWS_STEP, ROWS_STEP8, ROWS_SEQ, ROWS_SLOTS, ROWS_SLOTS8, ROWS_32_SEQS, ROWS_64_SEQS = sorted(PLAN_ROWS)
PACK_STAGED_ROWS = 2048            # launch_pack_rows_t: the staged row pack from this many padded rows on


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def ring_stages(tile: int, m: int, n: int) -> int:
    """The LDS ring depth of the plan's kernel, as dispatch_dequant derives it from the tile count."""
    if tile == 32:
        return 4
    if tile == 64:
        return 3 if (round_up(m, 64) // 64) * (round_up(n, 64) // 64) <= 512 else 2
    return 0


def _frozen(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.flags.writeable = False
    return a


# ---- the encoder's batches ----------------------------------------------------------------------------------------
LEN_CYCLE = (33, 1, 40, 32, 7, 64, 31, 56)     # 264 rows per 8 sequences
ENC_MAX_SEQ = 64
MAX_ROWS = ROWS_64_SEQS
BATCHES = (32, 64)                             # sequences per forward_batch call: ROWS_32_SEQS and ROWS_64_SEQS rows


def lens(n_seqs: int) -> tuple:
    return tuple(LEN_CYCLE[b % len(LEN_CYCLE)] for b in range(n_seqs))


def oracle_checked(n_seqs: int) -> tuple:
    """The sequences of a batch held against the CPU oracle: the first eight (every length of the cycle; 0, 1 and 5
    among them), every 8th and the last."""
    return tuple(sorted(set(range(8)) | set(range(0, n_seqs, 8)) | {n_seqs - 1}))


PERMUTATION = tuple((37 * i + 11) % 64 for i in range(64))   # 37 is odd: a permutation of 0 .. 63


@functools.lru_cache(maxsize=None)
def encoder_seq(b: int) -> np.ndarray:
    """Sequence b's input rows: the same in every batch that holds it."""
    return _frozen(O.uniform((lens(b + 1)[b], D), 5000 + b))


@functools.lru_cache(maxsize=None)
def encoder_expected(b: int) -> np.ndarray:
    return _frozen(attn_oracle.encoder_forward_ref(encoder_seq(b), *WIDE, SEED))


# ---- the decoder's slots ------------------------------------------------------------------------------------------
N_SLOTS = 64
DEC_MAX_SEQ = 72
DEC_MAX_ENC = 33
# the slots held against the causal oracle: slot 0, slot 63, slots 1, 5, 9 .. (odd: every call reaches them; 5 is a
# slot with the longest prefix, DEC_MAX_SEQ rows) and three even ones of other prefill lengths -- a third of the slots
DEC_ORACLE_SLOTS = tuple(sorted(set(range(1, N_SLOTS, 4)) | {0, 2, 4, 6, 63}))


def enc_rows(b: int) -> int:
    return 1 + (5 * b) % DEC_MAX_ENC


@functools.lru_cache(maxsize=None)
def slot_enc(b: int) -> np.ndarray:
    return _frozen(O.uniform((enc_rows(b), D), 6001 + 2 * b))


@functools.lru_cache(maxsize=None)
def _slot_pool(b: int) -> np.ndarray:
    """Slot b's input rows in the order the schedule consumes them (a rewind takes fresh rows)."""
    return _frozen(O.uniform((DEC_MAX_SEQ + 16, D), 6000 + 2 * b))


@functools.lru_cache(maxsize=None)
def decoder_schedule() -> tuple:
    """The four calls of tests/test_gpu_decoder_batch_plans.py as (kind, rows_per_seq, slots, pos, n_rows, chunks):
    kind "varlen" or "batch", chunks the read-only input rows of every slot of the call, in the call's slot order.
      0  step_varlen prefills all 64 slots with lens(64), the slot order permuted: ROWS_64_SEQS rows;
      1  step_batch, 8 rows each, all 64 slots: ROWS_SLOTS8 rows.  The eight slots prefilled to 64 rows would leave no
         room for the calls after it, so they REWIND to position 56 with other rows than their prefill's;
      2  step_batch, one row each, all 64 slots in reverse order: ROWS_SLOTS rows;
      3  step_varlen on the 32 odd slots with 1 .. 9 rows each (as many as still fit where fewer do)."""
    filled = [0] * N_SLOTS
    used = [0] * N_SLOTS     # rows of the slot's pool consumed

    def take(b, n):
        rows = _slot_pool(b)[used[b]:used[b] + n]
        assert rows.shape[0] == n
        used[b] += n
        return rows

    calls = []
    pre = lens(N_SLOTS)
    order = list(PERMUTATION)
    calls.append(("varlen", 0, tuple(order), tuple(0 for _ in order), tuple(pre[b] for b in order),
                  tuple(take(b, pre[b]) for b in order)))
    for b in range(N_SLOTS):
        filled[b] = pre[b]
    order = list(range(N_SLOTS))
    pos = [min(filled[b], 56) for b in order]
    calls.append(("batch", 8, tuple(order), tuple(pos), tuple(8 for _ in order), tuple(take(b, 8) for b in order)))
    for b in order:
        filled[b] = pos[b] + 8
    order = list(range(N_SLOTS))[::-1]
    calls.append(("batch", 1, tuple(order), tuple(filled[b] for b in order), tuple(1 for _ in order),
                  tuple(take(b, 1) for b in order)))
    for b in order:
        filled[b] += 1
    order = list(range(1, N_SLOTS, 2))[::-1]
    n = [min(1 + (4 * (b // 2)) % 9, DEC_MAX_SEQ - filled[b]) for b in order]
    calls.append(("varlen", 0, tuple(order), tuple(filled[b] for b in order), tuple(n),
                  tuple(take(b, k) for b, k in zip(order, n))))
    return tuple(calls)


def slot_calls(b: int) -> list:
    """Slot b's part of the schedule: [(call index, pos, rows)] in call order."""
    out = []
    for c, (_, _, slots, pos, _, chunks) in enumerate(decoder_schedule()):
        if b in slots:
            i = slots.index(b)
            out.append((c, pos[i], chunks[i]))
    return out


def final_filled() -> list:
    filled = [0] * N_SLOTS
    for _, _, slots, pos, n_rows, _ in decoder_schedule():
        for b, p, n in zip(slots, pos, n_rows):
            assert p <= filled[b]
            filled[b] = p + n
    return filled


@functools.lru_cache(maxsize=None)
def slot_expected(b: int) -> dict:
    """{call index: the causal oracle's output rows for slot b's rows of that call}: the decoder's forward on the
    slot's whole sequence as it stands at that call.  forward(X[:n]) is forward(X)[:n], so one forward serves every call
    up to the next rewind."""
    out, pending = {}, []
    cur = np.zeros((0, D), np.float32)

    def flush():
        if pending:
            ref = causal_oracle.decoder_forward_causal_ref(cur, slot_enc(b), *WIDE, SEED)
            for c, p, n in pending:
                out[c] = _frozen(ref[p:p + n])
            del pending[:]

    for c, p, rows in slot_calls(b):
        if p < cur.shape[0]:
            flush()     # a rewind: the rows past p are about to change
        cur = np.concatenate([cur[:p], rows])
        pending.append((c, p, rows.shape[0]))
    flush()
    return out


# ---- the head at a real vocabulary --------------------------------------------------------------------------------
VOCAB = 50257                      # odd: every second row of a dense logits buffer starts off a 16-byte boundary
HEAD_MAX_ROWS = 64
HEAD_ROWS = (1, 2, 8, 33, 64)
TIED_ROWS = (0, 1, 2, 3, 4, 5, 6, 7, 33, 63)   # the hidden rows whose winning column is planted again elsewhere
VOCAB_TWO_PARTS = 8195             # the smallest odd width the argmax tests split, with max_rows 3
VOCAB_MANY_PARTS = 262147          # one row of it is cut into more than 32 parts, with max_rows 2


def argmax_chunk(w: int, parts: int) -> int:
    """The columns of one part of a split argmax (csrc/head.hip, argmax_plan): ceil(w / parts) rounded up to a
    multiple of 4."""
    return round_up((w + parts - 1) // parts, 4)


@functools.lru_cache(maxsize=None)
def head_hidden() -> np.ndarray:
    return _frozen(O.uniform((HEAD_MAX_ROWS, D), 7003))


def plant_ties(W, bias, logits, rows, part_counts):
    """Copies, for every row of `rows`, the column of W (and the bias entry) that wins that row's argmax to a column
    20000 further on (back where the row's end is nearer) -- another part under every plan of part_counts -- and, under
    each of those plans, to a column at a part seam: the first column past the winner's part, else the last one before
    it, else the seams further away in that order.  In place; a column that is some row's winner or already planted is
    never a target."""
    w = W.shape[1]
    winners = np.argmax(logits, axis=1)
    taken = set(int(c) for c in winners)
    for r in rows:
        c = int(winners[r])
        targets = [[c + 20000, c + 20001] if c + 20001 < w else [c - 20000, c - 20001]]
        for parts in part_counts:
            chunk = argmax_chunk(w, parts)
            part = c // chunk
            seams = [t for j in range(1, parts) for t in ((part + j) * chunk, (part - j + 1) * chunk - 1)]
            targets.append([t for t in seams if 0 <= t < w])
        for candidates in targets:
            t = next(t for t in candidates if t not in taken)
            taken.add(t)
            W[:, t] = W[:, c]
            bias[t] = bias[c]


@functools.lru_cache(maxsize=None)
def head_model(part_counts=(12, 8)):
    """(W d_model x VOCAB, bias) with the ties planted; part_counts: the argmax plans' parts for 1 / 8 and for 64 rows,
    which tests/test_batch_plans_host.py holds against qgemm_argmax_rows_plan."""
    W, bias = O.uniform((D, VOCAB), 7001), O.uniform((VOCAB,), 7002, -0.05, 0.05)
    plant_ties(W, bias, O.linear(head_hidden(), W, bias), TIED_ROWS, part_counts)
    return _frozen(W), _frozen(bias)


@functools.lru_cache(maxsize=None)
def head_logits() -> np.ndarray:
    """oracle.linear of all 64 hidden rows (a row's logits do not depend on the rows beside it)."""
    W, bias = head_model()
    return _frozen(O.linear(head_hidden(), W, bias))


@functools.lru_cache(maxsize=None)
def head_tokens() -> np.ndarray:
    return _frozen(head_oracle.argmax_rows_ref(head_logits())[0], np.int32)


def rows_tied_across_parts(logits, parts: int) -> list:
    """The rows whose maximum is attained in two or more columns that lie in different parts of a `parts`-part plan."""
    chunk = argmax_chunk(logits.shape[1], parts)
    out = []
    for r in range(logits.shape[0]):
        cols = np.flatnonzero(logits[r] == logits[r].max())
        if len(set((cols // chunk).tolist())) > 1:
            out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def small_head(vocab: int, rows: int):
    """(W, bias, H, logits, tokens) of the two small-row heads."""
    W, bias = O.uniform((D, vocab), 7100 + vocab % 97), O.uniform((vocab,), 7101 + vocab % 97, -0.05, 0.05)
    H = O.uniform((rows, D), 7102 + vocab % 97)
    logits = O.linear(H, W, bias)
    return _frozen(W), _frozen(bias), _frozen(H), _frozen(logits), _frozen(head_oracle.argmax_rows_ref(logits)[0],
                                                                          np.int32)


# ---- generate with 64 sequences -----------------------------------------------------------------------------------
GEN_N_NEW = 3
GEN_ORACLE_SEQS = tuple(sorted(set(range(0, N_SLOTS, 4)) | {N_SLOTS - 1}))    # every 4th, 0 and 63
GEN_PROBE_SLOTS = (0, 4, 40, 63)   # of GEN_ORACLE_SEQS: prefills of 0, 4, 0 and 7 rows


def gen_prefill_rows(b: int) -> int:
    return b % 8                   # 0 .. 7 rows: every 8th slot starts empty


def gen_token_in(b: int) -> int:
    return (37 * b + 17) % VOCAB


@functools.lru_cache(maxsize=None)
def gen_tables():
    """E (VOCAB x d_model) and P (DEC_MAX_SEQ x d_model)."""
    return _frozen(O.uniform((VOCAB, D), 7201)), _frozen(O.uniform((DEC_MAX_SEQ, D), 7202, -0.1, 0.1))


@functools.lru_cache(maxsize=None)
def gen_prefill(b: int) -> np.ndarray:
    n = gen_prefill_rows(b)
    return _frozen(O.uniform((n, D), 7300 + b) if n else np.zeros((0, D), np.float32))


@functools.lru_cache(maxsize=None)
def gen_expected(b: int) -> tuple:
    """head_oracle.generate_ref on sequence b alone: its GEN_N_NEW tokens."""
    (E, P), (W, bias) = gen_tables(), head_model()
    return tuple(head_oracle.generate_ref(gen_prefill(b), slot_enc(b), gen_token_in(b), GEN_N_NEW, E, W, bias, P, WIDE,
                                          SEED))


@functools.lru_cache(maxsize=None)
def gen_first_tokens() -> np.ndarray:
    """The first token of all 64 sequences from generate_ref's own steps, the vocabulary projection done once on the
    stacked last rows (oracle.linear works row by row).  Only the count of distinct first tokens is taken from this;
    tests/test_batch_plans_host.py holds it against generate_ref."""
    (E, P), (W, bias) = gen_tables(), head_model()
    last = []
    for b in range(N_SLOTS):
        row = head_oracle.embed_rows_ref(E, [gen_token_in(b)], P, [gen_prefill_rows(b)])
        X = np.concatenate([gen_prefill(b), row])
        last.append(causal_oracle.decoder_forward_causal_ref(X, slot_enc(b), *WIDE, SEED)[-1])
    return _frozen(head_oracle.argmax_rows_ref(O.linear(np.stack(last), W, bias))[0], np.int32)
