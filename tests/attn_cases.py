"""Special-value inputs for qgemm_softmax_rows and qgemm_attention, built once for the host checks
(tests/test_attn_oracle_host.py asserts on the oracle's result alone that each set produces the condition it is named
for) and for the GPU tests (tests/test_gpu_attention.py, tests/test_gpu_encoder.py), which then cannot pass vacuously.
TEST INFRASTRUCTURE ONLY.

Every builder returns {name: (inputs, description)}.  The *_expected functions compute the oracle's result once per
process and hand out the same read-only array to every test that asks.
"""
import functools

import numpy as np

import attn_oracle
from oracle import oracle as O

SOFTMAX_W = 200
SOFTMAX_ROWS = "abcdef"  # the row order of every six-row softmax set
ATTN_BASE = (33, 100, 2, 24)       # (seq_q, seq_kv, H, d_k): the fused launch
ATTN_FALLBACK = (33, 513, 2, 24)   # the same variants one key chunk past the fused envelope: three launches
ATTN_SEED = 41                     # Q, K, V from seeds 41, 42, 43


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.flags.writeable = False
    return a


def softmax_rows_matrix() -> np.ndarray:
    """The six rows (a) .. (f), SOFTMAX_W wide."""
    w = SOFTMAX_W
    S = np.empty((6, w), np.float32)
    # (a) exps of fl(x - 0) run through the whole subnormal range (below about -87.3) down to +0 (below about -103.3)
    S[0] = np.linspace(0.0, -110.0, w, dtype=np.float32)
    # (b) -inf everywhere but one finite element, away from the seed column
    S[1] = -np.inf
    S[1, 77] = O.uniform((1,), 5)[0]
    # (c) non-positive values whose maximum is a zero of both signs: -0 seeds the max, +0 sits in another lane
    S[2] = -np.abs(O.uniform((w,), 6)) - np.float32(0.25)
    S[2, ::3] = -0.0
    S[2, 7] = 0.0
    # (d), (e) NaN in the seed column / in a lane's strided share; (f) +inf: exp(inf - inf)
    for r, seed in ((3, 7), (4, 8), (5, 9)):
        S[r] = O.uniform((w,), seed) * np.float32(8.0)
    S[3, 0] = np.nan
    S[4, 100] = np.nan
    S[5, 150] = np.inf
    return S


def softmax_sets() -> dict:
    """{name: ((S, scale), description)}: the six rows at scale 1, 0 and -1, and row (a) x 1e37 at scale 100."""
    S = softmax_rows_matrix()
    with np.errstate(over="ignore"):
        huge = S[:1] * np.float32(1e37)   # the far end of the row is -inf already; the products finish the rest
    return {
        "scale_1": ((S, 1.0), "rows (a)-(f): subnormal exps, a -inf row, a signed-zero maximum, NaN first, NaN inside, "
                               "+inf"),
        "scale_0": ((S, 0.0), "scale 0: finite elements become signed zeros, infinities become NaN"),
        "scale_neg1": ((S, -1.0), "scale -1: the order of every row reverses, -inf becomes +inf and +inf becomes -inf"),
        "overflow": ((huge, 100.0), "row (a) x 1e37 at scale 100: every product but the first overflows to -inf"),
    }


@functools.lru_cache(maxsize=None)
def softmax_expected(name: str) -> np.ndarray:
    S, scale = softmax_sets()[name][0]
    return _frozen(O.softmax_rows(S, scale))


def attention_sets(shape=ATTN_BASE) -> dict:
    """{name: ((Q, K, V), description)} at shape = (seq_q, seq_kv, H, d_k), seq_kv >= 38, H * d_k >= 31."""
    seq_q, seq_kv, H, dk = shape
    d = H * dk

    def base():
        return (O.uniform((seq_q, d), ATTN_SEED), O.uniform((seq_kv, d), ATTN_SEED + 1),
                O.uniform((seq_kv, d), ATTN_SEED + 2))

    out = {}
    Q, K, V = base()
    K[37, 5] = np.nan
    out["nan_in_k"] = ((Q, K, V), "NaN at K[37, 5]: every score row of head 0 holds a NaN, head 1 none")
    Q, K, V = base()
    V[37, 30] = np.inf
    out["inf_in_v"] = ((Q, K, V), "+inf at V[37, 30]: P[:, 37] > 0, so column 30 is +inf in every row")
    Q, K, V = base()
    V[37, 30] = np.inf
    out["inf_in_v_peaked"] = ((Q * np.float32(60.0), K, V), "the same V with Q x 60: where exp underflowed P[i, 37] is "
                                                            "+0 and 0 * inf is NaN")
    Q, K, V = base()
    Q[4, :] = 0.0
    out["zero_q_row"] = ((Q, K, V), "Q[4, :] = 0: row 4's scores are all +0, P is uniform")
    Q, K, V = base()
    Q[5, :dk] *= np.float32(1e30)
    out["overflowing_scores"] = ((Q, K * np.float32(1e10), V), "Q[5, :d_k] x 1e30 with K x 1e10: head 0's row 5 has "
                                                               "scores of +-inf, inf - inf is NaN")
    Q, K, V = base()
    V[:] = -0.0
    out["neg_zero_v"] = ((Q, K, V), "V all -0.0: the chain starts at +0, so every output is +0")
    Q, K, V = base()
    out["tiny_v"] = ((Q, K, V * np.float32(1e-38)), "V x 1e-38: every product and sum of P V is subnormal")
    return out


@functools.lru_cache(maxsize=None)
def attention_expected(name: str, shape=ATTN_BASE) -> np.ndarray:
    Q, K, V = attention_sets(shape)[name][0]
    return _frozen(attn_oracle.attention_ref(Q, K, V, shape[2], attn_oracle.default_scale(shape[3])))


ATTENTION_NAMES = ("nan_in_k", "inf_in_v", "inf_in_v_peaked", "zero_q_row", "overflowing_scores", "neg_zero_v",
                   "tiny_v")


def zero_row_decoder_inputs(seq=33, enc_seq=100, d=64):
    """X with row 3 all zero and enc_out with row 7 all zero: absmax 0, scale inf, 0 * inf -> NaN -> 0 in the pack."""
    X, enc = O.uniform((seq, d), 11), O.uniform((enc_seq, d), 12)
    X[3, :] = 0.0
    enc[7, :] = 0.0
    return X, enc
