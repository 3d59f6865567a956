"""Expected results for the output end of the model (qgemm_argmax_rows, qgemm_embed_rows, the head object and
qgemm_decoder_generate), restated in numpy and plain Python.  TEST INFRASTRUCTURE ONLY.

argmax_rows_ref is the reference's op_argmax chain as written (op_reduction.cuh MaxAccumFunc): the seed is index 0 and
the index moves to i iff S[i] > S[best], strictly, one element after another.
"""
import numpy as np

import causal_oracle
from oracle import oracle as O

QUIET_NAN = 0x7FC00000  # the row of a token outside the vocabulary


def argmax_rows_ref(S):
    """(idx int32[rows], val float32[rows]) of the literal sequential chain over every row of S."""
    S = np.asarray(S, dtype=np.float32)
    rows, w = S.shape
    idx = np.zeros(rows, np.int32)
    val = np.empty(rows, np.float32)
    for r in range(rows):
        row = S[r].tolist()  # float32 -> Python float is exact, and so are the comparisons
        best, acc = 0, row[0]
        for i in range(1, w):
            x = row[i]
            if x > acc:
                acc, best = x, i
        idx[r] = best
        val[r] = S[r, best]
    return idx, val


def embed_rows_ref(E, tokens, P=None, pos=None, rows_per_seq=1):
    """Y[r] = E[tokens[r]] (+ P[pos[r // rows_per_seq] + r % rows_per_seq], one fp32 add); a token outside the
    vocabulary gives a row of quiet NaNs."""
    E = np.asarray(E, dtype=np.float32)
    tokens = np.asarray(tokens).reshape(-1)
    Y = np.empty((len(tokens), E.shape[1]), np.float32)
    for r, t in enumerate(tokens.tolist()):
        if not 0 <= t < E.shape[0]:
            Y[r].view(np.uint32)[:] = QUIET_NAN
            continue
        Y[r] = E[t]
        if P is not None:
            p = int(pos[r // rows_per_seq]) + r % rows_per_seq
            Y[r] = E[t] + np.asarray(P, dtype=np.float32)[p]  # float32 + float32: one rounding
    return Y


def model_forward(dims, seed, forward=None):
    """The model of a whole-search oracle as a callable (X, enc) -> hidden rows on the whole input rows of one
    sequence: `forward` where given (any stack architecture: tests/stack_cases.py), else the reference block with
    seeded weights, causal_oracle.decoder_forward_causal_ref(X, enc, *dims, seed)."""
    if forward is not None:
        return forward
    return lambda X, enc: causal_oracle.decoder_forward_causal_ref(X, enc, *dims, seed)


def generate_ref(prefix, enc, token_in, n_new, E, W, bias, P, dims, seed, forward=None):
    """Greedy decoding of ONE sequence: `prefix` (rows x d_model, may be empty) are the input rows already fed; then
    token by token the embedding of the last token is appended, the causal decoder runs on the WHOLE prefix
    (model_forward: causal_oracle.decoder_forward_causal_ref unless `forward` is given), its last row goes through
    oracle.linear onto the vocabulary and argmax_rows_ref picks the next token.  Returns the n_new tokens."""
    model = model_forward(dims, seed, forward)
    X = np.ascontiguousarray(prefix, dtype=np.float32).reshape(-1, dims[0])
    out, tok = [], int(token_in)
    for _ in range(n_new):
        row = embed_rows_ref(E, [tok], P, [X.shape[0]])
        X = np.concatenate([X, row])
        H = model(X, enc)[-1:]
        tok = int(argmax_rows_ref(O.linear(np.ascontiguousarray(H), W, bias))[0][0])
        out.append(tok)
    return out
