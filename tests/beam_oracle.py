"""Expected results of beam search (qgemm_logsumexp_rows, qgemm_beam_step, Decoder.generate_beam), restated rule by
rule from include/qgemm.h in numpy and plain Python.  TEST INFRASTRUCTURE ONLY.

The sum is the binary tree written as repeated pairwise adds of a float32 array; the per-row lists are the argmax order
written as a sort (sample_oracle's); the group selection is a stable sort of the candidates in place order; the whole
search runs the causal decoder oracle on every live beam's whole prefix.
"""
import numpy as np

import head_oracle
from oracle import oracle as O

F32 = np.float32
NEG_INF = F32(-np.inf)


def tree_sum(e):
    """The root of the perfect binary tree over e padded with +0 to the least power of two >= max(len(e), 1024)."""
    e = np.asarray(e, dtype=F32)
    p = 1024
    while p < len(e):
        p *= 2
    x = np.zeros(p, F32)
    x[:len(e)] = e
    with np.errstate(invalid="ignore", over="ignore"):
        while len(x) > 1:
            x = x[0::2] + x[1::2]          # float32 + float32: one rounding per node
    return x[0]


def candidate_order(row):
    """The candidate columns (row > -inf) in the argmax's order: value descending (+0 == -0), then index ascending."""
    row = np.asarray(row, dtype=F32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(row > -np.inf)
    return cand[np.lexsort((cand, -row[cand]))]


def row_exps(row):
    """(m, e): rules 2 and 3 on one row; m = -inf and e = +0 everywhere without a candidate."""
    row = np.asarray(row, dtype=F32)
    e = np.zeros(len(row), F32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(row > -np.inf)
    if len(cand) == 0:
        return NEG_INF, e
    first = cand[np.lexsort((cand, -row[cand]))[0]]
    m = row[first]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (row[cand] - m).astype(F32)                 # fl(S - m)
        e[cand] = np.exp(d.astype(np.float64)).astype(F32)
    return m, e


def logsumexp_rows_ref(S):
    """(mx float32[rows], logz float32[rows])."""
    S = np.asarray(S, dtype=F32)
    mx, logz = np.empty(S.shape[0], F32), np.empty(S.shape[0], F32)
    for r in range(S.shape[0]):
        mx[r], e = row_exps(S[r])
        with np.errstate(divide="ignore", invalid="ignore"):
            logz[r] = F32(np.log(np.float64(tree_sum(e))))
    return mx, logz


def beam_step_ref(S, beams, scores_in=None, prev=None, eos=-1):
    """(parents int32[rows], tokens int32[rows], scores float32[rows]) of qgemm_beam_step's rules 1-5."""
    S = np.asarray(S, dtype=F32)
    rows = S.shape[0]
    assert rows % beams == 0
    if scores_in is None:
        scores_in = np.where(np.arange(rows) % beams == 0, F32(0.0), NEG_INF).astype(F32)
    scores_in = np.asarray(scores_in, dtype=F32)
    parents, tokens = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    scores = np.full(rows, NEG_INF, F32)
    for g in range(rows // beams):
        cands = []                                       # (c, place b * beams + j, token), in place order
        for b in range(beams):
            r = g * beams + b
            with np.errstate(invalid="ignore"):
                if not scores_in[r] > -np.inf:
                    continue                             # dead
            if eos >= 0 and prev is not None and int(prev[r]) == eos:
                cands.append((scores_in[r], b * beams, eos))
                continue                                 # finished: held
            cols = candidate_order(S[r])[:beams]
            if len(cols) == 0:
                continue
            m, e = row_exps(S[r])
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                logz = F32(np.log(np.float64(tree_sum(e))))
                for j, t in enumerate(cols):
                    lp = F32(F32(S[r, t] - m) - logz)
                    cands.append((F32(scores_in[r] + lp), b * beams + j, int(t)))
        with np.errstate(invalid="ignore"):
            cands = [c for c in cands if c[0] > -np.inf]
        cands.sort(key=lambda c: -float(c[0]))           # stable: equal values (+0 == -0) keep their place order
        for i in range(beams):
            at = g * beams + i
            if i < len(cands):
                scores[at], parents[at], tokens[at] = cands[i][0], cands[i][1] // beams, cands[i][2]
            else:
                parents[at] = i
    return parents, tokens, scores


def generate_beam_ref(prefixes, encs, tokens_in, n_new, beams, E, W, bias, P, dims, seed, scores_in=None, eos=-1,
                      forward=None):
    """The whole search on whole prefixes: group g starts from prefixes[g] (rows x d_model, may be empty) with encoder
    output encs[g]; every live beam keeps its own input rows, the causal decoder oracle runs on all of them at every
    step, its last row goes through oracle.linear and beam_step_ref chooses.  tokens_in: one token per row.  Returns
    (tokens, parents, scores), each n_new x rows, and the final input rows of every place (None for a dead one).
    forward: the model as a callable (X, enc) -> hidden rows, head_oracle.generate_ref's."""
    model = head_oracle.model_forward(dims, seed, forward)
    n_groups = len(prefixes)
    rows = n_groups * beams
    d, vocab = dims[0], np.asarray(W).shape[1]
    X = [np.ascontiguousarray(prefixes[r // beams], dtype=F32).reshape(-1, d) for r in range(rows)]
    tok = np.asarray(tokens_in, np.int32).reshape(rows)
    sc = None if scores_in is None else np.asarray(scores_in, F32)
    out_t, out_p, out_s = (np.zeros((n_new, rows), np.int32), np.zeros((n_new, rows), np.int32),
                           np.zeros((n_new, rows), F32))
    for t in range(n_new):
        with np.errstate(invalid="ignore"):
            live = np.arange(rows) % beams == 0 if sc is None else sc > -np.inf
        logits = np.zeros((rows, vocab), F32)
        for r in range(rows):
            X[r] = np.concatenate([X[r], head_oracle.embed_rows_ref(E, [int(tok[r])], P, [X[r].shape[0]])])
            if live[r] and not (eos >= 0 and int(tok[r]) == eos):
                H = model(X[r], encs[r // beams])[-1:]
                logits[r] = O.linear(np.ascontiguousarray(H), W, bias)[0]
        par, ntok, nsc = beam_step_ref(logits, beams, sc, tok, eos)
        X = [X[r // beams * beams + int(par[r])] for r in range(rows)]
        out_t[t], out_p[t], out_s[t] = ntok, par, nsc
        tok, sc = ntok, nsc
    with np.errstate(invalid="ignore"):
        final = [X[r] if n_new == 0 or out_s[-1, r] > -np.inf else None for r in range(rows)]
    return out_t, out_p, out_s, final
