"""Expected results of the sampled token choice (qgemm_sample_rows, Head.sample_tokens, Decoder.generate_sampled),
restated rule by rule from include/qgemm.h in numpy and plain Python.  TEST INFRASTRUCTURE ONLY.

The list is the argmax order written as a sort (greater value first, lower index among equal values, NaN and -inf left
out); the probabilities are the oracle's own softmax_rows at scale 1 / temperature; the cumulative sums are a float32
loop; the draw is the oracle's oracle_uniform_at.
"""
import numpy as np

import head_oracle
from oracle import oracle as O

F32 = np.float32


def uniform_at(seed, counter):
    """u of rule 6: element `counter` of the [0, 1) fill with `seed` (counter: any 64-bit value)."""
    return F32(O.lib().oracle_uniform_at(int(seed), int(counter) & (2 ** 64 - 1), 0.0, 1.0))


def inv_temperature(temperature):
    """(top_k override, inv_t) of rule 2."""
    t = F32(temperature)
    return (1, F32(1.0)) if t == 0 else (None, F32(1.0) / t)


def row_list(row, top_k, inv_t):
    """Rules 1, 3 and 4 on one row: (columns t_j, probabilities p_j, cumulative sums c_j), each of length k'."""
    row = np.asarray(row, dtype=F32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(row > -np.inf)          # false for a NaN and for -inf
        order = cand[np.lexsort((cand, -row[cand]))]  # value descending (+0 == -0), then index ascending
    cols = order[:top_k].astype(np.int32)
    if len(cols) == 0:
        return cols, np.zeros(0, F32), np.zeros(0, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = O.softmax_rows(np.ascontiguousarray(row[cols]).reshape(1, -1), float(inv_t))[0]
        c = np.empty(len(cols), F32)
        acc = F32(0.0)
        for j in range(len(cols)):
            acc = F32(acc + p[j])
            c[j] = acc
    return cols, p, c


def nucleus(c, top_p):
    """Rule 5: n."""
    with np.errstate(invalid="ignore"):
        thr = F32(F32(top_p) * c[-1])
        hit = np.flatnonzero(c >= thr)
    return int(hit[0]) + 1 if len(hit) else len(c)


def draw(c, n, u):
    """Rule 6: the position j in the list."""
    with np.errstate(invalid="ignore"):
        r = F32(F32(u) * c[n - 1])
        hit = np.flatnonzero(c[:n] > r)
    return int(hit[0]) if len(hit) else 0


def sample_rows_draws(S, top_k, top_p=1.0, temperature=1.0, seed=0, counter0s=(0,), counter_sets=None, prev=None,
                      eos=None):
    """sample_rows_ref for several draws from the same rows: one per entry of counter0s (row r's counter is
    counter0 + (r << 32)) or, where given, per entry of counter_sets (one counter per row).  The list, its
    probabilities and the nucleus do not depend on the counter and are worked out once per row.  Returns
    (idx int32[draws x rows], top_idx, top_prob, n_kept)."""
    S = np.asarray(S, dtype=F32)
    rows = S.shape[0]
    k_one, inv_t = inv_temperature(temperature)
    k = k_one or top_k
    sets = counter_sets if counter_sets is not None else [[c0 + (r << 32) for r in range(rows)] for c0 in counter0s]
    idx = np.zeros((len(sets), rows), np.int32)
    top_idx = np.full((rows, top_k), -1, np.int32)
    top_prob = np.zeros((rows, top_k), F32)
    n_kept = np.zeros(rows, np.int32)
    for r in range(rows):
        cols, p, c = row_list(S[r], k, inv_t)
        if len(cols):
            n = nucleus(c, top_p)
            for d, counters in enumerate(sets):
                idx[d, r] = cols[draw(c, n, uniform_at(seed, counters[r]))]
            top_idx[r, :len(cols)] = cols
            top_prob[r, :len(cols)] = p
            n_kept[r] = n
        if prev is not None and eos is not None and eos >= 0 and int(prev[r]) == eos:
            idx[:, r] = eos
    return idx, top_idx, top_prob, n_kept


def sample_rows_ref(S, top_k, top_p=1.0, temperature=1.0, seed=0, counter0=0, counters=None, prev=None, eos=None):
    """(idx int32[rows], top_idx int32[rows x top_k], top_prob float32[rows x top_k], n_kept int32[rows]): -1 and +0
    past the candidates, as qgemm_sample_rows stores them."""
    idx, top_idx, top_prob, n_kept = sample_rows_draws(S, top_k, top_p, temperature, seed, (counter0,),
                                                       None if counters is None else [counters], prev, eos)
    return idx[0], top_idx, top_prob, n_kept


def generate_sampled_ref(prefix, enc, token_in, n_new, E, W, bias, P, dims, seed, top_k, top_p, temperature,
                         sample_seed, stream, eos=None, forward=None):
    """head_oracle.generate_ref with sample_rows_ref in argmax_rows_ref's place: ONE sequence, the draw of the step that
    feeds position q made with the counter (stream << 32) + q, the token fed as prev.  forward: as generate_ref's."""
    model = head_oracle.model_forward(dims, seed, forward)
    X = np.ascontiguousarray(prefix, dtype=F32).reshape(-1, dims[0])
    out, tok = [], int(token_in)
    for _ in range(n_new):
        q = X.shape[0]
        X = np.concatenate([X, head_oracle.embed_rows_ref(E, [tok], P, [q])])
        H = model(X, enc)[-1:]
        logits = O.linear(np.ascontiguousarray(H), W, bias)
        tok = int(sample_rows_ref(logits, top_k, top_p, temperature, sample_seed, counters=[(stream << 32) + q],
                                  prev=[tok], eos=eos)[0][0])
        out.append(tok)
    return out
