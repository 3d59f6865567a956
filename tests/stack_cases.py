"""The model matrix of the generation-loop tests: every stack architecture at the suite's small size (d_model 64, 4
heads, d_ff 200, 2 blocks, max_seq 16, weights from prenorm_oracle.prenorm_weights), each with the keywords of its
qg.Decoder call, the weight kinds it loads and its oracle chain as a callable (X, enc) -> hidden rows -- the `forward`
of head_oracle.generate_ref, sample_oracle.generate_sampled_ref and beam_oracle.generate_beam_ref.  Built once for the
host checks (tests/test_generate_archs_host.py asserts, on the oracles alone, that every case is sensitive to the error
it is there for) and for the GPU tests (tests/test_gpu_generate_archs.py), which then cannot pass vacuously.  TEST
INFRASTRUCTURE ONLY.

A RoPE entry's chain takes the tables as an argument: the GPU tests hand it the tables READ BACK from the model, so no
bit-exact check rests on two libms agreeing; the host checks use rope_oracle.make_tables.  Every expected result is
computed once per process and per pair of tables.
"""
import collections
import functools

import numpy as np

import beam_oracle
import head_oracle
import prenorm_oracle as PO
import rope_oracle as RO
import sample_oracle
from oracle import oracle as O

D, H, DFF, BLOCKS, MAX_SEQ = 64, 4, 200, 2, 16
DK = D // H
DIMS = (D, H, DFF, BLOCKS)
MODEL_SEED = 404                   # the creators' seed; every tensor the chains read is loaded over it
WEIGHT_SEED = 23
VOCAB = 50
MAX_ENC = 7
ENC_ROWS = (7, 5, 3)               # encoder rows of sequence / group b on the cross-attention entries

# generate and generate_sampled: three slots
PRE, N_NEW = (4, 0, 2), 4
TOP_K, TOP_P, TEMPERATURE, SAMPLE_SEED, STREAMS = 8, 0.9, 0.7, 77, (5, 1, 9)
# the beam searches: two groups of three beams
BEAMS, GROUPS, BEAM_PRE = 3, 2, (3, 1)
ROWS = BEAMS * GROUPS
# the tables' end: the last token fed stands at position MAX_SEQ - 1
END_PRE, END_N_NEW = (MAX_SEQ - 4, MAX_SEQ - 5), 4

Model = collections.namedtuple("Model", "name only base pre rope activation pick")
# pick: the seed of the entry's inputs and start tokens, chosen on the CPU so that tests/test_generate_archs_host.py's
# conditions hold (a wrong rotation changes a token, the beams reorder after their first step)
MODELS = collections.OrderedDict((m.name, m) for m in (
    Model("dec-post-gelu", False, 1, False, False, "gelu_tanh", 0),
    Model("dec-pre-final", False, 1, True, False, "relu", 0),
    Model("dec-post-rope", False, 1, False, True, "relu", 1),
    Model("only-ref", True, 0, False, False, "relu", 0),
    Model("only-post", True, 1, False, False, "relu", 0),
    Model("only-pre-rope", True, 1, True, True, "relu", 0),
))
NAMES = list(MODELS)
ROPE_NAMES = [n for n in NAMES if MODELS[n].rope]


def _frozen(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.flags.writeable = False
    return a


# ---- the model ----------------------------------------------------------------------------------------------------------
def arch(name) -> int:
    """the oracle's arch word: the base in the low byte, the pre-LN bits"""
    m = MODELS[name]
    return m.base | (0x300 if m.pre else 0)


def decoder_keywords(name) -> dict:
    """the keywords of qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, max_enc_seq(name), seed=MODEL_SEED, causal=True,
    kv_cache=True, **decoder_keywords(name))"""
    m = MODELS[name]
    kw = {}
    if m.only:
        kw["decoder_only"] = True
    if m.base:
        kw.update(arch="standard", activation=m.activation)
    if m.pre:
        kw.update(norm_first=True, final_norm=True)
    if m.rope:
        kw["rope"] = True
    return kw


def max_enc_seq(name) -> int:
    return 0 if MODELS[name].only else MAX_ENC


@functools.lru_cache(maxsize=None)
def weights(cross: bool):
    W = PO.prenorm_weights(D, H, DFF, BLOCKS, WEIGHT_SEED, cross=cross, final_norm=True)
    for a in W.values():
        a.flags.writeable = False
    return W


def loaded_kinds(name):
    """[(block, kind)] of the tensors the entry loads: the reference block's matrices, the standard block's matrices
    and vectors, and with a final norm its gamma and beta"""
    m = MODELS[name]
    keep = (lambda k: k < 12) if m.base == 0 else (lambda k: k < PO.GF or m.pre)
    return [key for key in weights(not m.only) if keep(key[1])]


def host_tables(name):
    """the tables by the creation formula, for the host checks; None without RoPE"""
    return RO.make_tables(MAX_SEQ, DK) if MODELS[name].rope else None


def forward(name, tables=None):
    """The entry's chain as (X, enc) -> hidden rows.  tables: (cos, sin) on a RoPE entry -- the model's own, read back
    -- and None elsewhere."""
    m = MODELS[name]
    assert (tables is not None) == m.rope, "the tables belong to the RoPE entries, and those need them"
    return _chain(name, tables)


def _chain(name, tables):
    m, W, a = MODELS[name], weights(not MODELS[name].only), arch(name)
    if m.only:
        return lambda X, enc: RO.decoder_only_forward(X, W, D, H, BLOCKS, a, causal=True, rope=tables,
                                                      activation=m.activation)
    return lambda X, enc: RO.decoder_forward_rope(X, enc, W, D, H, BLOCKS, tables, a, causal=True,
                                                  activation=m.activation)


def unrotated_forward(name):
    """a RoPE entry's chain WITHOUT the rotation: a wrong model of the sensitivity checks"""
    assert MODELS[name].rope
    return _chain(name, None)


def ahead_forward(name, tables, from_row):
    """a RoPE entry's chain on shifted_tables(tables, from_row): the wrong model whose rows from from_row on stand one
    position ahead of the rows before them"""
    assert MODELS[name].rope
    return _chain(name, shifted_tables(tables, from_row))


def shifted_tables(tables, from_row=0):
    """the tables with every row from `from_row` on replaced by its successor (the last one stays): the rows a loop
    would read whose position runs one ahead from there on"""
    out = []
    for t in tables:
        s = np.array(t, np.float32)
        s[from_row:-1] = t[from_row + 1:]
        out.append(s)
    return tuple(out)


# ---- the head ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_tables():
    """E, P, W (d_model x vocab) and a bias, as _head of tests/test_gpu_decoder_only.py: read-only"""
    return (_frozen(O.uniform((VOCAB, D), 601)), _frozen(O.uniform((MAX_SEQ, D), 602, -0.1, 0.1)),
            _frozen(O.uniform((D, VOCAB), 603)), _frozen(O.uniform((VOCAB,), 604, -0.05, 0.05)))


# ---- the inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(seed, n):
    return _frozen(O.uniform((n, D), seed) if n else np.zeros((0, D), np.float32))


def enc_rows(name, b):
    """sequence / group b's encoder output; None on a decoder-only entry"""
    return None if MODELS[name].only else rows(1500 + 10 * MODELS[name].pick + b, ENC_ROWS[b])


def prefix(name, b, n=None):
    """slot b's prefill rows of generate / generate_sampled (PRE[b] of them unless n says otherwise)"""
    return rows(1100 + 10 * MODELS[name].pick + b, PRE[b] if n is None else n)


def beam_prefix(name, g):
    return rows(1300 + 10 * MODELS[name].pick + g, BEAM_PRE[g])


def tokens_in(name, n=3):
    p = MODELS[name].pick
    return [(7 + 13 * p + 21 * b) % VOCAB for b in range(n)]


def beam_tokens_in(name):
    p = MODELS[name].pick
    return [(5 + 11 * p + 26 * g) % VOCAB for g in range(GROUPS)]


def probe_row(r):
    """the fixed row fed to place r after a search"""
    return rows(1700 + r, 1)


# ---- the expected results ------------------------------------------------------------------------------------------------
_cache = {}


def _once(what, name, tables, make):
    key = (what, name) + (() if tables is None else tuple(t.tobytes() for t in tables))
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def greedy(name, fwd, pre=PRE, n_new=N_NEW):
    """generate_ref per slot on the chain fwd, or on fwd[b] for slot b: n_new x len(pre)"""
    E, P, W, bias = head_tables()
    tin = tokens_in(name)
    per_slot = fwd if isinstance(fwd, (list, tuple)) else [fwd] * len(pre)
    cols = [head_oracle.generate_ref(prefix(name, b, pre[b]), enc_rows(name, b), tin[b], n_new, E, W, bias, P, DIMS,
                                     None, forward=per_slot[b]) for b in range(len(pre))]
    return _frozen(np.array(cols, np.int32).T, np.int32)


def expected_generate(name, tables=None):
    """generate_ref per slot, N_NEW x 3"""
    return _once("generate", name, tables, lambda: greedy(name, forward(name, tables)))


def expected_generate_end(name, tables):
    """generate_ref on the two long prefixes of the tables' end, END_N_NEW x 2"""
    return _once("end", name, tables, lambda: greedy(name, forward(name, tables), END_PRE, END_N_NEW))


def expected_sampled(name, tables=None, eos=None):
    """generate_sampled_ref per slot, N_NEW x 3"""
    def make():
        E, P, W, bias = head_tables()
        tin, fwd = tokens_in(name), forward(name, tables)
        cols = [sample_oracle.generate_sampled_ref(prefix(name, b), enc_rows(name, b), tin[b], N_NEW, E, W, bias, P,
                                                   DIMS, None, TOP_K, TOP_P, TEMPERATURE, SAMPLE_SEED, STREAMS[b],
                                                   eos=eos, forward=fwd) for b in range(3)]
        return _frozen(np.array(cols, np.int32).T, np.int32)
    return _once(("sampled", eos), name, tables, make)


def expected_beam(name, tables=None, eos=-1):
    """generate_beam_ref over the two groups: (tokens, parents, scores, final rows)"""
    def make():
        E, P, W, bias = head_tables()
        tin = np.repeat(np.array(beam_tokens_in(name), np.int32), BEAMS)
        out = beam_oracle.generate_beam_ref([beam_prefix(name, g) for g in range(GROUPS)],
                                            [enc_rows(name, g) for g in range(GROUPS)], tin, N_NEW, BEAMS, E, W, bias,
                                            P, DIMS, None, eos=eos, forward=forward(name, tables))
        for a in out[:3]:
            a.flags.writeable = False
        return out
    return _once(("beam", eos), name, tables, make)


def end_token(tokens):
    """The end token of an `eos` case: the token the run without one chooses in its second step at place 0 -- so the
    run with it produces it before its last step and holds it from there."""
    return int(np.asarray(tokens)[1, 0])


def fed_rows(name, b, tokens, pre=PRE):
    """the input rows generate fed to slot b: the embeddings of its start token and of all but its last chosen token"""
    E, P = head_tables()[:2]
    fed = [tokens_in(name)[b]] + np.asarray(tokens)[:-1, b].tolist()
    return head_oracle.embed_rows_ref(E, fed, P, [pre[b]], rows_per_seq=len(fed))
