"""Host checks of the generation-loop cases (tests/stack_cases.py), on the oracles alone.

1. The whole-search oracles' `forward=` keyword leaves the default path alone: with the old hard-wired chain passed
   explicitly, each of the three returns exactly what the default call returns on a case of the existing GPU tests.
2. Every case of tests/test_gpu_generate_archs.py is sensitive to the error it is there for, so a later edit of the seeds
   cannot quietly make the GPU tests blind:
   * on a RoPE entry the greedy tokens of the chain without the rotation differ from the rotated chain's;
   * and so do the tokens of a chain whose new rows stand one position ahead of the prefix.  The tables shifted by one
     position as a WHOLE are no such model: q_m . k_n under the rotation depends on m - n alone, so a uniform shift
     changes no score beyond its last bits and moved no token on any of 12 input seeds of either entry, so no seed can
     be picked for it; the shift therefore starts at the sequence's first new row, which is what a loop whose position
     is stale or runs ahead computes;
   * every beam search reorders after its first step: some parent at a step >= 1 is not the place's own index (at step
     0 only beam 0 lives and every parent is 0), so the gather / the re-index moves rows between live places;
   * every `eos` case produces its end token before the last step and holds it.
"""
import numpy as np
import pytest

import beam_oracle
import causal_oracle
import head_oracle
import sample_oracle
import stack_cases as C
from oracle import oracle as O

DIMS, SEED = causal_oracle.DECODER_FUSED[2:], causal_oracle.DECODER_SEED
D = DIMS[0]
VOCAB, MAX_POS = 1000, 40


@pytest.fixture(scope="module")
def old_case(oracle):
    """sequence 2 of tests/test_gpu_generate.py (2 prefill rows, 9 encoder rows, start token 0) and its head tables"""
    head = (O.uniform((VOCAB, D), 601), O.uniform((MAX_POS, D), 602, -0.1, 0.1), O.uniform((D, VOCAB), 603),
            O.uniform((VOCAB,), 604, -0.05, 0.05))
    return O.uniform((2, D), 622), O.uniform((9, D), 632), 0, head


class _Chain:
    """the chain the oracles had hard-wired, counting its calls"""

    def __init__(self):
        self.calls = 0

    def __call__(self, X, enc):
        self.calls += 1
        return causal_oracle.decoder_forward_causal_ref(X, enc, *DIMS, SEED)


# ---- 1. the default path ------------------------------------------------------------------------------------------------
def test_generate_ref_default_is_the_explicit_chain(old_case):
    X, enc, tok, (E, P, W, bias) = old_case
    chain = _Chain()
    want = head_oracle.generate_ref(X, enc, tok, 6, E, W, bias, P, DIMS, SEED)
    got = head_oracle.generate_ref(X, enc, tok, 6, E, W, bias, P, DIMS, None, forward=chain)
    assert got == want and chain.calls == 6


def test_generate_sampled_ref_default_is_the_explicit_chain(old_case):
    X, enc, tok, (E, P, W, bias) = old_case
    chain = _Chain()
    args = (X, enc, tok, 6, E, W, bias, P, DIMS)
    want = sample_oracle.generate_sampled_ref(*args, SEED, 40, 0.9, 0.8, 12345, 2, eos=None)
    got = sample_oracle.generate_sampled_ref(*args, None, 40, 0.9, 0.8, 12345, 2, eos=None, forward=chain)
    assert got == want and chain.calls == 6
    assert len(set(want)) > 1


def test_generate_beam_ref_default_is_the_explicit_chain(old_case):
    X, enc, tok, (E, P, W, bias) = old_case
    chain = _Chain()
    tin = np.full(3, tok, np.int32)
    want = beam_oracle.generate_beam_ref([X], [enc], tin, 4, 3, E, W, bias, P, DIMS, SEED)
    got = beam_oracle.generate_beam_ref([X], [enc], tin, 4, 3, E, W, bias, P, DIMS, None, forward=chain)
    assert chain.calls > 4
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g.view(np.int32), w.view(np.int32))
    for g, w in zip(got[3], want[3]):
        assert (g is None) == (w is None) and (g is None or np.array_equal(g.view(np.int32), w.view(np.int32)))


# ---- the matrix ------------------------------------------------------------------------------------------------------------
def test_the_matrix_has_the_six_architectures(oracle):
    want = {"dec-post-gelu": (False, 1, "gelu_tanh", False), "dec-pre-final": (False, 0x301, "relu", False),
            "dec-post-rope": (False, 1, "relu", True), "only-ref": (True, 0, "relu", False),
            "only-post": (True, 1, "relu", False), "only-pre-rope": (True, 0x301, "relu", True)}
    for name, (only, arch, act, rope) in want.items():
        m = C.MODELS[name]
        assert (m.only, C.arch(name), m.activation, m.rope) == (only, arch, act, rope), name
        kinds = {k for _, k in C.loaded_kinds(name)}
        assert (26 in kinds) == bool(arch & 0x200) and (12 in kinds) == bool(arch & 0xff), name
        assert (8 in kinds) == (not only), f"{name}: the cross-attention's matrices"
        assert (C.enc_rows(name, 0) is None) == only
    assert C.ENC_ROWS == (7, 5, 3) and C.PRE == (4, 0, 2) and C.BEAM_PRE == (3, 1) and C.N_NEW == 4
    assert len(set(C.STREAMS)) == 3 and set(C.STREAMS) != {0, 1, 2}, "streams other than the slots"
    assert max(p + C.END_N_NEW for p in C.END_PRE) == C.MAX_SEQ, "the last token fed stands at position max_seq - 1"


# ---- 2. sensitivity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ROPE_NAMES)
def test_rope_cases_see_a_missing_rotation_and_a_position_one_ahead(oracle, name):
    tables = C.host_tables(name)
    want = C.expected_generate(name, tables)
    plain = C.greedy(name, C.unrotated_forward(name))
    assert (plain != want).any(axis=0).any(), f"{name}: without the rotation the tokens are the same"
    # the new rows one position ahead of the prefix; slot 1 has no prefix, where the shift is uniform and changes nothing
    ahead = C.greedy(name, [C.ahead_forward(name, tables, p) for p in C.PRE])
    moved = (ahead != want).any(axis=0)
    assert moved[[b for b, p in enumerate(C.PRE) if p]].any(), f"{name}: a position one ahead gives the same tokens"
    # the long prefixes of the tables' end as well: their new rows read the tables' last rows
    end = C.expected_generate_end(name, tables)
    end_ahead = C.greedy(name, [C.ahead_forward(name, tables, p) for p in C.END_PRE], C.END_PRE, C.END_N_NEW)
    assert (end_ahead != end).any(), f"{name}: the tables' end, a position one ahead gives the same tokens"


@pytest.mark.parametrize("name", C.NAMES)
def test_beam_cases_reorder_after_the_first_step(oracle, name):
    tables = C.host_tables(name)
    own = np.arange(C.ROWS) % C.BEAMS
    for eos in (-1, C.end_token(C.expected_beam(name, tables)[0])):
        tok, par, sc, final = C.expected_beam(name, tables, eos)
        assert (par[0] == 0).all()
        live = sc[1:] > -np.inf
        assert ((par[1:] != own) & live).any(), f"{name}, eos {eos}: every live place continues itself"
        assert np.isfinite(sc[-1]).all() and all(f is not None for f in final), f"{name}: a place died"
        assert all(f.shape[0] == C.BEAM_PRE[r // C.BEAMS] + C.N_NEW for r, f in enumerate(final))


@pytest.mark.parametrize("name", C.NAMES)
def test_eos_cases_hold_their_end_token(oracle, name):
    tables = C.host_tables(name)
    # sampled: some sequence draws eos before its last step and holds it to the end
    free = C.expected_sampled(name, tables)
    eos = C.end_token(free)
    held = C.expected_sampled(name, tables, eos)
    first = [int(np.flatnonzero(held[:, b] == eos)[0]) if (held[:, b] == eos).any() else C.N_NEW for b in range(3)]
    assert min(first) < C.N_NEW - 1, f"{name}: eos {eos} is not drawn before the last step"
    for b in range(3):
        assert (held[first[b]:, b] == eos).all(), f"{name}: sequence {b} left its end token"
    # beams: some beam ends before the last step; the row that holds it keeps token and score
    tok, par, sc, _ = C.expected_beam(name, tables)
    eos = C.end_token(tok)
    tok, par, sc, _ = C.expected_beam(name, tables, eos)
    assert (tok[:-1] == eos).any(), f"{name}: no beam ends before the last step"
    kept = 0
    for t in range(1, C.N_NEW):
        for r in range(C.ROWS):
            src = r // C.BEAMS * C.BEAMS + int(par[t, r])
            if tok[t - 1, src] == eos and sc[t, r] > -np.inf:
                assert tok[t, r] == eos and sc[t, r].view(np.int32) == sc[t - 1, src].view(np.int32)
                kept += 1
    assert kept, f"{name}: no finished beam survived a step"
