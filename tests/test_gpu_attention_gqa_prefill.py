"""GPU parity of qgemm_attention_gqa outside the decode kernel's envelope -- the grouped three launches:
the batched fp32 GEMMs in G rounds of n_kv_heads batches and one softmax -- bit for bit the oracles on K and V with
every head repeated.  Through qg.attention(n_kv_heads=...), which brings the workspace the path needs."""
import pytest
import torch

from test_gpu_attention_decode_gqa import _dev, _qkv, _want
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

# (seq_q, seq_kv, heads, kv heads, d_k, q_pos0); q_pos0 None: no mask
CASES = (
    (40, 40, 6, 2, 64, 0),         # causal prefill inside the fused launch's envelope: the workspace is needed all the same
    (33, 600, 8, 2, 128, None),    # unmasked, wide heads, past 512 keys
    (2, 50, 32, 1, 16, 48),        # G = 32: decode-shaped, but more heads per group than the decode kernel takes
)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_grouped_three_launches_bit_exact(qg, oracle, device, case):
    seq_q, seq_kv, H, n_kv, dk, q_pos0 = case
    assert qg.attention_gqa_plan(seq_q, seq_kv, H, n_kv, dk) == "grouped_three_launches"
    assert qg.load().qgemm_attention_gqa_workspace_size(seq_q, seq_kv, H, n_kv, dk) == 4 * H * seq_q * seq_kv
    Q, K, V = _qkv(seq_q, seq_kv, H, n_kv, dk, 801)
    out = torch.full((seq_q, H * dk), float("nan"), device=device)
    qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H, O=out, causal=q_pos0 is not None, q_pos0=q_pos0,
                 n_kv_heads=n_kv)
    assert_bits_equal(out.cpu().numpy(), _want(Q, K, V, H, n_kv, q_pos0), f"grouped three launches {case}")
