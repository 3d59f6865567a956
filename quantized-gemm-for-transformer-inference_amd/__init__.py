"""qgemm_amd -- host-side mirror of the reference's quantized-GEMM operator over the C-ABI.

The product is ``build/libqgemm.so`` (hand-written gfx950 HIP kernels behind the C-ABI in
``include/qgemm.h``).  This module binds that ABI with ctypes and mirrors the reference's
operator interface for the hot path:

    op_quantized_mm(X, W, O, range)   <- op_mm.cuh:67-101 (same name, argument meaning, asserts)
    op_mm_quantize(A, B, C)           <- the north-star C-ABI op_mm_quantize(A,B,C,M,N,K)
    pack_a / pack_b / mm_packed       <- the chain's stages (op_absmax+op_inv_divide+op_multiply,
                                         op_mm<int8_t,int>+op_dequantize+op_multiply)
    fill_uniform                      <- op_uniform_init (op_elemwise.cuh:728-744), seeded

PyTorch is plumbing here: it owns device memory and streams.  There is NO CPU fallback: if the
HIP library is missing, every compute entry point raises.

Import it by path (the directory name is not a Python identifier)::

    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("qgemm_amd", "<repo>/quantized-gemm-for-transformer-inference_amd/__init__.py")
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "build", "libqgemm.so")
HEADER_PATH = os.path.join(REPO_DIR, "include", "qgemm.h")
DIST_LIB_PATH = os.path.join(PKG_DIR, "build", "libqgemm_dist.so")
DIST_HEADER_PATH = os.path.join(REPO_DIR, "include", "qgemm_dist.h")

DEFAULT_RANGE = 127.0  # `range` at every reference call site (test_quantize.cu:76, timing_quantize.cu:43)
ROW_PAD = 256          # packed operand rows are padded to the GEMM macro-tile
K_PAD = 128            # packed operand k is padded to the GEMM k-step

# Every symbol include/qgemm.h declares (checked against the header by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "op_mm_quantize",
    "op_mm_quantize_ex",
    "op_mm_quantize_workspace_size",
    "op_mm_quantize_ws",
    "qgemm_packed_size",
    "qgemm_pack_a",
    "qgemm_pack_b",
    "qgemm_mm_packed",
    "qgemm_mm_packed_i32",
    "qgemm_mm_fp32",
    "qgemm_mm_fp32_plan",
    "qgemm_error_stats",
    "qgemm_linear_workspace_size",
    "qgemm_linear",
    "qgemm_pack_a_dt",
    "qgemm_mm_packed_dt",
    "qgemm_linear_dt",
    "op_mm_quantize_prepacked",
    "op_mm_quantize_prepacked_workspace_size",
    "op_mm_quantize_prepacked_ws",
    "qgemm_softmax_rows",
    "qgemm_softmax_rows_causal",
    "qgemm_add_layernorm_rows",
    "qgemm_encoder_create",
    "qgemm_encoder_forward",
    "qgemm_encoder_destroy",
    "qgemm_attention_workspace_size",
    "qgemm_attention",
    "qgemm_attention_causal",
    "qgemm_attention_plan",
    "qgemm_decoder_create",
    "qgemm_decoder_create_ex",
    "qgemm_decoder_forward",
    "qgemm_decoder_begin",
    "qgemm_decoder_step",
    "qgemm_decoder_destroy",
    "qgemm_attention_decode_batched",
    "qgemm_decoder_create_slots",
    "qgemm_decoder_begin_slot",
    "qgemm_decoder_step_slot",
    "qgemm_decoder_step_batch",
    "qgemm_decoder_copy_slot",
    "qgemm_decoder_slot_state",
    "qgemm_attention_varlen_workspace_size",
    "qgemm_attention_varlen",
    "qgemm_attention_varlen_plan",
    "qgemm_encoder_create_rows",
    "qgemm_encoder_forward_batch",
    "qgemm_decoder_create_rows",
    "qgemm_decoder_step_varlen",
    "qgemm_argmax_rows_workspace_size",
    "qgemm_argmax_rows_plan",
    "qgemm_argmax_rows",
    "qgemm_embed_rows",
    "qgemm_head_create",
    "qgemm_head_logits",
    "qgemm_head_next_tokens",
    "qgemm_head_embed",
    "qgemm_head_destroy",
    "qgemm_decoder_generate",
    "qgemm_sample_rows_plan",
    "qgemm_sample_rows_workspace_size",
    "qgemm_sample_rows",
    "qgemm_head_sample_tokens",
    "qgemm_decoder_generate_sampled",
    "qgemm_logsumexp_rows_plan",
    "qgemm_logsumexp_rows_workspace_size",
    "qgemm_logsumexp_rows",
    "qgemm_beam_step_plan",
    "qgemm_beam_step_workspace_size",
    "qgemm_beam_step",
    "qgemm_head_beam_step",
    "qgemm_decoder_gather_slots",
    "qgemm_decoder_read_slot",
    "qgemm_decoder_generate_beam",
    "qgemm_attention_decode_indirect",
    "qgemm_beam_reindex",
    "qgemm_decoder_beam_begin",
    "qgemm_decoder_step_batch_indirect",
    "qgemm_decoder_beam_reindex",
    "qgemm_decoder_read_beam_table",
    "qgemm_decoder_generate_beam_indirect",
    "qgemm_pack_b_window",
    "qgemm_pack_b_window_plan",
    "qgemm_model_weight_shape",
    "qgemm_model_set_weight",
    "qgemm_model_packed_weight",
    "qgemm_model_bias",
    "qgemm_mm_outlier_workspace_size",
    "qgemm_mm_outlier",
    "qgemm_outlier_count",
    "qgemm_linear_outlier_workspace_size",
    "qgemm_linear_outlier",
    "qgemm_set_gemm_events",
    "qgemm_set_event_mode",
    "qgemm_fill_uniform",
    "qgemm_gemm_plan",
    "qgemm_version",
    "qgemm_layernorm_rows",
    "qgemm_layernorm_pack_a",
    "qgemm_gelu_rows",
    "qgemm_gelu_pack_a",
    "qgemm_model_create",
    "qgemm_model_info",
    "qgemm_prenorm_pack_a",
    "qgemm_add_rows",
    "qgemm_decoder_slot_begun",
    "qgemm_model_rope_tables",
    "qgemm_rope_rows",
    "qgemm_rope_rows_varlen",
    "qgemm_rmsnorm_rows",
    "qgemm_rmsnorm_pack_a",
    "qgemm_prenorm_rms_pack_a",
    "qgemm_glu_rows",
    "qgemm_glu_pack_a",
)

# Every symbol include/qgemm_dist.h declares (libqgemm_dist.so: M-shards + RCCL all-gather).
DIST_EXPORTED_SYMBOLS = (
    "qgemm_shard_rows",
    "op_mm_quantize_shard",
    "qgemm_comm_unique_id",
    "qgemm_comm_init_rank",
    "qgemm_comm_init_all",
    "qgemm_comm_destroy",
    "qgemm_comm_count",
    "qgemm_comm_user_rank",
    "qgemm_allgather_rows",
    "qgemm_allgather_plan",
    "qgemm_allgather_chunk_plan",
    "op_mm_quantize_shard_pipelined_workspace_size",
    "op_mm_quantize_shard_pipelined",
    "qgemm_node_allgather_plan",
    "qgemm_node_mm_quantize",
)
COMM_ID_BYTES = 128

HIP_ERROR_INVALID_VALUE = 1
QGEMM_F32, QGEMM_BF16 = 0, 1  # element-type tags of the _dt entry points (include/qgemm.h)
QGEMM_DECODER_CAUSAL = 1       # qgemm_decoder_create_ex flag: causal mask on the self-attention
QGEMM_DECODER_KV_CACHE = 8     # ... and per-block key / value caches for begin() / step() (with CAUSAL only)
QGEMM_DECODE_MAX_BATCH = 64    # sequences per attention_decode_batched / step_batch call, cache slots per decoder
QGEMM_VARLEN_MAX_SEQS = 64     # sequences per attention_varlen / forward_batch / step_varlen call
QGEMM_ARCH_REFERENCE, QGEMM_ARCH_STANDARD = 0, 1  # qgemm_model_create: the reference's block / the post-LN block
QGEMM_ACT_RELU, QGEMM_ACT_GELU_TANH = 0, 1        # ... and the FFN's activation (GELU: standard only)
QGEMM_ARCH_NORM_FIRST, QGEMM_ARCH_FINAL_NORM = 0x100, 0x200  # modifier bits on arch: the pre-LN block
# ... a decoder without the cross-attention third / rotary embeddings on Q and K
QGEMM_ARCH_DECODER_ONLY, QGEMM_ARCH_ROPE = 0x400, 0x800
# ... the RMS norm with gamma alone / the gated FFN (act(x W1) * (x W3)) W2 of Llama-style blocks;
# 0x1000 is no bit of arch.  SiLU: with the gated FFN only
QGEMM_ARCH_RMSNORM, QGEMM_ARCH_GATED_FFN = 0x2000, 0x4000
QGEMM_ACT_SILU = 2
ARCHS = {"reference": QGEMM_ARCH_REFERENCE, "standard": QGEMM_ARCH_STANDARD}
ACTIVATIONS = {"relu": QGEMM_ACT_RELU, "gelu_tanh": QGEMM_ACT_GELU_TANH, "silu": QGEMM_ACT_SILU}
NORMS = ("layer", "rms")


class ModelDesc(ctypes.Structure):
    """qgemm_model_desc (include/qgemm.h)."""
    _fields_ = [("size", ctypes.c_uint32), ("cross", ctypes.c_int), ("d_model", ctypes.c_int),
                ("n_heads", ctypes.c_int), ("d_ff", ctypes.c_int), ("n_blocks", ctypes.c_int),
                ("max_seq", ctypes.c_int), ("max_enc_seq", ctypes.c_int), ("seed", ctypes.c_uint64),
                ("flags", ctypes.c_int), ("n_slots", ctypes.c_int), ("max_rows", ctypes.c_int),
                ("arch", ctypes.c_int), ("activation", ctypes.c_int), ("ln_eps", ctypes.c_float)]

_lock = threading.Lock()
_lib = None
_dist = None


class QGemmError(RuntimeError):
    """A non-zero hipError_t returned through the C-ABI."""

    def __init__(self, fn: str, code: int):
        super().__init__(f"{fn} failed with hipError_t {code}")
        self.code = code


def build(verbose: bool = False) -> str:
    """Compile libqgemm.so and the harness binaries for gfx950 (hipcc; see Makefile)."""
    out = None if verbose else subprocess.DEVNULL
    jobs = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", PKG_DIR, "-j", jobs, "all"], check=True, stdout=out)
    return LIB_PATH


def load() -> ctypes.CDLL:
    """Load the HIP library (no fallback: raises if it was not built)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"qgemm HIP library not built: {LIB_PATH} missing (run build())")
        L = ctypes.CDLL(LIB_PATH)
        i64, i32, f32, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
        L.op_mm_quantize.argtypes = [vp, vp, vp, i32, i32, i32]
        L.op_mm_quantize.restype = i32
        L.op_mm_quantize_ex.argtypes = [vp, i64, i64, vp, i64, i64, vp, i64, i64, i32, i32, i32, f32, vp]
        L.op_mm_quantize_ex.restype = i32
        L.op_mm_quantize_workspace_size.argtypes = [i32, i32, i32]
        L.op_mm_quantize_workspace_size.restype = sz
        L.op_mm_quantize_ws.argtypes = [vp, i64, i64, vp, i64, i64, vp, i64, i64, i32, i32, i32, f32, vp, sz, vp]
        L.op_mm_quantize_ws.restype = i32
        L.qgemm_packed_size.argtypes = [i32, i32]
        L.qgemm_packed_size.restype = sz
        L.qgemm_pack_a.argtypes = [vp, i64, i64, i32, i32, f32, vp, vp]
        L.qgemm_pack_a.restype = i32
        L.qgemm_pack_b.argtypes = [vp, i64, i64, i32, i32, f32, vp, vp]
        L.qgemm_pack_b.restype = i32
        L.qgemm_mm_packed.argtypes = [vp, vp, vp, i64, i64, i32, i32, i32, f32, vp]
        L.qgemm_mm_packed.restype = i32
        L.qgemm_mm_packed_i32.argtypes = [vp, vp, vp, i32, i32, i32, vp]
        L.qgemm_mm_packed_i32.restype = i32
        L.qgemm_mm_fp32.argtypes = [vp, i64, i64, vp, i64, i64, vp, i64, i64, i32, i32, i32, vp]
        L.qgemm_mm_fp32.restype = i32
        L.qgemm_mm_fp32_plan.argtypes = [i32, i32, i32, i32, vp, i64, i64, i64, vp, i64, i64, i64,
                                         ctypes.POINTER(ctypes.c_char_p)]
        L.qgemm_mm_fp32_plan.restype = i32
        L.qgemm_error_stats.argtypes = [vp, vp, i64, i32, vp, vp]
        L.qgemm_error_stats.restype = i32
        L.qgemm_linear_workspace_size.argtypes = [i32, i32, i32]
        L.qgemm_linear_workspace_size.restype = sz
        L.qgemm_linear.argtypes = [vp, i64, i32, i32, vp, i32, vp, i32, vp, i64, vp, sz, vp]
        L.qgemm_linear.restype = i32
        L.qgemm_pack_a_dt.argtypes = [vp, i32, i64, i64, i32, i32, f32, vp, vp]
        L.qgemm_pack_a_dt.restype = i32
        L.qgemm_mm_packed_dt.argtypes = [vp, vp, vp, i32, i64, i64, i32, i32, i32, f32, vp]
        L.qgemm_mm_packed_dt.restype = i32
        L.qgemm_linear_dt.argtypes = [vp, i32, i64, i32, i32, vp, i32, vp, i32, vp, i32, i64, vp, sz, vp]
        L.qgemm_linear_dt.restype = i32
        L.op_mm_quantize_prepacked.argtypes = [vp, vp, vp, i32, i32, i32]
        L.op_mm_quantize_prepacked.restype = i32
        L.op_mm_quantize_prepacked_workspace_size.argtypes = [i32, i32, i32]
        L.op_mm_quantize_prepacked_workspace_size.restype = sz
        L.op_mm_quantize_prepacked_ws.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, vp, sz, vp]
        L.op_mm_quantize_prepacked_ws.restype = i32
        L.qgemm_softmax_rows.argtypes = [vp, vp, i64, i32, f32, vp]
        L.qgemm_softmax_rows.restype = i32
        L.qgemm_softmax_rows_causal.argtypes = [vp, vp, i64, i32, f32, i32, i32, vp]
        L.qgemm_softmax_rows_causal.restype = i32
        L.qgemm_add_layernorm_rows.argtypes = [vp, vp, vp, i64, i32, vp]
        L.qgemm_add_layernorm_rows.restype = i32
        L.qgemm_encoder_create.argtypes = [i32, i32, i32, i32, i32, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.qgemm_encoder_create.restype = i32
        L.qgemm_encoder_forward.argtypes = [vp, vp, vp, i32, vp]
        L.qgemm_encoder_forward.restype = i32
        L.qgemm_encoder_destroy.argtypes = [vp]
        L.qgemm_encoder_destroy.restype = i32
        L.qgemm_attention_workspace_size.argtypes = [i32, i32, i32, i32]
        L.qgemm_attention_workspace_size.restype = sz
        L.qgemm_attention.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, f32, vp, sz, vp]
        L.qgemm_attention.restype = i32
        L.qgemm_attention_causal.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, f32, i32, vp, sz,
                                             vp]
        L.qgemm_attention_causal.restype = i32
        L.qgemm_decoder_create_ex.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_uint64, i32, ctypes.POINTER(vp)]
        L.qgemm_decoder_create_ex.restype = i32
        L.qgemm_decoder_create.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.qgemm_decoder_create.restype = i32
        L.qgemm_decoder_forward.argtypes = [vp, vp, vp, vp, i32, i32, vp]
        L.qgemm_decoder_forward.restype = i32
        L.qgemm_decoder_begin.argtypes = [vp, vp, i32, vp]
        L.qgemm_decoder_begin.restype = i32
        L.qgemm_decoder_step.argtypes = [vp, vp, vp, i32, i32, vp]
        L.qgemm_decoder_step.restype = i32
        L.qgemm_attention_plan.argtypes = [i32, i32, i32, i32, ctypes.POINTER(ctypes.c_char_p)]
        L.qgemm_attention_plan.restype = i32
        L.qgemm_decoder_destroy.argtypes = [vp]
        L.qgemm_decoder_destroy.restype = i32
        ip = ctypes.POINTER(i32)
        L.qgemm_attention_decode_batched.argtypes = [vp, i64, vp, i64, i64, vp, i64, i64, vp, i64, i32, i32, ip, ip, ip,
                                                     i32, i32, f32, vp]
        L.qgemm_attention_decode_batched.restype = i32
        L.qgemm_decoder_create_slots.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_uint64, i32, i32,
                                                 ctypes.POINTER(vp)]
        L.qgemm_decoder_create_slots.restype = i32
        L.qgemm_decoder_begin_slot.argtypes = [vp, i32, vp, i32, vp]
        L.qgemm_decoder_begin_slot.restype = i32
        L.qgemm_decoder_step_slot.argtypes = [vp, i32, vp, vp, i32, i32, vp]
        L.qgemm_decoder_step_slot.restype = i32
        L.qgemm_decoder_step_batch.argtypes = [vp, i32, ip, ip, i32, vp, vp, vp]
        L.qgemm_decoder_step_batch.restype = i32
        L.qgemm_decoder_copy_slot.argtypes = [vp, i32, i32, vp]
        L.qgemm_decoder_copy_slot.restype = i32
        L.qgemm_decoder_slot_state.argtypes = [vp, i32, ip, ip]
        L.qgemm_decoder_slot_state.restype = i32
        lp = ctypes.POINTER(i64)
        L.qgemm_attention_varlen_workspace_size.argtypes = [i32, ip, ip, i32, i32]
        L.qgemm_attention_varlen_workspace_size.restype = sz
        L.qgemm_attention_varlen.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i32, lp, ip, lp, ip, ip, i32, i32, f32,
                                             vp, sz, vp]
        L.qgemm_attention_varlen.restype = i32
        L.qgemm_attention_varlen_plan.argtypes = [i32, ip, ip, i32, i32, ctypes.POINTER(ctypes.c_char_p)]
        L.qgemm_attention_varlen_plan.restype = i32
        L.qgemm_encoder_create_rows.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.qgemm_encoder_create_rows.restype = i32
        L.qgemm_encoder_forward_batch.argtypes = [vp, vp, vp, i32, ip, vp]
        L.qgemm_encoder_forward_batch.restype = i32
        L.qgemm_decoder_create_rows.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_uint64, i32, i32, i32,
                                                ctypes.POINTER(vp)]
        L.qgemm_decoder_create_rows.restype = i32
        L.qgemm_decoder_step_varlen.argtypes = [vp, i32, ip, ip, ip, vp, vp, vp]
        L.qgemm_decoder_step_varlen.restype = i32
        L.qgemm_argmax_rows_workspace_size.argtypes = [i64, i32]
        L.qgemm_argmax_rows_workspace_size.restype = sz
        L.qgemm_argmax_rows_plan.argtypes = [i64, i32, ip]
        L.qgemm_argmax_rows_plan.restype = i32
        L.qgemm_argmax_rows.argtypes = [vp, i64, i64, i32, vp, vp, vp, sz, vp]
        L.qgemm_argmax_rows.restype = i32
        L.qgemm_embed_rows.argtypes = [vp, i64, i32, i32, vp, vp, i64, i32, ip, i32, i32, vp, i64, vp]
        L.qgemm_embed_rows.restype = i32
        L.qgemm_head_create.argtypes = [vp, i32, i32, vp, vp, i64, vp, i64, i32, i32, ctypes.POINTER(vp)]
        L.qgemm_head_create.restype = i32
        L.qgemm_head_logits.argtypes = [vp, vp, i64, i32, vp, i64, vp]
        L.qgemm_head_logits.restype = i32
        L.qgemm_head_next_tokens.argtypes = [vp, vp, i64, i32, vp, vp]
        L.qgemm_head_next_tokens.restype = i32
        L.qgemm_head_embed.argtypes = [vp, vp, ip, i32, i32, vp, i64, vp]
        L.qgemm_head_embed.restype = i32
        L.qgemm_head_destroy.argtypes = [vp]
        L.qgemm_head_destroy.restype = i32
        L.qgemm_decoder_generate.argtypes = [vp, vp, i32, ip, vp, i32, ip, vp, vp]
        L.qgemm_decoder_generate.restype = i32
        u64 = ctypes.c_uint64
        L.qgemm_sample_rows_plan.argtypes = [i64, i32, i32, ip]
        L.qgemm_sample_rows_plan.restype = i32
        L.qgemm_sample_rows_workspace_size.argtypes = [i64, i32, i32]
        L.qgemm_sample_rows_workspace_size.restype = sz
        L.qgemm_sample_rows.argtypes = [vp, i64, i64, i32, i32, f32, f32, u64, u64, ctypes.POINTER(u64), vp, i32, vp,
                                        vp, vp, vp, vp, sz, vp]
        L.qgemm_sample_rows.restype = i32
        L.qgemm_head_sample_tokens.argtypes = [vp, vp, i64, i32, i32, f32, f32, u64, u64, ctypes.POINTER(u64), vp, i32,
                                               vp, vp]
        L.qgemm_head_sample_tokens.restype = i32
        L.qgemm_decoder_generate_sampled.argtypes = [vp, vp, i32, ip, vp, i32, ip, i32, f32, f32, u64,
                                                     ctypes.POINTER(ctypes.c_uint32), i32, vp, vp]
        L.qgemm_decoder_generate_sampled.restype = i32
        L.qgemm_logsumexp_rows_plan.argtypes = [i64, i32, ip]
        L.qgemm_logsumexp_rows_plan.restype = i32
        L.qgemm_logsumexp_rows_workspace_size.argtypes = [i64, i32]
        L.qgemm_logsumexp_rows_workspace_size.restype = sz
        L.qgemm_logsumexp_rows.argtypes = [vp, i64, i64, i32, vp, vp, vp, sz, vp]
        L.qgemm_logsumexp_rows.restype = i32
        L.qgemm_beam_step_plan.argtypes = [i32, i32, i32, ip, ip]
        L.qgemm_beam_step_plan.restype = i32
        L.qgemm_beam_step_workspace_size.argtypes = [i32, i32, i32]
        L.qgemm_beam_step_workspace_size.restype = sz
        L.qgemm_beam_step.argtypes = [vp, i64, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]
        L.qgemm_beam_step.restype = i32
        L.qgemm_head_beam_step.argtypes = [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp, vp, vp]
        L.qgemm_head_beam_step.restype = i32
        L.qgemm_decoder_gather_slots.argtypes = [vp, i32, i32, ip, ip, vp, ip, vp]
        L.qgemm_decoder_gather_slots.restype = i32
        L.qgemm_decoder_read_slot.argtypes = [vp, i32, i32, vp, vp, vp]
        L.qgemm_decoder_read_slot.restype = i32
        L.qgemm_decoder_generate_beam.argtypes = [vp, vp, i32, i32, ip, ip, vp, i32, ip, vp, i32, vp, vp, vp, vp]
        L.qgemm_decoder_generate_beam.restype = i32
        L.qgemm_attention_decode_indirect.argtypes = [vp, i64, vp, i64, i64, vp, i64, i64, vp, i64, i32, i32, vp, i64,
                                                      i32, ip, ip, ip, i32, i32, f32, vp]
        L.qgemm_attention_decode_indirect.restype = i32
        L.qgemm_beam_reindex.argtypes = [vp, i64, i32, i32, ip, vp, ip, vp]
        L.qgemm_beam_reindex.restype = i32
        L.qgemm_decoder_beam_begin.argtypes = [vp, i32, i32, ip, ip, ip, vp]
        L.qgemm_decoder_beam_begin.restype = i32
        L.qgemm_decoder_step_batch_indirect.argtypes = [vp, i32, ip, ip, ip, i32, vp, vp, vp]
        L.qgemm_decoder_step_batch_indirect.restype = i32
        L.qgemm_decoder_beam_reindex.argtypes = [vp, i32, i32, ip, vp, ip, vp]
        L.qgemm_decoder_beam_reindex.restype = i32
        L.qgemm_decoder_read_beam_table.argtypes = [vp, vp, vp]
        L.qgemm_decoder_read_beam_table.restype = i32
        L.qgemm_decoder_generate_beam_indirect.argtypes = [vp, vp, i32, i32, ip, ip, vp, i32, ip, vp, i32, vp, vp, vp,
                                                           vp]
        L.qgemm_decoder_generate_beam_indirect.restype = i32
        L.qgemm_pack_b_window.argtypes = [vp, i32, i64, i64, i32, i32, i32, i32, f32, vp, vp]
        L.qgemm_pack_b_window.restype = i32
        L.qgemm_pack_b_window_plan.argtypes = [vp, i32, i64, i64, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_char_p)]
        L.qgemm_pack_b_window_plan.restype = i32
        L.qgemm_model_weight_shape.argtypes = [vp, i32, ip, ip, ip]
        L.qgemm_model_weight_shape.restype = i32
        L.qgemm_model_set_weight.argtypes = [vp, i32, i32, i32, vp, i32, i64, i64, vp]
        L.qgemm_model_set_weight.restype = i32
        L.qgemm_model_packed_weight.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ip, ip]
        L.qgemm_model_packed_weight.restype = i32
        L.qgemm_model_bias.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ip]
        L.qgemm_model_bias.restype = i32
        L.qgemm_mm_outlier_workspace_size.argtypes = [i32, i32, i32]
        L.qgemm_mm_outlier_workspace_size.restype = sz
        L.qgemm_mm_outlier.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, sz, vp]
        L.qgemm_mm_outlier.restype = i32
        L.qgemm_outlier_count.argtypes = [i32, vp, ctypes.POINTER(i32)]
        L.qgemm_outlier_count.restype = i32
        L.qgemm_linear_outlier_workspace_size.argtypes = [i32, i32, i32]
        L.qgemm_linear_outlier_workspace_size.restype = sz
        L.qgemm_linear_outlier.argtypes = [vp, i64, i32, i32, vp, i32, vp, i32, f32, vp, i64, vp, sz, vp]
        L.qgemm_linear_outlier.restype = i32
        L.qgemm_fill_uniform.argtypes = [vp, i64, ctypes.c_uint64, f32, f32, vp]
        L.qgemm_fill_uniform.restype = i32
        L.qgemm_set_gemm_events.argtypes = [vp, vp]
        L.qgemm_set_gemm_events.restype = i32
        L.qgemm_set_event_mode.argtypes = [i32]
        L.qgemm_set_event_mode.restype = i32
        L.qgemm_gemm_plan.argtypes = [i32, i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_char_p)]
        L.qgemm_gemm_plan.restype = i32
        L.qgemm_version.argtypes = []
        L.qgemm_version.restype = ctypes.c_char_p
        L.qgemm_layernorm_rows.argtypes = [vp, vp, vp, vp, f32, vp, i64, i32, vp]
        L.qgemm_layernorm_rows.restype = i32
        L.qgemm_layernorm_pack_a.argtypes = [vp, vp, vp, vp, f32, vp, i64, i32, f32, vp, vp]
        L.qgemm_layernorm_pack_a.restype = i32
        L.qgemm_gelu_rows.argtypes = [vp, i64, vp, i64, i64, i32, vp]
        L.qgemm_gelu_rows.restype = i32
        L.qgemm_gelu_pack_a.argtypes = [vp, i64, i32, i32, f32, vp, vp]
        L.qgemm_gelu_pack_a.restype = i32
        L.qgemm_model_create.argtypes = [ctypes.POINTER(ModelDesc), ctypes.POINTER(vp)]
        L.qgemm_model_create.restype = i32
        L.qgemm_model_info.argtypes = [vp, ctypes.POINTER(ModelDesc)]
        L.qgemm_model_info.restype = i32
        L.qgemm_prenorm_pack_a.argtypes = [vp, vp, vp, vp, f32, vp, i64, i32, f32, vp, vp]
        L.qgemm_prenorm_pack_a.restype = i32
        L.qgemm_add_rows.argtypes = [vp, vp, vp, i64, i32, vp]
        L.qgemm_add_rows.restype = i32
        L.qgemm_decoder_slot_begun.argtypes = [vp, i32, ip]
        L.qgemm_decoder_slot_begun.restype = i32
        L.qgemm_model_rope_tables.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ip, ip]
        L.qgemm_model_rope_tables.restype = i32
        L.qgemm_rope_rows.argtypes = [vp, i64, i64, i32, i32, vp, vp, i32, i32, vp]
        L.qgemm_rope_rows.restype = i32
        L.qgemm_rope_rows_varlen.argtypes = [vp, i64, i32, i32, vp, vp, i32, i32, lp, ip, ip, vp]
        L.qgemm_rope_rows_varlen.restype = i32
        L.qgemm_rmsnorm_rows.argtypes = [vp, vp, vp, f32, vp, i64, i32, vp]
        L.qgemm_rmsnorm_rows.restype = i32
        L.qgemm_rmsnorm_pack_a.argtypes = [vp, vp, vp, f32, vp, i64, i32, f32, vp, vp]
        L.qgemm_rmsnorm_pack_a.restype = i32
        L.qgemm_prenorm_rms_pack_a.argtypes = [vp, vp, vp, f32, vp, i64, i32, f32, vp, vp]
        L.qgemm_prenorm_rms_pack_a.restype = i32
        L.qgemm_glu_rows.argtypes = [vp, i64, vp, i64, i64, i32, i32, vp]
        L.qgemm_glu_rows.restype = i32
        L.qgemm_glu_pack_a.argtypes = [vp, i64, i32, i32, i32, f32, vp, vp]
        L.qgemm_glu_pack_a.restype = i32
        _lib = L
        return L


def load_dist() -> ctypes.CDLL:
    """Load libqgemm_dist.so (M-sharded calls + the RCCL all-gather; no fallback)."""
    global _dist
    load()
    with _lock:
        if _dist is not None:
            return _dist
        if not os.path.exists(DIST_LIB_PATH):
            raise RuntimeError(f"qgemm multi-GPU library not built: {DIST_LIB_PATH} missing (run build())")
        D = ctypes.CDLL(DIST_LIB_PATH)
        i32, vp = ctypes.c_int, ctypes.c_void_p
        D.qgemm_shard_rows.argtypes = [i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        D.qgemm_shard_rows.restype = i32
        D.op_mm_quantize_shard.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
        D.op_mm_quantize_shard.restype = i32
        D.qgemm_comm_unique_id.argtypes = [vp]
        D.qgemm_comm_unique_id.restype = i32
        D.qgemm_comm_init_rank.argtypes = [ctypes.POINTER(vp), i32, vp, i32]
        D.qgemm_comm_init_rank.restype = i32
        D.qgemm_comm_init_all.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(i32)]
        D.qgemm_comm_init_all.restype = i32
        D.qgemm_comm_destroy.argtypes = [vp]
        D.qgemm_comm_destroy.restype = i32
        D.qgemm_comm_count.argtypes = [vp, ctypes.POINTER(i32)]
        D.qgemm_comm_count.restype = i32
        D.qgemm_comm_user_rank.argtypes = [vp, ctypes.POINTER(i32)]
        D.qgemm_comm_user_rank.restype = i32
        D.qgemm_allgather_rows.argtypes = [vp, i32, i32, i32, i32, vp, vp]
        D.qgemm_allgather_rows.restype = i32
        i64p = ctypes.POINTER(ctypes.c_int64)
        D.qgemm_allgather_plan.argtypes = [i32, i32, i32, i64p, i64p, ctypes.POINTER(i32), i32]
        D.qgemm_allgather_plan.restype = i32
        D.qgemm_allgather_chunk_plan.argtypes = [i32, i32, i32, i32, i64p, i64p, ctypes.POINTER(i32), i32]
        D.qgemm_allgather_chunk_plan.restype = i32
        D.op_mm_quantize_shard_pipelined_workspace_size.argtypes = [i32, i32, i32, i32, i32]
        D.op_mm_quantize_shard_pipelined_workspace_size.restype = ctypes.c_size_t
        D.op_mm_quantize_shard_pipelined.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, ctypes.c_size_t,
                                                     vp, vp]
        D.op_mm_quantize_shard_pipelined.restype = i32
        D.qgemm_node_allgather_plan.argtypes = [i32, i32, i32, ctypes.POINTER(CollOp), i32]
        D.qgemm_node_allgather_plan.restype = i32
        D.qgemm_node_mm_quantize.argtypes = [vp, vp, vp, i32, i32, i32, i32, ctypes.POINTER(i32), vp, vp, i32]
        D.qgemm_node_mm_quantize.restype = i32
        _dist = D
        return D


def shard_rows(m: int, world: int, rank: int) -> tuple:
    """(m0, rows) of rank's contiguous row shard (qgemm_shard_rows)."""
    m0, rows = ctypes.c_int(), ctypes.c_int()
    _check("qgemm_shard_rows", load_dist().qgemm_shard_rows(m, world, rank, ctypes.byref(m0), ctypes.byref(rows)))
    return m0.value, rows.value


class CollOp(ctypes.Structure):
    """qgemm_coll_op (include/qgemm_dist.h): one planned collective of the one-process node path."""
    _fields_ = [("rank", ctypes.c_int), ("root", ctypes.c_int), ("send_off", ctypes.c_int64),
                ("recv_off", ctypes.c_int64), ("count", ctypes.c_int64)]


def node_allgather_plan(m: int, n: int, ndev: int) -> list:
    """The collectives qgemm_node_mm_quantize enqueues in its ONE RCCL group, in issue order, as
    [(rank, root, send_off, recv_off, count)] (root -1: in-place all-gather; else an in-place broadcast)."""
    D = load_dist()
    cnt = D.qgemm_node_allgather_plan(m, n, ndev, None, 0)
    if cnt < 0:
        raise QGemmError("qgemm_node_allgather_plan", -cnt)
    ops = (CollOp * max(1, cnt))()
    got = D.qgemm_node_allgather_plan(m, n, ndev, ops, cnt)
    if got != cnt:
        raise QGemmError("qgemm_node_allgather_plan", -got if got < 0 else 1)
    return [(o.rank, o.root, o.send_off, o.recv_off, o.count) for o in ops[:cnt]]


def allgather_plan(m: int, n: int, world: int) -> list:
    """The collectives qgemm_allgather_rows enqueues for an m x n C over `world` ranks, as
    [(first, count, root)]: root -1 = one in-place all-gather of `count` floats per rank starting at
    element `first`; root >= 0 = an in-place broadcast of [first, first + count) from that rank."""
    cap = max(1, world)
    first, count, root = (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int * cap)()
    ops = load_dist().qgemm_allgather_plan(m, n, world, first, count, root, cap)
    if ops < 0:
        raise QGemmError("qgemm_allgather_plan", -ops)
    return [(first[i], count[i], root[i]) for i in range(ops)]


def allgather_chunk_plan(m: int, n: int, world: int, chunks: int) -> list:
    """The broadcasts op_mm_quantize_shard_pipelined issues, chunk-major, as [(first, count, root)]
    (qgemm_allgather_chunk_plan): each moves `count` floats at element `first` of C from rank `root`."""
    D = load_dist()
    cnt = D.qgemm_allgather_chunk_plan(m, n, world, chunks, None, None, None, 0)
    if cnt < 0:
        raise QGemmError("qgemm_allgather_chunk_plan", -cnt)
    cap = max(1, cnt)
    first, count, root = (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int * cap)()
    got = D.qgemm_allgather_chunk_plan(m, n, world, chunks, first, count, root, cap)
    if got != cnt:
        raise QGemmError("qgemm_allgather_chunk_plan", -got if got < 0 else 1)
    return [(first[i], count[i], root[i]) for i in range(cnt)]


def op_mm_quantize_shard_pipelined(A, B, C, world: int, rank: int, chunks: int, comm=None, gather_stream=None,
                                   workspace=None) -> None:
    """op_mm_quantize_shard with the all-gather of C pipelined under the chunks' compute
    (op_mm_quantize_shard_pipelined): on return (stream order) every rank's C holds all rows."""
    import torch
    for t, nm in ((A, "A"), (B, "B"), (C, "C")):
        _require_device_f32(t, nm)
        assert t.is_contiguous(), f"{nm} must be contiguous row-major"
    M, K = A.shape
    N = B.shape[1]
    assert B.shape[0] == K and C.shape == (M, N), "A m x k, B k x n, C m x n"
    D = load_dist()
    need = D.op_mm_quantize_shard_pipelined_workspace_size(M, N, K, world, chunks)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=A.device)
    assert workspace.numel() >= need, "workspace too small"
    s = _stream(A.device)
    g = ctypes.c_void_p(gather_stream.cuda_stream) if gather_stream is not None else s  # a torch.cuda.Stream
    _check("op_mm_quantize_shard_pipelined",
           D.op_mm_quantize_shard_pipelined(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, world, rank, chunks,
                                            comm.handle if comm is not None else None, workspace.data_ptr(),
                                            workspace.numel(), s, g))


def op_mm_quantize_shard(A, B, C, world: int, rank: int) -> None:
    """Rows [m0, m0 + rows) of C = op_mm_quantize(A, B) on this rank (per-rank pointer offsets into the
    full row-major A and C; bit-identical to those rows of the one-GPU call)."""
    for t, nm in ((A, "A"), (B, "B"), (C, "C")):
        _require_device_f32(t, nm)
        assert t.is_contiguous(), f"{nm} must be contiguous row-major"
    M, K = A.shape
    N = B.shape[1]
    assert B.shape[0] == K and C.shape == (M, N), "A m x k, B k x n, C m x n"
    _check("op_mm_quantize_shard", load_dist().op_mm_quantize_shard(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K,
                                                                    world, rank, _stream(A.device)))


class Comm:
    """An RCCL communicator of libqgemm_dist.so (one rank per process, or world == 1 alone)."""

    def __init__(self, world: int, rank: int, unique_id: bytes):
        assert len(unique_id) == COMM_ID_BYTES
        self.world, self.rank = world, rank
        self._id = ctypes.create_string_buffer(unique_id, COMM_ID_BYTES)
        self.handle = ctypes.c_void_p()
        _check("qgemm_comm_init_rank",
               load_dist().qgemm_comm_init_rank(ctypes.byref(self.handle), world, self._id, rank))

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        _check("qgemm_comm_unique_id", load_dist().qgemm_comm_unique_id(buf))
        return buf.raw

    def allgather_rows(self, C) -> None:
        """In place: every rank's row shard of the full C (m x n) to every rank (qgemm_allgather_rows)."""
        _require_device_f32(C, "C")
        assert C.is_contiguous()
        _check("qgemm_allgather_rows", load_dist().qgemm_allgather_rows(C.data_ptr(), C.shape[0], C.shape[1], self.world,
                                                                        self.rank, self.handle, _stream(C.device)))

    def count(self) -> int:
        """The communicator's size as RCCL reports it (ncclCommCount)."""
        c = ctypes.c_int(-1)
        _check("qgemm_comm_count", load_dist().qgemm_comm_count(self.handle, ctypes.byref(c)))
        return c.value

    def user_rank(self) -> int:
        r = ctypes.c_int(-1)
        _check("qgemm_comm_user_rank", load_dist().qgemm_comm_user_rank(self.handle, ctypes.byref(r)))
        return r.value

    def close(self) -> None:
        if self.handle:
            _check("qgemm_comm_destroy", load_dist().qgemm_comm_destroy(self.handle))
            self.handle = ctypes.c_void_p()


def version() -> str:
    return load().qgemm_version().decode()


def source_hash() -> str:
    """The Makefile's SRC_HASH recomputed from this tree: sha256 of the Makefile, csrc/*.{hip,h,cpp}, include/*.h and
    the harness sources src/*.cpp, src/*/*.{h,cuh}
    concatenated in sorted path order (make's $(sort) of the same relative paths), first 16 hex digits."""
    import glob
    import hashlib
    rel = ["Makefile"]
    for pat in ("csrc/*.hip", "csrc/*.h", "csrc/*.cpp", "../include/*.h", "src/*.cpp", "src/*.hip", "src/*/*.h",
                "src/*/*.cuh"):
        rel += [os.path.relpath(p, PKG_DIR) for p in glob.glob(os.path.join(PKG_DIR, pat))]
    h = hashlib.sha256()
    for r in sorted(rel):
        with open(os.path.join(PKG_DIR, r), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def binary_hash() -> str:
    """The source hash compiled into the loaded libqgemm.so (the `src=` field of qgemm_version())."""
    for field in version().split():
        if field.startswith("src="):
            return field[4:]
    return "none"


def file_hash(path: str = LIB_PATH) -> str:
    """The source hash tagged inside a built libqgemm.so, read from the file (no dlopen): "" if absent."""
    import re
    try:
        with open(path, "rb") as f:
            m = re.search(rb"QGEMM_SRC_HASH=([0-9a-f]{16})", f.read())
    except OSError:
        return ""
    return m.group(1).decode() if m else ""


def check_binary() -> str:
    """Refuse a libqgemm.so built from other sources than this tree's (a stale build/ shipped with the
    snapshot): returns the hash, raises RuntimeError on a mismatch."""
    want, got = source_hash(), binary_hash()
    if got != want:
        raise RuntimeError(f"{LIB_PATH} was built from sources src={got}, this tree is src={want}: rebuild "
                           "(make -C quantized-gemm-for-transformer-inference_amd all)")
    return got


def _check(fn: str, rc: int) -> None:
    if rc != 0:
        raise QGemmError(fn, rc)


def _stream(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_device_f32(t, name):
    import torch
    assert isinstance(t, torch.Tensor) and t.dim() == 2, f"{name} must be a 2-D tensor"
    assert t.is_cuda, f"{name}.on_device (op_mm.cuh:72)"
    assert t.dtype == torch.float32, f"{name} must be float32 (op_quantized_mm is instantiated at T=float)"


def _require_device_act(t, name) -> int:
    """An activation / output of the prepacked path: fp32 or bf16.  Returns its element-type tag."""
    import torch
    if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16:
        assert t.dim() == 2, f"{name} must be a 2-D tensor"
        assert t.is_cuda, f"{name}.on_device (op_mm.cuh:72)"
        return QGEMM_BF16
    _require_device_f32(t, name)
    return QGEMM_F32


def _out_dtype(out, out_dtype, default):
    """The output type of mm_packed / linear: a given output tensor decides, then out_dtype, then `default`."""
    import torch
    if out is not None:
        assert out_dtype is None or out_dtype == out.dtype, "out_dtype disagrees with the output tensor given"
        return out.dtype
    dt = default if out_dtype is None else out_dtype
    assert dt in (torch.float32, torch.bfloat16), "out_dtype must be torch.float32 or torch.bfloat16"
    return dt


# ------------------------------------------------------------------------------- the operator
def op_quantized_mm(X, W, O, range: float = DEFAULT_RANGE) -> None:  # noqa: A002 - reference name
    """O = quantized X @ W, in place -- the reference's ``op_quantized_mm<float>`` (op_mm.cuh:67-101).

    Same argument meaning and the same asserts (op_mm.cuh:71-72): ``X.h == O.h && W.w == O.w &&
    X.w == W.h`` and all three on the device.  Strided/transposed views are accepted, as the
    reference's Index() macro accepts them.  Enqueued on torch's current stream.
    """
    for t, nm in ((X, "X"), (W, "W"), (O, "O")):
        _require_device_f32(t, nm)
    assert X.shape[0] == O.shape[0] and W.shape[1] == O.shape[1] and X.shape[1] == W.shape[0], \
        "X.h == O.h && W.w == O.w && X.w == W.h (op_mm.cuh:71)"
    M, K = X.shape
    N = W.shape[1]
    if M == 0 or N == 0:
        return
    rc = load().op_mm_quantize_ex(X.data_ptr(), X.stride(0), X.stride(1), W.data_ptr(), W.stride(0), W.stride(1),
                                  O.data_ptr(), O.stride(0), O.stride(1), M, N, K, float(range), _stream(X.device))
    _check("op_mm_quantize_ex", rc)


def op_mm_quantize(A, B, C=None):
    """The north-star C-ABI op_mm_quantize(A, B, C, M, N, K) on contiguous row-major tensors."""
    import torch
    _require_device_f32(A, "A")
    _require_device_f32(B, "B")
    M, K = A.shape
    N = B.shape[1]
    if C is None:
        C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    op_quantized_mm(A, B, C, DEFAULT_RANGE)
    return C


# ------------------------------------------------------------------------- packed operands
def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class Packed:
    """A packed (quantized, MFMA-ready) operand: [scale f32][reserved u32 partials][q int8, rows_pad x k_pad]."""

    def __init__(self, buf, rows: int, k: int, range_: float):
        self.buf, self.rows, self.k, self.range = buf, rows, k, range_
        self.rows_pad, self.k_pad = _round_up(rows, ROW_PAD), _round_up(k, K_PAD)

    @property
    def scale(self):
        """Cx (for A) or Cw (for B), padded to rows_pad."""
        import torch
        return self.buf[: 4 * self.rows_pad].view(torch.float32)

    @property
    def q_raw(self):
        """The packed bytes as stored: FRAGMENT-MAJOR (csrc/qgemm_internal.h fofs) -- 1-KiB blocks of 16
        rows x 64 k in MFMA lane order, block (rg, kb) at (rg * k_pad / 64 + kb) * 1024."""
        import torch
        parts = -(-(self.k - 1) // 256) if self.k > 1 else 1
        off = _round_up(4 * self.rows_pad * (1 + parts), 256)
        return self.buf[off: off + self.rows_pad * self.k_pad].view(torch.int8)

    @property
    def q(self):
        """X_int8 (rows_pad x k_pad) or W_int8^T (n_pad x k_pad), zero padded, row-major -- a COPY, un-permuted
        from the fragment-major storage ([rg][kb][kc][r][16 B] -> [rg][r][kb][kc][16 B]): writes into it do not
        reach the packed buffer; in-place edits go through q_raw."""
        r16, kb = self.rows_pad // 16, self.k_pad // 64
        return (self.q_raw.view(r16, kb, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(self.rows_pad, self.k_pad))


def _alloc_packed(rows, k, device):
    import torch
    nbytes = load().qgemm_packed_size(rows, k)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def pack_a(A, range: float = DEFAULT_RANGE) -> Packed:  # noqa: A002
    """Cx = absmax rows (op_mm.cuh:76-77) and X_int8 (op_mm.cuh:82-87), fused.  A bf16 A is widened exactly
    on the way in (qgemm_pack_a_dt): the packed operand is that of A.float()."""
    tag = _require_device_act(A, "A")
    M, K = A.shape
    p = Packed(_alloc_packed(M, K, A.device), M, K, range)
    if tag == QGEMM_F32:
        _check("qgemm_pack_a", load().qgemm_pack_a(A.data_ptr(), A.stride(0), A.stride(1), M, K, float(range),
                                                  p.buf.data_ptr(), _stream(A.device)))
    else:
        _check("qgemm_pack_a_dt", load().qgemm_pack_a_dt(A.data_ptr(), tag, A.stride(0), A.stride(1), M, K,
                                                        float(range), p.buf.data_ptr(), _stream(A.device)))
    return p


def pack_b(B, range: float = DEFAULT_RANGE) -> Packed:  # noqa: A002
    """Cw = absmax columns (op_mm.cuh:78-79) and W_int8 (op_mm.cuh:84-89), stored transposed."""
    _require_device_f32(B, "B")
    K, N = B.shape
    p = Packed(_alloc_packed(N, K, B.device), N, K, range)
    _check("qgemm_pack_b", load().qgemm_pack_b(B.data_ptr(), B.stride(0), B.stride(1), K, N, float(range),
                                              p.buf.data_ptr(), _stream(B.device)))
    return p


def _window_source(B, layout: str, name: str):
    """A weight tensor given as "kn" ([in, out]: rows along k) or "nk" ([out, in], a checkpoint's layout): its
    element-type tag, k, the number of columns and the element strides along k and along the columns."""
    tag = _require_device_act(B, name)
    assert layout in ("kn", "nk"), 'layout is "kn" ([in, out]) or "nk" ([out, in])'
    if layout == "kn":
        return tag, B.shape[0], B.shape[1], B.stride(0), B.stride(1)
    return tag, B.shape[1], B.shape[0], B.stride(1), B.stride(0)


def pack_b_window(B, packed: Packed, col0: int, layout: str = "kn", range: float = DEFAULT_RANGE) -> Packed:  # noqa: A002
    """Pack B -- fp32 or bf16, k x ncols as layout "kn" or ncols x k as "nk", any strides -- into columns col0 ..
    col0 + ncols - 1 of `packed`, a packed k x n weight (qgemm_pack_b_window): those columns' scales and packed rows
    become, bit for bit, what pack_b writes for them; no other scale or q byte changes.  One launch, in place."""
    tag, K, ncols, sh, sw = _window_source(B, layout, "B")
    assert K == packed.k, "B's k is the packed weight's"
    _check("qgemm_pack_b_window",
           load().qgemm_pack_b_window(B.data_ptr(), tag, sh, sw, K, packed.rows, int(col0), ncols, float(range),
                                      packed.buf.data_ptr(), _stream(B.device)))
    return packed


def pack_b_window_plan(B, packed: Packed, col0: int, layout: str = "kn") -> str:
    """The source path pack_b_window takes for this tensor (qgemm_pack_b_window_plan): nothing is launched."""
    tag, K, ncols, sh, sw = _window_source(B, layout, "B")
    name = ctypes.c_char_p()
    _check("qgemm_pack_b_window_plan",
           load().qgemm_pack_b_window_plan(B.data_ptr(), tag, sh, sw, K, packed.rows, int(col0), ncols,
                                           ctypes.byref(name)))
    return name.value.decode()


def mm_packed(pa: Packed, pb: Packed, C=None, out_dtype=None):
    """int8 MFMA GEMM + fused dequantize (op_mm.cuh:92-99) on packed operands.  The output is fp32 unless a bf16 C
    or out_dtype=torch.bfloat16 is given: then each fp32 result is rounded once to bf16 (qgemm_mm_packed_dt)."""
    import torch
    assert pa.k == pb.k, "X.w == W.h"
    if C is None:
        C = torch.empty((pa.rows, pb.rows), dtype=_out_dtype(None, out_dtype, torch.float32), device=pa.buf.device)
    else:
        _out_dtype(C, out_dtype, None)
    tag = _require_device_act(C, "C")
    assert C.shape == (pa.rows, pb.rows)
    if tag == QGEMM_F32:
        _check("qgemm_mm_packed", load().qgemm_mm_packed(pa.buf.data_ptr(), pb.buf.data_ptr(), C.data_ptr(),
                                                        C.stride(0), C.stride(1), pa.rows, pb.rows, pa.k,
                                                        float(pa.range), _stream(C.device)))
    else:
        _check("qgemm_mm_packed_dt", load().qgemm_mm_packed_dt(pa.buf.data_ptr(), pb.buf.data_ptr(), C.data_ptr(), tag,
                                                              C.stride(0), C.stride(1), pa.rows, pb.rows, pa.k,
                                                              float(pa.range), _stream(C.device)))
    return C


def mm_packed_i32(pa: Packed, pb: Packed):
    """The raw int32 accumulator O_int32 (op_mm.cuh:92-93)."""
    import torch
    acc = torch.empty((pa.rows, pb.rows), dtype=torch.int32, device=pa.buf.device)
    _check("qgemm_mm_packed_i32", load().qgemm_mm_packed_i32(pa.buf.data_ptr(), pb.buf.data_ptr(), acc.data_ptr(),
                                                            pa.rows, pb.rows, pa.k, _stream(acc.device)))
    return acc


def mm_fp32(A, B, C=None):
    """The reference's unquantized op_mm<float,float> (op_mm.cuh:49-65), bit-exact, on the GPU.  Any views of A, B and
    C inside qgemm_mm_fp32's stride envelope (include/qgemm.h: no negative stride, a tile's offsets below 2^31 bytes);
    QGemmError outside it.  mm_fp32_plan names the kernel a call takes."""
    import torch
    _require_device_f32(A, "A")
    _require_device_f32(B, "B")
    M, K = A.shape
    N = B.shape[1]
    assert B.shape[0] == K
    if C is None:
        C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    _check("qgemm_mm_fp32", load().qgemm_mm_fp32(A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(), B.stride(0),
                                                B.stride(1), C.data_ptr(), C.stride(0), C.stride(1), M, N, K,
                                                _stream(A.device)))
    return C


def mm_fp32_plan(m: int, n: int, k: int, a_stride, b_stride, batch: int = 1, a_batch_stride: int = 0,
                 b_batch_stride: int = 0, a_ptr: int = 0, b_ptr: int = 0) -> str:
    """The kernel mm_fp32 -- or one batched GEMM of attention's three launches -- takes for a call
    (qgemm_mm_fp32_plan): "mm_f32_dma_<tile>_bkc" / "_bnc" or "mm_f32_mfma_<tile>".  a_stride and b_stride are
    (stride_h, stride_w) in floats, as torch's Tensor.stride(); a_ptr and b_ptr are read for their 16-byte alignment
    only (Tensor.data_ptr(); 0 stands for an aligned base).  Needs no GPU; raises QGemmError for dimensions < 1."""
    name = ctypes.c_char_p()
    _check("qgemm_mm_fp32_plan",
           load().qgemm_mm_fp32_plan(m, n, k, batch, a_ptr, a_stride[0], a_stride[1], a_batch_stride, b_ptr,
                                     b_stride[0], b_stride[1], b_batch_stride, ctypes.byref(name)))
    return name.value.decode()


def error_stats(C, O, reference_order: bool = False) -> dict:
    """Quantization error of O against the unquantized C, on the device (qgemm_error_stats).

    signed_mean_ref is the reference's printed metric (timing_quantize.cu:67-70 via tensor.cuh:201-211,
    sequential fp32) -- only with reference_order=True (one GPU lane, slow at large sizes)."""
    import torch
    _require_device_f32(C, "C")
    _require_device_f32(O, "O")
    assert C.shape == O.shape and C.is_contiguous() and O.is_contiguous()
    st = torch.empty(5, dtype=torch.float64, device=C.device)
    _check("qgemm_error_stats", load().qgemm_error_stats(C.data_ptr(), O.data_ptr(), C.numel(),
                                                        1 if reference_order else 0, st.data_ptr(),
                                                        _stream(C.device)))
    v = st.cpu().tolist()
    return dict(signed_mean_ref=v[0], signed_mean=v[1], mean_abs=v[2], max_abs=v[3],
                rel=v[2] / v[4] if v[4] else float("nan"))


def linear(X, pw: Packed, bias=None, relu: bool = False, Y=None, out_dtype=None):
    """LinearLayer.forward on the quantized path (linear.cuh:50-54): quantized_mm(X, W) [+ b] [relu],
    W packed once by pack_b.  X and Y are fp32 or bf16, independently (qgemm_linear_dt): a given Y decides the
    output type, then out_dtype, then X's own type.  bias stays fp32."""
    import torch
    xt = _require_device_act(X, "X")
    assert X.stride(1) == 1 and X.shape[1] == pw.k
    assert pw.range == DEFAULT_RANGE, f"qgemm_linear needs a weight packed with range {DEFAULT_RANGE}"
    M, K = X.shape
    N = pw.rows
    if Y is None:
        Y = torch.empty((M, N), dtype=_out_dtype(None, out_dtype, X.dtype), device=X.device)
    else:
        _out_dtype(Y, out_dtype, None)
    yt = _require_device_act(Y, "Y")
    assert Y.shape == (M, N) and Y.stride(1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32, "bias stays float32"
    L = load()
    ws = torch.empty(max(1, L.qgemm_linear_workspace_size(M, N, K)), dtype=torch.uint8, device=X.device)
    b = 0 if bias is None else bias.data_ptr()
    if xt == QGEMM_F32 and yt == QGEMM_F32:
        _check("qgemm_linear", L.qgemm_linear(X.data_ptr(), X.stride(0), M, K, pw.buf.data_ptr(), N, b,
                                              1 if relu else 0, Y.data_ptr(), Y.stride(0), ws.data_ptr(), ws.numel(),
                                              _stream(X.device)))
    else:
        _check("qgemm_linear_dt", L.qgemm_linear_dt(X.data_ptr(), xt, X.stride(0), M, K, pw.buf.data_ptr(), N, b,
                                                    1 if relu else 0, Y.data_ptr(), yt, Y.stride(0), ws.data_ptr(),
                                                    ws.numel(), _stream(X.device)))
    return Y


def op_mm_quantize_prepacked(A, pb: Packed, C=None):
    """The weight-cache drop-in: C = op_quantized_mm(A, W) with W packed once by
    pack_b; A quantized on every call (op_mm.cuh:76-77, 82-87), then the int8 GEMM + dequantize."""
    import torch
    _require_device_f32(A, "A")
    assert A.stride(1) == 1 and A.shape[1] == pb.k, "X.w == W.h"
    # the C entry point quantizes A with range 127 and dequantizes with 1/127^2: a B packed with another
    # range would silently differ from op_mm_quantize
    assert pb.range == DEFAULT_RANGE, f"op_mm_quantize_prepacked needs a B packed with range {DEFAULT_RANGE}"
    M, K = A.shape
    N = pb.rows
    if C is None:
        C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    assert C.shape == (M, N) and C.stride(1) == 1
    L = load()
    ws = torch.empty(max(1, L.op_mm_quantize_prepacked_workspace_size(M, N, K)), dtype=torch.uint8, device=A.device)
    _check("op_mm_quantize_prepacked_ws",
           L.op_mm_quantize_prepacked_ws(A.data_ptr(), A.stride(0), pb.buf.data_ptr(), C.data_ptr(), C.stride(0), M, N,
                                         K, ws.data_ptr(), ws.numel(), _stream(A.device)))
    return C


def softmax_rows(S, scale: float = 1.0, P=None):
    """op_multiply(S, scale) + op_softmax (attention.cuh:65-68) over the rows of a contiguous S."""
    import torch
    _require_device_f32(S, "S")
    assert S.is_contiguous()
    P = torch.empty_like(S) if P is None else P
    _check("qgemm_softmax_rows", load().qgemm_softmax_rows(S.data_ptr(), P.data_ptr(), S.numel() // S.shape[-1],
                                                          S.shape[-1], float(scale), _stream(S.device)))
    return P


def softmax_rows_causal(S, seq_q: int, q_pos0: int = 0, scale: float = 1.0, P=None):
    """softmax_rows under the causal mask (qgemm_softmax_rows_causal): S is a contiguous stack of score matrices of
    seq_q rows each; query row i = r % seq_q sees its first min(w, i + q_pos0 + 1) columns, the rest of P is +0."""
    import torch
    assert isinstance(S, torch.Tensor) and S.dim() >= 2, "S must be a tensor of 2 or more dimensions"
    assert S.is_cuda and S.dtype == torch.float32 and S.is_contiguous(), "S: contiguous float32 on the device"
    rows = S.numel() // S.shape[-1]
    assert seq_q >= 1 and rows % seq_q == 0, "the rows are whole matrices of seq_q rows"
    assert q_pos0 >= 0
    P = torch.empty_like(S) if P is None else P
    assert P.shape == S.shape and P.dtype == torch.float32 and P.is_cuda and P.is_contiguous(), "P: as S"
    _check("qgemm_softmax_rows_causal",
           load().qgemm_softmax_rows_causal(S.data_ptr(), P.data_ptr(), rows, S.shape[-1], float(scale), seq_q, q_pos0,
                                            _stream(S.device)))
    return P


def add_layernorm_rows(A, B, Y=None):
    """op_add(A, B) + op_layernorm (transformer.cu:58-59, op_layernorm.cuh as written)."""
    import torch
    for t, nm in ((A, "A"), (B, "B")):
        _require_device_f32(t, nm)
        assert t.is_contiguous()
    assert A.shape == B.shape
    Y = torch.empty_like(A) if Y is None else Y
    _check("qgemm_add_layernorm_rows", load().qgemm_add_layernorm_rows(A.data_ptr(), B.data_ptr(), Y.data_ptr(),
                                                                      A.numel() // A.shape[-1], A.shape[-1],
                                                                      _stream(A.device)))
    return Y


def _ln_args(A, B, gamma, beta, Y):
    import torch
    _require_device_f32(A, "A")
    assert A.dim() == 2 and A.is_contiguous(), "A: rows x w, contiguous"
    w = A.shape[1]
    if B is not None:
        _require_device_f32(B, "B")
        assert B.shape == A.shape and B.is_contiguous(), "B: as A"
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == w and \
            t.is_contiguous(), f"{nm}: w float32 values on the device, contiguous"
    Y = torch.empty_like(A) if Y is None else Y
    _require_device_f32(Y, "Y")
    assert Y.shape == A.shape and Y.is_contiguous(), "Y: as A"
    return Y


def layernorm_rows(A, B, gamma, beta, eps: float = 1e-5, Y=None):
    """Y = LN(A + B) with gamma, beta and eps, the standard layer normalisation (qgemm_layernorm_rows);
    B may be None, Y may be A or B."""
    Y = _ln_args(A, B, gamma, beta, Y)
    _check("qgemm_layernorm_rows",
           load().qgemm_layernorm_rows(A.data_ptr(), 0 if B is None else B.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                       float(eps), Y.data_ptr(), A.shape[0], A.shape[1], _stream(A.device)))
    return Y


def _packed_out(out, M: int, K: int, device):
    """The buffer of a fused pack: a fresh one, or the caller's Packed of the same geometry."""
    if out is None:
        return _alloc_packed(M, K, device)
    assert isinstance(out, Packed) and (out.rows, out.k) == (M, K), f"out: a Packed of {M} x {K}"
    return out.buf


def layernorm_pack_a(A, B, gamma, beta, eps: float = 1e-5, Y=None, range: float = DEFAULT_RANGE, out=None):  # noqa: A002
    """layernorm_rows that also packs Y's rows for the next quantized linear (qgemm_layernorm_pack_a): returns
    (Y, Packed), the Packed byte for byte pack_a(Y) (written into `out`'s buffer where given)."""
    Y = _ln_args(A, B, gamma, beta, Y)
    M, K = A.shape
    buf = _packed_out(out, M, K, A.device)
    _check("qgemm_layernorm_pack_a",
           load().qgemm_layernorm_pack_a(A.data_ptr(), 0 if B is None else B.data_ptr(), gamma.data_ptr(),
                                         beta.data_ptr(), float(eps), Y.data_ptr(), M, K, float(range), buf.data_ptr(),
                                         _stream(A.device)))
    return Y, Packed(buf, M, K, range)


def prenorm_pack_a(A, B, gamma, beta, eps: float = 1e-5, S=None, range: float = DEFAULT_RANGE, out=None):  # noqa: A002
    """The pre-LN boundary in one launch (qgemm_prenorm_pack_a): S = A + B, the updated residual stream
    (B may be None: S = A; S=None: not stored; S may be A or B), and LN(A + B) written only packed.  Returns
    (S, Packed), the Packed byte for byte layernorm_pack_a's for the same arguments."""
    _ln_args(A, B, gamma, beta, A if S is None else S)
    M, K = A.shape
    buf = _packed_out(out, M, K, A.device)
    _check("qgemm_prenorm_pack_a",
           load().qgemm_prenorm_pack_a(A.data_ptr(), 0 if B is None else B.data_ptr(), gamma.data_ptr(),
                                       beta.data_ptr(), float(eps), 0 if S is None else S.data_ptr(), M, K,
                                       float(range), buf.data_ptr(), _stream(A.device)))
    return S, Packed(buf, M, K, range)


def add_rows(A, B, S=None):
    """S = A + B on rows x w floats (qgemm_add_rows): the last boundary of a pre-LN model without a final norm.  S may
    be A or B."""
    import torch
    for t, nm in ((A, "A"), (B, "B")):
        _require_device_f32(t, nm)
    assert A.dim() == 2 and A.is_contiguous() and B.shape == A.shape and B.is_contiguous(), "A, B: rows x w, contiguous"
    S = torch.empty_like(A) if S is None else S
    _require_device_f32(S, "S")
    assert S.shape == A.shape and S.is_contiguous(), "S: as A"
    _check("qgemm_add_rows", load().qgemm_add_rows(A.data_ptr(), B.data_ptr(), S.data_ptr(), A.shape[0], A.shape[1],
                                                  _stream(A.device)))
    return S


def gelu_rows(X, Y=None):
    """The tanh-form GELU elementwise (qgemm_gelu_rows): X rows x w with unit inner stride, any row stride."""
    import torch
    _require_device_f32(X, "X")
    assert X.dim() == 2 and X.stride(1) == 1, "X: rows x w, unit inner stride"
    Y = torch.empty(X.shape, dtype=torch.float32, device=X.device) if Y is None else Y
    _require_device_f32(Y, "Y")
    assert Y.shape == X.shape and Y.stride(1) == 1
    _check("qgemm_gelu_rows", load().qgemm_gelu_rows(X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0), X.shape[0],
                                                    X.shape[1], _stream(X.device)))
    return Y


def gelu_pack_a(X, range: float = DEFAULT_RANGE, out=None) -> Packed:  # noqa: A002
    """pack_a(gelu_rows(X)) in one launch, the GELU'd matrix never written (qgemm_gelu_pack_a); k <= 16384."""
    _require_device_f32(X, "X")
    assert X.dim() == 2 and X.stride(1) == 1, "X: m x k, unit inner stride"
    M, K = X.shape
    buf = _packed_out(out, M, K, X.device)
    _check("qgemm_gelu_pack_a", load().qgemm_gelu_pack_a(X.data_ptr(), X.stride(0), M, K, float(range), buf.data_ptr(),
                                                        _stream(X.device)))
    return Packed(buf, M, K, range)


def rmsnorm_rows(A, B, gamma, eps: float = 1e-5, Y=None):
    """Y = RMSNorm(A + B) with gamma and eps, the root-mean-square norm of Llama-style blocks (qgemm_rmsnorm_rows,
    DESIGN.md s28); B may be None, Y may be A or B."""
    Y = _ln_args(A, B, gamma, gamma, Y)
    _check("qgemm_rmsnorm_rows",
           load().qgemm_rmsnorm_rows(A.data_ptr(), 0 if B is None else B.data_ptr(), gamma.data_ptr(), float(eps),
                                     Y.data_ptr(), A.shape[0], A.shape[1], _stream(A.device)))
    return Y


def rmsnorm_pack_a(A, B, gamma, eps: float = 1e-5, Y=None, range: float = DEFAULT_RANGE, out=None):  # noqa: A002
    """rmsnorm_rows that also packs Y's rows for the next quantized linear (qgemm_rmsnorm_pack_a): returns
    (Y, Packed), the Packed byte for byte pack_a(Y) (written into `out`'s buffer where given)."""
    Y = _ln_args(A, B, gamma, gamma, Y)
    M, K = A.shape
    buf = _packed_out(out, M, K, A.device)
    _check("qgemm_rmsnorm_pack_a",
           load().qgemm_rmsnorm_pack_a(A.data_ptr(), 0 if B is None else B.data_ptr(), gamma.data_ptr(), float(eps),
                                       Y.data_ptr(), M, K, float(range), buf.data_ptr(), _stream(A.device)))
    return Y, Packed(buf, M, K, range)


def prenorm_rms_pack_a(A, B, gamma, eps: float = 1e-5, S=None, range: float = DEFAULT_RANGE, out=None):  # noqa: A002
    """The pre-norm boundary of an RMS model in one launch (qgemm_prenorm_rms_pack_a): S = A + B (B may
    be None: S = A; S=None: not stored; S may be A or B), and RMSNorm(A + B) written only packed.  Returns (S, Packed),
    the Packed byte for byte rmsnorm_pack_a's for the same arguments."""
    _ln_args(A, B, gamma, gamma, A if S is None else S)
    M, K = A.shape
    buf = _packed_out(out, M, K, A.device)
    _check("qgemm_prenorm_rms_pack_a",
           load().qgemm_prenorm_rms_pack_a(A.data_ptr(), 0 if B is None else B.data_ptr(), gamma.data_ptr(), float(eps),
                                           0 if S is None else S.data_ptr(), M, K, float(range), buf.data_ptr(),
                                           _stream(A.device)))
    return S, Packed(buf, M, K, range)


def _glu_args(X, activation):
    _require_device_f32(X, "X")
    assert X.dim() == 2 and X.stride(1) == 1 and X.shape[1] % 2 == 0, "X: rows x 2w ([gate | up]), unit inner stride"
    assert activation in ACTIVATIONS, f"activation: one of {sorted(ACTIVATIONS)}"
    return X.shape[0], X.shape[1] // 2, ACTIVATIONS[activation]


def glu_rows(X, activation: str = "silu", Y=None):
    """act(gate) * up elementwise (qgemm_glu_rows): X rows x 2w with the gate in its left half and up
    in its right half, unit inner stride, any row stride; Y rows x w."""
    import torch
    rows, w, act = _glu_args(X, activation)
    Y = torch.empty((rows, w), dtype=torch.float32, device=X.device) if Y is None else Y
    _require_device_f32(Y, "Y")
    assert Y.shape == (rows, w) and Y.stride(1) == 1
    _check("qgemm_glu_rows", load().qgemm_glu_rows(X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0), rows, w, act,
                                                  _stream(X.device)))
    return Y


def glu_pack_a(X, activation: str = "silu", range: float = DEFAULT_RANGE, out=None) -> Packed:  # noqa: A002
    """pack_a(glu_rows(X)) in one launch, the product never written (qgemm_glu_pack_a); w <= 16384."""
    M, K, act = _glu_args(X, activation)
    buf = _packed_out(out, M, K, X.device)
    _check("qgemm_glu_pack_a", load().qgemm_glu_pack_a(X.data_ptr(), X.stride(0), M, K, act, float(range),
                                                      buf.data_ptr(), _stream(X.device)))
    return Packed(buf, M, K, range)


def _rope_args(X, groups: int, d_k: int, cos, sin):
    _require_device_f32(X, "X")
    _require_device_f32(cos, "cos")
    _require_device_f32(sin, "sin")
    assert X.dim() == 2 and X.stride(1) == 1 and X.shape[1] == groups * d_k, "X: rows x groups * d_k, unit inner stride"
    assert cos.is_contiguous() and sin.is_contiguous() and cos.dim() == 2 and cos.shape == sin.shape and \
        2 * cos.shape[1] == d_k, "cos, sin: table_rows x d_k / 2, contiguous"
    return cos.shape[0]


def rope_rows(X, groups: int, d_k: int, cos, sin, pos0: int = 0):
    """Rotary position embedding IN PLACE on the rows of X (qgemm_rope_rows): rows x groups * d_k floats, any row
    stride; row r of every group is rotated (half-split pairing) by position pos0 + r of the tables cos, sin
    (table_rows x d_k / 2).  Returns X."""
    table_rows = _rope_args(X, groups, d_k, cos, sin)
    _check("qgemm_rope_rows", load().qgemm_rope_rows(X.data_ptr(), X.stride(0), X.shape[0], groups, d_k, cos.data_ptr(),
                                                    sin.data_ptr(), table_rows, int(pos0), _stream(X.device)))
    return X


def rope_rows_varlen(X, groups: int, d_k: int, cos, sin, row0, n_rows, pos0):
    """rope_rows on len(n_rows) <= 64 sequences in one launch (qgemm_rope_rows_varlen): sequence b is rows row0[b] ..
    row0[b] + n_rows[b] - 1 of X at positions pos0[b] ..; rows between the sequences are not touched.  Returns X."""
    table_rows = _rope_args(X, groups, d_k, cos, sin)
    n = len(n_rows)
    assert all(0 <= int(r) and int(r) + int(c) <= X.shape[0] for r, c in zip(row0, n_rows)), "a sequence leaves X"
    _check("qgemm_rope_rows_varlen",
           load().qgemm_rope_rows_varlen(X.data_ptr(), X.stride(0), groups, d_k, cos.data_ptr(), sin.data_ptr(),
                                         table_rows, n, _int64_array(row0, n, "row0"), _int_array(n_rows, n, "n_rows"),
                                         _int_array(pos0, n, "pos0"), _stream(X.device)))
    return X


def mm_outlier(A, B, threshold: float = 6.0, C=None):
    """LLM.int8() decomposition: outlier feature columns in fp32, the rest int8.
    Returns (C, number of outlier columns)."""
    import torch
    _require_device_f32(A, "A")
    _require_device_f32(B, "B")
    assert A.is_contiguous() and B.is_contiguous()
    M, K = A.shape
    N = B.shape[1]
    assert B.shape[0] == K
    if C is None:
        C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    L = load()
    ws = torch.empty(L.qgemm_mm_outlier_workspace_size(M, N, K), dtype=torch.uint8, device=A.device)
    _check("qgemm_mm_outlier", L.qgemm_mm_outlier(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, float(threshold),
                                                  ws.data_ptr(), ws.numel(), _stream(A.device)))
    cnt = ctypes.c_int()
    torch.cuda.current_stream(A.device).synchronize()
    _check("qgemm_outlier_count", L.qgemm_outlier_count(K, ws.data_ptr(), ctypes.byref(cnt)))
    return C, cnt.value


def linear_outlier(X, pw: Packed, threshold: float = 6.0, bias=None, relu: bool = False, Y=None):
    """LLM.int8() decomposition on a cached weight (qgemm_linear_outlier): X's outlier feature columns are found per
    call and multiplied in fp32 against the matching rows of pw dequantized from its int8 (Wq * Cw / 127), the rest runs
    the int8 chain on pw as linear() does; then [+ b] [relu].  fp32 X and Y.  Returns (Y, number of outlier columns)."""
    import torch
    # the entry point quantizes X with range 127 and dequantizes the weight's rows with 1/127
    assert pw.range == DEFAULT_RANGE, f"qgemm_linear_outlier needs a weight packed with range {DEFAULT_RANGE}"
    _require_device_f32(X, "X")
    assert X.stride(1) == 1 and X.shape[1] == pw.k
    M, K = X.shape
    N = pw.rows
    if Y is None:
        Y = torch.empty((M, N), dtype=torch.float32, device=X.device)
    _require_device_f32(Y, "Y")
    assert Y.shape == (M, N) and Y.stride(1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32, "bias stays float32"
    assert bias is not None or not relu, "relu follows a bias (qgemm_linear_outlier)"
    L = load()
    ws = torch.empty(max(4, L.qgemm_linear_outlier_workspace_size(M, N, K)), dtype=torch.uint8, device=X.device)
    if M == 0 or N == 0:
        return Y, 0
    _check("qgemm_linear_outlier",
           L.qgemm_linear_outlier(X.data_ptr(), X.stride(0), M, K, pw.buf.data_ptr(), N,
                                  0 if bias is None else bias.data_ptr(), 1 if relu else 0, float(threshold),
                                  Y.data_ptr(), Y.stride(0), ws.data_ptr(), ws.numel(), _stream(X.device)))
    cnt = ctypes.c_int()
    torch.cuda.current_stream(X.device).synchronize()
    _check("qgemm_outlier_count", L.qgemm_outlier_count(K, ws.data_ptr(), ctypes.byref(cnt)))
    return Y, cnt.value


ENCODER_WEIGHT_KINDS = ("Wq", "Wk", "Wv", "Wo", "W1", "b1", "W2", "b2")
DECODER_WEIGHT_KINDS = ENCODER_WEIGHT_KINDS + ("Wq2", "Wk2", "Wv2", "Wo2")  # kinds 8..11: the cross-attention's


def encoder_weight_seed(base: int, block: int, kind: int, head: int) -> int:
    """Seed of one encoder weight tensor (include/qgemm.h, transformer.hip)."""
    return (base * 1000003 + block * 4099 + kind * 131 + head) & 0xFFFFFFFFFFFFFFFF


# The weight kinds by name (include/qgemm.h): KIND_WQ .. KIND_WV and KIND_WQ2 .. KIND_WV2 are one tensor per head.
(KIND_WQ, KIND_WK, KIND_WV, KIND_WO, KIND_W1, KIND_B1, KIND_W2, KIND_B2,
 KIND_WQ2, KIND_WK2, KIND_WV2, KIND_WO2) = range(12)
# The standard architecture's vectors (qgemm_model_create), 1 x d_model each, head 0; KIND_BQ2 .. on a
# decoder only.  A reference-arch model refuses them.
(KIND_BQ, KIND_BK, KIND_BV, KIND_BO, KIND_G1, KIND_BE1, KIND_G3, KIND_BE3,
 KIND_BQ2, KIND_BK2, KIND_BV2, KIND_BO2, KIND_G2, KIND_BE2) = range(12, 26)
# The final norm of a pre-LN model created with final_norm=True: block 0, head 0; refused elsewhere.
KIND_GF, KIND_BEF = 26, 27
# The rotary tables of a model created with rope=True: max_seq x d_k / 2 each, block 0, head 0.
KIND_ROPE_COS, KIND_ROPE_SIN = 28, 29
# The up projection of a model created with gated_ffn=True and its bias: d_model x d_ff and 1 x d_ff,
# every block's, head 0.  KIND_W1 is then the gate (HF gate_proj), KIND_W3 up (up_proj), KIND_W2 down (down_proj).
KIND_W3, KIND_B3 = 30, 31
_VECTOR_KINDS = (KIND_B1, KIND_B2, KIND_B3) + tuple(range(KIND_BQ, KIND_BEF + 1))
# packed_weight's `which`
(WEIGHT_WQKV, WEIGHT_WO, WEIGHT_W1, WEIGHT_W2, WEIGHT_WQ2, WEIGHT_WKV2, WEIGHT_WO2) = range(7)


class _DeviceView:
    """Device memory owned by someone else, for torch.as_tensor: `owner` stays alive as long as the tensor does."""

    def __init__(self, ptr: int, nbytes: int, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class _ArchKeywords(type):
    """Encoder(..., arch=, activation=, ln_eps=, norm_first=, final_norm=, rope=) and the same on Decoder, which also takes
    decoder_only=: keyword-only arguments of the class call, set on the object before __init__ runs.  decoder_only
    (Decoder, with max_enc_seq = 0): the blocks lack the cross-attention; rope (arch="standard" only): rotary
    embeddings on Q and K.  norm_first (arch="standard" only): the pre-LN
    block; final_norm (with norm_first only): a LayerNorm behind the last block.  norm="rms"
    (arch="standard" only): every norm is the RMS norm with gamma alone; gated_ffn=True (arch="standard" only): the FFN
    is (act(x W1 + b1) * (x W3 + b3)) W2 + b2, and activation="silu" is valid with it alone.  __init__ keeps its parameter list as it was (its last parameters stay
    max_rows, and n_slots on a Decoder), so positional callers and tools that read that list see no change."""

    def __call__(cls, *args, arch: str = "reference", activation: str = "relu", ln_eps: float = 1e-5,
                 norm_first: bool = False, final_norm: bool = False, decoder_only: bool = False, rope: bool = False,
                 norm: str = "layer", gated_ffn: bool = False, **kw):
        assert not norm_first or arch != "reference", "norm_first needs arch='standard'"
        assert norm_first or not final_norm, "final_norm needs norm_first=True"
        assert not rope or arch != "reference", "rope needs arch='standard'"
        assert norm in NORMS, f"norm: one of {NORMS}"
        assert norm == "layer" or arch != "reference", "norm='rms' needs arch='standard'"
        assert not gated_ffn or arch != "reference", "gated_ffn needs arch='standard'"
        assert activation != "silu" or gated_ffn, "activation='silu' needs gated_ffn=True"
        if decoder_only:  # (Decoder's parameters: d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, ..)
            assert cls.__name__ == "Decoder", "decoder_only belongs to Decoder"
            max_enc_seq = kw["max_enc_seq"] if "max_enc_seq" in kw else (args[5] if len(args) > 5 else None)
            assert max_enc_seq == 0, "decoder_only needs max_enc_seq = 0"
        self = cls.__new__(cls)
        self.arch, self.activation, self.ln_eps = arch, activation, float(ln_eps)
        self.norm_first, self.final_norm = bool(norm_first), bool(final_norm)
        self.decoder_only, self.rope = bool(decoder_only), bool(rope)
        self.norm, self.gated_ffn = norm, bool(gated_ffn)
        self.__init__(*args, **kw)
        return self


class _ModelWeights(metaclass=_ArchKeywords):
    """Caller-supplied weights of an Encoder or Decoder (qgemm_model_*).  A weight tensor is rows x
    cols with y = x W, as layout "kn"; a checkpoint's [out, in] tensor is layout "nk".  fp32 or bf16, any strides."""

    def weight_shape(self, kind: int) -> tuple:
        """(rows, cols, heads) of a tensor of `kind`: heads > 1 tensors exist for the per-head kinds."""
        shapes = self.__dict__.setdefault("_weight_shapes", {})   # fixed at creation: asked once per kind
        if kind not in shapes:
            r, c, h = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            _check("qgemm_model_weight_shape",
                   load().qgemm_model_weight_shape(self._h, kind, ctypes.byref(r), ctypes.byref(c), ctypes.byref(h)))
            shapes[kind] = (r.value, c.value, h.value)
        return shapes[kind]

    def set_weight(self, block: int, kind: int, W, head=None, layout: str = "kn"):
        """Load tensor (block, kind, head) from W (qgemm_model_set_weight): one window-pack launch into the block's
        packed weight, or a copy for a bias (W: n elements, 1-D or 1 x n).  head=None: head 0 for a kind without
        heads, and for a per-head kind W is [n_heads, rows, cols] ("kn") or [n_heads, cols, rows] ("nk") and every head
        is loaded.  On a decoder with caches every slot goes back to "not begun"."""
        import torch
        assert isinstance(W, torch.Tensor) and W.is_cuda and W.dtype in (torch.float32, torch.bfloat16), \
            "W must be a float32 or bfloat16 device tensor"
        rows, cols, heads = self.weight_shape(kind)
        if head is None and heads > 1:
            assert W.dim() == 3 and W.shape[0] == heads, "head=None on a per-head kind takes [n_heads, ...]"
            for h in range(heads):
                self.set_weight(block, kind, W[h], head=h, layout=layout)
            return
        head = 0 if head is None else int(head)
        if kind in _VECTOR_KINDS:
            W = W.reshape(1, -1) if W.dim() == 1 else W
            layout = "kn"
        tag, r, c, sh, sw = _window_source(W, layout, "W")
        assert (r, c) == (rows, cols), f"kind {kind} is {rows} x {cols}"
        _check("qgemm_model_set_weight",
               load().qgemm_model_set_weight(self._h, block, kind, head, W.data_ptr(), tag, sh, sw, _stream(W.device)))

    def load_weights(self, mapping, layout: str = "kn"):
        """set_weight for every entry of a mapping keyed (block, kind) or (block, kind, head)."""
        for key, W in mapping.items():
            block, kind = key[0], key[1]
            self.set_weight(block, kind, W, head=key[2] if len(key) > 2 else None, layout=layout)

    def _create_model(self, cross: bool, max_enc_seq: int, flags: int, n_slots: int, max_rows, arch: str,
                      activation: str, ln_eps: float):
        """qgemm_model_create: the creator that knows architectures (the older creators make reference-arch models)."""
        assert arch in ARCHS, f"arch: one of {sorted(ARCHS)}"
        assert activation in ACTIVATIONS, f"activation: one of {sorted(ACTIVATIONS)}"
        desc = ModelDesc(ctypes.sizeof(ModelDesc), 1 if cross else 0, self.d_model, self.n_heads, self.d_ff,
                         self.n_blocks, self.max_seq, max_enc_seq, self.seed, flags, n_slots,
                         0 if max_rows is None else int(max_rows),
                         ARCHS[arch] | (QGEMM_ARCH_NORM_FIRST if self.norm_first else 0) |
                         (QGEMM_ARCH_FINAL_NORM if self.final_norm else 0) |
                         (QGEMM_ARCH_DECODER_ONLY if getattr(self, "decoder_only", False) else 0) |
                         (QGEMM_ARCH_ROPE if getattr(self, "rope", False) else 0) |
                         (QGEMM_ARCH_RMSNORM if getattr(self, "norm", "layer") == "rms" else 0) |
                         (QGEMM_ARCH_GATED_FFN if getattr(self, "gated_ffn", False) else 0),
                         ACTIVATIONS[activation], float(ln_eps))
        h = ctypes.c_void_p()
        _check("qgemm_model_create", load().qgemm_model_create(ctypes.byref(desc), ctypes.byref(h)))
        return h

    def info(self) -> dict:
        """The descriptor the model was created with (qgemm_model_info), as a dict."""
        desc = ModelDesc()
        _check("qgemm_model_info", load().qgemm_model_info(self._h, ctypes.byref(desc)))
        return {name: getattr(desc, name) for name, _ in ModelDesc._fields_}

    def load_torch_layer(self, block: int, layer):
        """Load every tensor of `block` from a torch.nn.TransformerEncoderLayer (an Encoder) or TransformerDecoderLayer
        (a Decoder) whose norm_first is the model's: the set_weight calls for the q / k / v thirds of in_proj_weight head by head
        (rows h d_k .. of a third are head h's [out, in] tensor), in_proj_bias, out_proj, linear1 / linear2 and the
        norms; a decoder layer's multihead_attn is the cross-attention and its norm2 LN2, an encoder layer's norm2 is
        the FFN's LN (kinds KIND_G3 / KIND_BE3) -- on a pre-LN layer the same norms stand in front of their sub-layers.
        Tensors are copied to the current device as they are (fp32 or bf16,
        anything else as fp32).  ValueError: a norm_first that is not the model's, a width, head count or epsilon that is not the model's, a
        layer of the other kind, or a reference-arch model.  The layer's activation is not looked at: create the model
        with the matching one."""
        import torch
        if self.arch != "standard":
            raise ValueError("load_torch_layer needs a model created with arch='standard'")
        if getattr(self, "norm", "layer") != "layer" or getattr(self, "gated_ffn", False):
            raise ValueError("torch.nn has no layer with an RMS norm or a gated FFN: load such a model with set_weight")
        cross = hasattr(layer, "multihead_attn")
        if cross != (isinstance(self, Decoder) and not getattr(self, "decoder_only", False)):
            raise ValueError("an Encoder or a decoder-only Decoder takes a TransformerEncoderLayer, a Decoder with "
                             "cross-attention a TransformerDecoderLayer")
        if bool(getattr(layer, "norm_first", False)) != getattr(self, "norm_first", False):
            raise ValueError(f"the layer has norm_first={bool(getattr(layer, 'norm_first', False))}, the model "
                             f"norm_first={getattr(self, 'norm_first', False)}")
        d, H, dk = self.d_model, self.n_heads, self.d_model // self.n_heads
        attns = [layer.self_attn] + ([layer.multihead_attn] if cross else [])
        for a in attns:
            if a.embed_dim != d or a.num_heads != H or a.in_proj_weight is None or a.in_proj_bias is None:
                raise ValueError(f"attention of width {a.embed_dim} with {a.num_heads} heads (fused, biased in_proj) "
                                 f"expected: the model has d_model {d}, {H} heads")
        if (layer.linear1.in_features, layer.linear1.out_features) != (d, self.d_ff) or \
                (layer.linear2.in_features, layer.linear2.out_features) != (self.d_ff, d):
            raise ValueError(f"the layer's FFN is not {d} x {self.d_ff} x {d}")
        norms = [layer.norm1, layer.norm2] + ([layer.norm3] if cross else [])
        for n in norms:
            if tuple(n.normalized_shape) != (d,) or n.weight is None or n.bias is None or \
                    abs(n.eps - self.ln_eps) > 1e-12:
                raise ValueError(f"the layer's norms must be affine LayerNorm({d}, eps={self.ln_eps})")
        dev = torch.device("cuda", torch.cuda.current_device())

        def dv(t):
            t = t.detach()
            return t.to(dev) if t.dtype in (torch.float32, torch.bfloat16) else t.to(dev, torch.float32)

        def attn(a, wkinds, bkinds, wo, bo):
            Wi, bi = dv(a.in_proj_weight), dv(a.in_proj_bias)
            for j, (wk, bk) in enumerate(zip(wkinds, bkinds)):
                for h in range(H):
                    self.set_weight(block, wk, Wi[j * d + h * dk:j * d + (h + 1) * dk], head=h, layout="nk")
                self.set_weight(block, bk, bi[j * d:(j + 1) * d])
            self.set_weight(block, wo, dv(a.out_proj.weight), layout="nk")
            self.set_weight(block, bo, dv(a.out_proj.bias))

        attn(layer.self_attn, (KIND_WQ, KIND_WK, KIND_WV), (KIND_BQ, KIND_BK, KIND_BV), KIND_WO, KIND_BO)
        self.set_weight(block, KIND_G1, dv(layer.norm1.weight))
        self.set_weight(block, KIND_BE1, dv(layer.norm1.bias))
        if cross:
            attn(layer.multihead_attn, (KIND_WQ2, KIND_WK2, KIND_WV2), (KIND_BQ2, KIND_BK2, KIND_BV2), KIND_WO2, KIND_BO2)
            self.set_weight(block, KIND_G2, dv(layer.norm2.weight))
            self.set_weight(block, KIND_BE2, dv(layer.norm2.bias))
        self.set_weight(block, KIND_W1, dv(layer.linear1.weight), layout="nk")
        self.set_weight(block, KIND_B1, dv(layer.linear1.bias))
        self.set_weight(block, KIND_W2, dv(layer.linear2.weight), layout="nk")
        self.set_weight(block, KIND_B2, dv(layer.linear2.bias))
        ffn_norm = layer.norm3 if cross else layer.norm2
        self.set_weight(block, KIND_G3, dv(ffn_norm.weight))
        self.set_weight(block, KIND_BE3, dv(ffn_norm.bias))

    def load_torch_final_norm(self, ln):
        """Load the norm behind the last block (kinds KIND_GF / KIND_BEF) from an affine
        torch.nn.LayerNorm(d_model, eps=ln_eps): the `norm` of a torch.nn.TransformerEncoder / TransformerDecoder.
        ValueError: any other module, or a model created without final_norm=True."""
        import torch
        if not getattr(self, "final_norm", False):
            raise ValueError("load_torch_final_norm needs a model created with final_norm=True")
        if getattr(self, "norm", "layer") != "layer" or getattr(self, "gated_ffn", False):
            raise ValueError("torch.nn has no layer with an RMS norm or a gated FFN: load such a model with set_weight")
        if not isinstance(ln, torch.nn.LayerNorm) or tuple(ln.normalized_shape) != (self.d_model,) or \
                ln.weight is None or ln.bias is None or abs(ln.eps - self.ln_eps) > 1e-12:
            raise ValueError(f"the final norm must be an affine LayerNorm({self.d_model}, eps={self.ln_eps})")
        dev = torch.device("cuda", torch.cuda.current_device())
        for kind, t in ((KIND_GF, ln.weight), (KIND_BEF, ln.bias)):
            t = t.detach()
            self.set_weight(0, kind, t.to(dev) if t.dtype in (torch.float32, torch.bfloat16) else t.to(dev, torch.float32))

    def packed_weight(self, block: int, which: int) -> Packed:
        """Block's packed weight `which` (WEIGHT_WQKV ..) as a NON-OWNING Packed view of the model's own buffer, for
        tests and tools: read it, do not write it, and do not use it after close()."""
        import torch
        p, n, k = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        _check("qgemm_model_packed_weight",
               load().qgemm_model_packed_weight(self._h, block, which, ctypes.byref(p), ctypes.byref(n), ctypes.byref(k)))
        nbytes = load().qgemm_packed_size(n.value, k.value)
        buf = torch.as_tensor(_DeviceView(p.value, nbytes, self), device=torch.device("cuda", torch.cuda.current_device()))
        return Packed(buf, n.value, k.value, DEFAULT_RANGE)

    def bias(self, block: int, kind: int):
        """Block's bias KIND_B1 or KIND_B2 (KIND_B3 on a gated model), or on a standard model a vector of kinds
        KIND_BQ ..: a copy, n floats on the device."""
        import torch
        p, n = ctypes.c_void_p(), ctypes.c_int()
        _check("qgemm_model_bias", load().qgemm_model_bias(self._h, block, kind, ctypes.byref(p), ctypes.byref(n)))
        dev = torch.device("cuda", torch.cuda.current_device())
        return torch.as_tensor(_DeviceView(p.value, 4 * n.value, self), device=dev).view(torch.float32).clone()

    def rope_tables(self):
        """(cos, sin) of a model created with rope=True (qgemm_model_rope_tables): copies, max_seq x d_k / 2 floats each
        on the device -- what set_weight(0, KIND_ROPE_COS / KIND_ROPE_SIN, ..) replaces."""
        import torch
        c, s, rows, half = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        _check("qgemm_model_rope_tables", load().qgemm_model_rope_tables(self._h, ctypes.byref(c), ctypes.byref(s),
                                                                        ctypes.byref(rows), ctypes.byref(half)))
        dev = torch.device("cuda", torch.cuda.current_device())
        nbytes = 4 * rows.value * half.value
        return tuple(torch.as_tensor(_DeviceView(p.value, nbytes, self), device=dev).view(torch.float32)
                     .reshape(rows.value, half.value).clone() for p in (c, s))


class Encoder(_ModelWeights):
    """transformer.cu:14-77's Encoder with its linears on the quantized path.  max_rows
    (qgemm_encoder_create_rows): the rows forward_batch may run at once, max_seq where left out.
    arch="standard" (a keyword of the class call, as activation= and ln_eps= are; qgemm_model_create): the
    textbook post-LN block instead -- biases on every
    projection, block-input residuals, LayerNorm with gamma, beta and ln_eps, activation "relu" or "gelu_tanh" -- which
    load_torch_layer fills from a torch.nn.TransformerEncoderLayer; the defaults give the reference's block through the
    older creators.  norm_first=True (with arch="standard"): the pre-LN block of norm_first=True layers, and
    final_norm=True (with norm_first): a LayerNorm behind the last block, loaded by load_torch_final_norm (DESIGN.md
    s26)."""

    def __init__(self, d_model: int, n_heads: int, d_ff: int, n_blocks: int, max_seq: int, seed: int = 0,
                 max_rows=None):
        self.d_model, self.n_heads, self.d_ff, self.n_blocks, self.max_seq, self.seed = (
            d_model, n_heads, d_ff, n_blocks, max_seq, seed)
        self.max_rows = max_rows
        h = ctypes.c_void_p()
        if self.arch != "reference" or self.activation != "relu":
            # the post-LN block of torch.nn.TransformerEncoderLayer (qgemm_model_create)
            h = self._create_model(False, 0, 0, 0, max_rows, self.arch, self.activation, self.ln_eps)
        elif max_rows is None:
            _check("qgemm_encoder_create", load().qgemm_encoder_create(d_model, n_heads, d_ff, n_blocks, max_seq, seed,
                                                                      ctypes.byref(h)))
        else:
            _check("qgemm_encoder_create_rows",
                   load().qgemm_encoder_create_rows(d_model, n_heads, d_ff, n_blocks, max_seq, int(max_rows), seed,
                                                    ctypes.byref(h)))
        self._h = h

    def forward_batch(self, X, seq_lens, Y=None):
        """forward on len(seq_lens) sequences at once (qgemm_encoder_forward_batch): X holds their rows packed one
        after another, sum(seq_lens) x d_model; the rows of each sequence in Y are, bit for bit, forward's on that
        sequence alone."""
        import torch
        _require_device_f32(X, "X")
        seq_lens = [int(v) for v in seq_lens]
        assert X.is_contiguous() and X.shape == (sum(seq_lens), self.d_model), "X: sum(seq_lens) x d_model, contiguous"
        Y = torch.empty_like(X) if Y is None else Y
        _require_device_f32(Y, "Y")
        assert Y.is_contiguous() and Y.shape == X.shape
        n = len(seq_lens)
        _check("qgemm_encoder_forward_batch",
               load().qgemm_encoder_forward_batch(self._h, X.data_ptr(), Y.data_ptr(), n,
                                                  _int_array(seq_lens, n, "seq_lens"), _stream(X.device)))
        return Y

    def forward(self, X, Y=None):
        import torch
        _require_device_f32(X, "X")
        assert X.is_contiguous() and X.shape[1] == self.d_model
        Y = torch.empty_like(X) if Y is None else Y
        _check("qgemm_encoder_forward", load().qgemm_encoder_forward(self._h, X.data_ptr(), Y.data_ptr(), X.shape[0],
                                                                    _stream(X.device)))
        return Y

    def close(self):
        if getattr(self, "_h", None):
            load().qgemm_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def attention(Q, K, V, n_heads: int, scale=None, O=None, causal: bool = False, q_pos0=None):
    """Multi-head fp32 attention core (qgemm_attention): O_h = softmax(Q_h K_h^T * scale) V_h on columns
    h*d_k .. of each matrix, d_k = Q.shape[1] / n_heads.  Q: seq_q x d, K and V: seq_kv x d -- 2-D fp32 device
    tensors or views with unit inner stride (column slices of wider buffers included); O (seq_q x d) must not
    overlap them.  scale defaults to fl32(1 / sqrt(d_k)), as the encoder computes it.  One fused launch for
    d_k <= 64 and seq_kv <= 512, else three launches through a scores workspace allocated here; at most 8 query rows
    with d_k <= 64 take the decode launch instead, up to 4096 keys (attention_plan names the launch; the same bits).
    causal=True (qgemm_attention_causal): query row i sees keys 0 .. min(seq_kv, i + q_pos0 + 1) - 1, the masked
    columns of P are +0.  q_pos0 is the key position of query row 0; left out it is seq_kv - seq_q, the queries
    aligned to the end of the keys as with a key / value cache (seq_kv >= seq_q is then asserted)."""
    import math
    import torch
    for t, nm in ((Q, "Q"), (K, "K"), (V, "V")):
        _require_device_f32(t, nm)
        assert t.stride(1) == 1 or t.shape[1] == 1, f"{nm} must have unit inner stride"
    seq_q, d = Q.shape
    seq_kv = K.shape[0]
    assert K.shape == (seq_kv, d) and V.shape == (seq_kv, d), "K and V: seq_kv x d, d as Q"
    assert n_heads >= 1 and d % n_heads == 0, "d % n_heads == 0"
    dk = d // n_heads
    if scale is None:
        scale = ctypes.c_float(1.0 / math.sqrt(float(dk))).value  # attention.cuh:64
    if O is None:
        O = torch.empty((seq_q, d), dtype=torch.float32, device=Q.device)
    _require_device_f32(O, "O")
    assert O.shape == (seq_q, d) and (O.stride(1) == 1 or d == 1), "O: seq_q x d with unit inner stride"
    assert causal or q_pos0 is None, "q_pos0 belongs to causal=True"
    if causal and q_pos0 is None:
        assert seq_kv >= seq_q, "causal without q_pos0 aligns the queries to the end of the keys: seq_kv >= seq_q"
        q_pos0 = seq_kv - seq_q
    L = load()
    need = L.qgemm_attention_workspace_size(seq_q, seq_kv, n_heads, dk)
    ws = torch.empty(need, dtype=torch.uint8, device=Q.device) if need else None
    if causal:
        assert q_pos0 >= 0
        _check("qgemm_attention_causal",
               L.qgemm_attention_causal(Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0),
                                        O.data_ptr(), O.stride(0), seq_q, seq_kv, n_heads, dk, float(scale), q_pos0,
                                        ws.data_ptr() if need else None, need, _stream(Q.device)))
        return O
    _check("qgemm_attention",
           L.qgemm_attention(Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0),
                             O.data_ptr(), O.stride(0), seq_q, seq_kv, n_heads, dk, float(scale),
                             ws.data_ptr() if need else None, need, _stream(Q.device)))
    return O


def _int_array(values, n: int, name: str):
    """A host int array of n entries for the C-ABI (None stays NULL)."""
    if values is None:
        return None
    values = [int(v) for v in values]
    assert len(values) == n, f"{name}: one entry per sequence"
    return (ctypes.c_int * max(1, n))(*values)


def attention_decode_batched(Q, K, V, n_heads: int, seq_kv, q_pos0=None, kv_slot=None, rows_per_seq: int = 1,
                             scale=None, O=None):
    """The decode attention launch for up to 64 independent sequences at once (qgemm_attention_decode_batched).
    Q: (n_seqs * rows_per_seq) x d, sequence b's query rows at b * rows_per_seq ..; K and V: [slabs, rows, d] fp32
    device tensors or views with unit inner stride; sequence b attends to rows 0 .. seq_kv[b] - 1 of slab kv_slot[b]
    (left out: slab b).  q_pos0 (one per sequence) masks as attention(causal=True, q_pos0=q_pos0[b]); left out there
    is no mask.  seq_kv, q_pos0 and kv_slot are host sequences of ints, read at the call.  Rows b * rows_per_seq .. of
    the result equal attention() on that sequence's views bit for bit."""
    import math
    import torch
    _require_device_f32(Q, "Q")
    assert Q.stride(1) == 1 or Q.shape[1] == 1, "Q must have unit inner stride"
    for t, nm in ((K, "K"), (V, "V")):
        assert isinstance(t, torch.Tensor) and t.dim() == 3 and t.is_cuda and t.dtype == torch.float32, \
            f"{nm}: a 3-D float32 device tensor [slabs, rows, d]"
        assert t.stride(2) == 1 or t.shape[2] == 1, f"{nm} must have unit inner stride"
    rows, d = Q.shape
    assert K.shape[2] == d and V.shape[2] == d, "K and V: [slabs, rows, d], d as Q"
    assert rows_per_seq >= 1 and rows % rows_per_seq == 0, "Q holds rows_per_seq rows per sequence"
    n_seqs = rows // rows_per_seq
    assert n_heads >= 1 and d % n_heads == 0, "d % n_heads == 0"
    dk = d // n_heads
    seq_kv = [int(v) for v in seq_kv]
    slots = list(range(n_seqs)) if kv_slot is None else [int(v) for v in kv_slot]
    assert len(seq_kv) == n_seqs and len(slots) == n_seqs, "seq_kv and kv_slot: one entry per sequence"
    for b in range(n_seqs):  # the slabs and rows the call reads exist
        assert 0 <= slots[b] < min(K.shape[0], V.shape[0]), f"kv_slot[{b}] names no slab of K / V"
        assert seq_kv[b] <= min(K.shape[1], V.shape[1]), f"seq_kv[{b}] exceeds the slab's rows"
    if scale is None:
        scale = ctypes.c_float(1.0 / math.sqrt(float(dk))).value  # attention.cuh:64
    if O is None:
        O = torch.empty((rows, d), dtype=torch.float32, device=Q.device)
    _require_device_f32(O, "O")
    assert O.shape == (rows, d) and (O.stride(1) == 1 or d == 1), "O: as Q, with unit inner stride"
    _check("qgemm_attention_decode_batched",
           load().qgemm_attention_decode_batched(
               Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(1), K.stride(0), V.data_ptr(), V.stride(1),
               V.stride(0), O.data_ptr(), O.stride(0), n_seqs, rows_per_seq, _int_array(kv_slot, n_seqs, "kv_slot"),
               _int_array(seq_kv, n_seqs, "seq_kv"), _int_array(q_pos0, n_seqs, "q_pos0"), n_heads, dk, float(scale),
               _stream(Q.device)))
    return O


def _require_row_table(t, name):
    """A row table: a 2-D uint8 device tensor or view with unit inner stride (any row stride, any alignment)."""
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2, \
        f"{name}: a 2-D uint8 device tensor"
    assert t.stride(1) == 1 or t.shape[1] == 1, f"{name} must have unit inner stride"
    assert t.shape[0] <= 1 or t.stride(0) >= t.shape[1], f"{name}: the row stride covers a row"


def attention_decode_indirect(Q, K, V, n_heads: int, row_slab, seq_kv, q_pos0=None, tab_row=None,
                              rows_per_seq: int = 1, scale=None, O=None):
    """attention_decode_batched through a per-row slab table (qgemm_attention_decode_indirect): K / V
    row j of sequence b is row j of slab row_slab[tab_row[b]][j] (tab_row left out: row b).  row_slab: a 2-D uint8
    device tensor or view [table rows, entries], unit inner stride, any row stride and alignment; an entry >= the
    number of slabs stands for a row of quiet NaNs.  Bit for bit attention_decode_batched on slabs gathered that
    way."""
    import math
    import torch
    _require_device_f32(Q, "Q")
    assert Q.stride(1) == 1 or Q.shape[1] == 1, "Q must have unit inner stride"
    for t, nm in ((K, "K"), (V, "V")):
        assert isinstance(t, torch.Tensor) and t.dim() == 3 and t.is_cuda and t.dtype == torch.float32, \
            f"{nm}: a 3-D float32 device tensor [slabs, rows, d]"
        assert t.stride(2) == 1 or t.shape[2] == 1, f"{nm} must have unit inner stride"
    _require_row_table(row_slab, "row_slab")
    rows, d = Q.shape
    assert K.shape[2] == d and V.shape[2] == d, "K and V: [slabs, rows, d], d as Q"
    assert rows_per_seq >= 1 and rows % rows_per_seq == 0, "Q holds rows_per_seq rows per sequence"
    n_seqs = rows // rows_per_seq
    assert n_heads >= 1 and d % n_heads == 0, "d % n_heads == 0"
    dk = d // n_heads
    seq_kv = [int(v) for v in seq_kv]
    trows = list(range(n_seqs)) if tab_row is None else [int(v) for v in tab_row]
    assert len(seq_kv) == n_seqs and len(trows) == n_seqs, "seq_kv and tab_row: one entry per sequence"
    n_slabs = min(K.shape[0], V.shape[0])
    for b in range(n_seqs):  # the table rows, entries and slab rows the call reads exist
        assert 0 <= trows[b] < row_slab.shape[0], f"tab_row[{b}] names no row of the table"
        assert seq_kv[b] <= min(K.shape[1], V.shape[1], row_slab.shape[1]), f"seq_kv[{b}] exceeds the slab's rows"
    if scale is None:
        scale = ctypes.c_float(1.0 / math.sqrt(float(dk))).value  # attention.cuh:64
    if O is None:
        O = torch.empty((rows, d), dtype=torch.float32, device=Q.device)
    _require_device_f32(O, "O")
    assert O.shape == (rows, d) and (O.stride(1) == 1 or d == 1), "O: as Q, with unit inner stride"
    _check("qgemm_attention_decode_indirect",
           load().qgemm_attention_decode_indirect(
               Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(1), K.stride(0), V.data_ptr(), V.stride(1),
               V.stride(0), O.data_ptr(), O.stride(0), n_seqs, rows_per_seq, row_slab.data_ptr(),
               row_slab.stride(0) if row_slab.shape[0] > 1 else row_slab.shape[1], n_slabs,
               _int_array(tab_row, n_seqs, "tab_row"), _int_array(seq_kv, n_seqs, "seq_kv"),
               _int_array(q_pos0, n_seqs, "q_pos0"), n_heads, dk, float(scale), _stream(Q.device)))
    return O


def beam_reindex(row_slab, slots, parents, n_rows, beams: int):
    """Beam search's reorder on a row table, in place (qgemm_beam_reindex): row slots[g * beams + q] takes entries
    0 .. n_rows[g] - 1 of the old row slots[g * beams + parents[g * beams + q]], 255 for a parent outside [0, beams).
    row_slab: a 2-D uint8 device tensor or view; parents: int32 on the device; slots and n_rows: host values."""
    _require_row_table(row_slab, "row_slab")
    slots = [int(v) for v in slots]
    rows = len(slots)
    assert beams >= 1 and rows % beams == 0, "beams slots per group"
    n = rows // beams
    n_rows = [int(v) for v in n_rows]
    assert len(n_rows) == n, "n_rows: one entry per group"
    _require_device_i32(parents, "parents", rows)
    assert all(0 <= v < row_slab.shape[0] for v in slots), "slots: rows of the table"
    assert all(v <= row_slab.shape[1] for v in n_rows), "n_rows: inside a table row"
    _check("qgemm_beam_reindex",
           load().qgemm_beam_reindex(row_slab.data_ptr(),
                                     row_slab.stride(0) if row_slab.shape[0] > 1 else row_slab.shape[1], n, beams,
                                     _int_array(slots, rows, "slots"), parents.data_ptr(),
                                     _int_array(n_rows, n, "n_rows"), _stream(row_slab.device)))
    return row_slab


def _int64_array(values, n: int, name: str):
    values = [int(v) for v in values]
    assert len(values) == n, f"{name}: one entry per sequence"
    return (ctypes.c_int64 * max(1, n))(*values)


def _prefix_sums(counts):
    out, acc = [], 0
    for c in counts:
        out.append(acc)
        acc += int(c)
    return out


def attention_varlen(Q, K, V, n_heads: int, seq_q, seq_kv, q_row0=None, kv_row0=None, q_pos0=None, scale=None, O=None):
    """attention() for up to 64 independent sequences of different lengths in one call (qgemm_attention_varlen).
    Sequence b has seq_q[b] query rows from row q_row0[b] of Q -- and of O -- and seq_kv[b] keys from row kv_row0[b]
    of K and V; the row offsets default to the packed layout (prefix sums of seq_q / seq_kv).  q_pos0 (one per
    sequence) masks as attention(causal=True, q_pos0=q_pos0[b]); left out there is no mask.  All of them are host
    sequences of ints, read at the call.  One launch where d_k <= 64 and every seq_kv[b] <= 512, else sequence by
    sequence (attention_varlen_plan); each sequence's rows of the result equal attention() on its views bit for bit,
    and no other row of O is written (a fresh O is zero-filled)."""
    import math
    import torch
    for t, nm in ((Q, "Q"), (K, "K"), (V, "V")):
        _require_device_f32(t, nm)
        assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), f"{nm} must be 2-D with unit inner stride"
    d = Q.shape[1]
    assert K.shape[1] == d and V.shape[1] == d, "K and V: d columns as Q"
    assert n_heads >= 1 and d % n_heads == 0, "d % n_heads == 0"
    dk = d // n_heads
    seq_q, seq_kv = [int(v) for v in seq_q], [int(v) for v in seq_kv]
    n = len(seq_q)
    assert len(seq_kv) == n, "seq_q and seq_kv: one entry per sequence"
    q_row0 = _prefix_sums(seq_q) if q_row0 is None else [int(v) for v in q_row0]
    kv_row0 = _prefix_sums(seq_kv) if kv_row0 is None else [int(v) for v in kv_row0]
    assert len(q_row0) == n and len(kv_row0) == n, "q_row0 and kv_row0: one entry per sequence"
    if O is None:
        O = torch.zeros((Q.shape[0], d), dtype=torch.float32, device=Q.device)
    _require_device_f32(O, "O")
    assert O.dim() == 2 and O.shape[1] == d and (O.stride(1) == 1 or d == 1), "O: d columns, unit inner stride"
    for b in range(n):  # the rows the call reads and writes exist
        if q_row0[b] >= 0 and seq_q[b] >= 0:
            assert q_row0[b] + seq_q[b] <= min(Q.shape[0], O.shape[0]), f"sequence {b}'s query rows exceed Q / O"
        if kv_row0[b] >= 0 and seq_kv[b] >= 0:
            assert kv_row0[b] + seq_kv[b] <= min(K.shape[0], V.shape[0]), f"sequence {b}'s keys exceed K / V"
    if scale is None:
        scale = ctypes.c_float(1.0 / math.sqrt(float(dk))).value  # attention.cuh:64
    L = load()
    sq, skv = _int_array(seq_q, n, "seq_q"), _int_array(seq_kv, n, "seq_kv")
    need = L.qgemm_attention_varlen_workspace_size(n, sq, skv, n_heads, dk)
    ws = torch.empty(need, dtype=torch.uint8, device=Q.device) if need else None
    _check("qgemm_attention_varlen",
           L.qgemm_attention_varlen(Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0),
                                    O.data_ptr(), O.stride(0), n, _int64_array(q_row0, n, "q_row0"), sq,
                                    _int64_array(kv_row0, n, "kv_row0"), skv, _int_array(q_pos0, n, "q_pos0"), n_heads,
                                    dk, float(scale), ws.data_ptr() if need else None, need, _stream(Q.device)))
    return O


def attention_varlen_plan(seq_q, seq_kv, n_heads: int, d_k: int) -> str:
    """The path attention_varlen() takes (qgemm_attention_varlen_plan): "attention_fused_kernel<many>", one launch over
    the table of sequences, or "per_sequence".  Needs no GPU; raises QGemmError for arguments the call refuses."""
    seq_q, seq_kv = [int(v) for v in seq_q], [int(v) for v in seq_kv]
    n = len(seq_q)
    name = ctypes.c_char_p()
    _check("qgemm_attention_varlen_plan",
           load().qgemm_attention_varlen_plan(n, _int_array(seq_q, n, "seq_q"), _int_array(seq_kv, n, "seq_kv"), n_heads,
                                              d_k, ctypes.byref(name)))
    return name.value.decode()


def attention_plan(seq_q: int, seq_kv: int, n_heads: int, d_k: int) -> str:
    """The launch attention() takes for a shape (qgemm_attention_plan): a name that begins "attention_decode",
    "attention_fused" or "three_launches".  Needs no GPU; raises QGemmError for dimensions attention() refuses."""
    name = ctypes.c_char_p()
    _check("qgemm_attention_plan", load().qgemm_attention_plan(seq_q, seq_kv, n_heads, d_k, ctypes.byref(name)))
    return name.value.decode()


class Decoder(_ModelWeights):
    """transformer.cu:79-168's Decoder with its linears on the quantized path: per block self-attention,
    cross-attention on the encoder's output, FFN (DESIGN.md "Decoder").  causal=True (qgemm_decoder_create_ex,
    QGEMM_DECODER_CAUSAL): the self-attention is masked, row i sees rows 0 .. i, and forward(X[:n]) equals
    forward(X)[:n] bit for bit.  kv_cache=True (QGEMM_DECODER_KV_CACHE, with causal=True only): begin(enc_out) starts a
    sequence and step(X_new) returns the output rows of the new input rows alone -- the rows forward would give for them
    on the whole prefix, bit for bit -- from per-block key / value caches.  n_slots > 1
    (qgemm_decoder_create_slots): the caches hold that many independent sequences on one copy of the weights;
    begin_slot / step_slot drive one of them, step_batch advances many in one step, copy_slot forks one;
    begin / step are slot 0's.  max_rows (qgemm_decoder_create_rows; a keyword, ahead of n_slots only so that n_slots
    stays the last parameter): the rows step_varlen may run at once.  With n_slots > 1 the decoder also
    owns the row table of the copy-free beam search (beam_begin / step_batch_indirect / beam_reindex / beam_table /
    generate_beam_indirect).  arch / activation / ln_eps: as on Encoder; every call above works on a
    standard-arch decoder as it does on the reference's, and load_torch_layer fills a block from a
    torch.nn.TransformerDecoderLayer."""

    def __init__(self, d_model: int, n_heads: int, d_ff: int, n_blocks: int, max_seq: int, max_enc_seq: int,
                 seed: int = 0, causal: bool = False, kv_cache: bool = False, max_rows=None, n_slots: int = 1):
        self.d_model, self.n_heads, self.d_ff, self.n_blocks, self.max_seq, self.max_enc_seq, self.seed = (
            d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed)
        self.causal, self.kv_cache, self.n_slots = bool(causal), bool(kv_cache), int(n_slots)
        self.max_rows = max_rows
        h = ctypes.c_void_p()
        if self.arch != "reference" or self.activation != "relu" or getattr(self, "decoder_only", False):
            # the post-LN block of torch.nn.TransformerDecoderLayer (qgemm_model_create); a decoder-only
            # model of any architecture
            flags = (QGEMM_DECODER_CAUSAL if causal else 0) | (QGEMM_DECODER_KV_CACHE if kv_cache else 0)
            h = self._create_model(True, max_enc_seq, flags, n_slots, max_rows, self.arch, self.activation, self.ln_eps)
        elif max_rows is not None:
            # a row budget for step_varlen (qgemm_decoder_create_rows): create_slots with larger scratch buffers
            assert causal and kv_cache, "max_rows belongs to causal=True, kv_cache=True"
            _check("qgemm_decoder_create_rows",
                   load().qgemm_decoder_create_rows(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed,
                                                    QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE, n_slots,
                                                    int(max_rows), ctypes.byref(h)))
        elif n_slots != 1:
            # cache slots (qgemm_decoder_create_slots): n_slots sequences on one copy of the weights
            assert causal and kv_cache, "n_slots belongs to causal=True, kv_cache=True"
            _check("qgemm_decoder_create_slots",
                   load().qgemm_decoder_create_slots(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed,
                                                     QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE, n_slots,
                                                     ctypes.byref(h)))
        elif causal or kv_cache:
            flags = (QGEMM_DECODER_CAUSAL if causal else 0) | (QGEMM_DECODER_KV_CACHE if kv_cache else 0)
            _check("qgemm_decoder_create_ex",
                   load().qgemm_decoder_create_ex(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed,
                                                  flags, ctypes.byref(h)))
        else:
            _check("qgemm_decoder_create", load().qgemm_decoder_create(d_model, n_heads, d_ff, n_blocks, max_seq,
                                                                      max_enc_seq, seed, ctypes.byref(h)))
        self._h = h

    def _enc_args(self, enc_out):
        """(pointer, rows) of the encoder output a forward or a begin passes on: None on a decoder-only model alone."""
        if getattr(self, "decoder_only", False):
            assert enc_out is None, "a decoder-only model takes no enc_out"
            return None, 0
        assert enc_out is not None, "enc_out: the encoder's output rows"
        _require_device_f32(enc_out, "enc_out")
        assert enc_out.is_contiguous() and enc_out.shape[1] == self.d_model
        return enc_out.data_ptr(), enc_out.shape[0]

    def forward(self, X, enc_out=None, Y=None):
        import torch
        _require_device_f32(X, "X")
        assert X.is_contiguous() and X.shape[1] == self.d_model
        enc_ptr, enc_seq = self._enc_args(enc_out)
        Y = torch.empty_like(X) if Y is None else Y
        _check("qgemm_decoder_forward", load().qgemm_decoder_forward(self._h, X.data_ptr(), enc_ptr, Y.data_ptr(),
                                                                    X.shape[0], enc_seq, _stream(X.device)))
        return Y

    def slot_filled(self, slot: int):
        """The filled length of a cache slot as the decoder keeps it (qgemm_decoder_slot_state): None before the
        slot's begin (and on a decoder without caches)."""
        enc_seq, filled, begun = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if not getattr(self, "_h", None) or load().qgemm_decoder_slot_state(self._h, slot, ctypes.byref(enc_seq),
                                                                            ctypes.byref(filled)):
            return None
        if load().qgemm_decoder_slot_begun(self._h, slot, ctypes.byref(begun)):
            return None
        return filled.value if begun.value else None

    @property
    def filled(self):
        """Slot 0's filled length -- the sequence begin() / step() drive: None before begin()."""
        return self.slot_filled(0)

    def begin(self, enc_out=None):
        """Start a sequence (qgemm_decoder_begin): every block's [K2 | V2] of enc_out into its cross cache.  A
        decoder-only model takes no enc_out and launches nothing."""
        enc_ptr, enc_seq = self._enc_args(enc_out)
        _check("qgemm_decoder_begin", load().qgemm_decoder_begin(self._h, enc_ptr, enc_seq,
                                                                _stream(None if enc_out is None else enc_out.device)))

    def step(self, X_new, pos=None, Y=None):
        """The output rows of the input rows X_new (n x d_model) at positions pos .. pos + n - 1
        (qgemm_decoder_step); pos defaults to the filled length, an earlier pos rewinds."""
        import torch
        _require_device_f32(X_new, "X_new")
        assert X_new.is_contiguous() and X_new.shape[1] == self.d_model
        if pos is None:
            pos = self.filled
            assert pos is not None, "step() follows begin()"
        Y = torch.empty_like(X_new) if Y is None else Y
        _require_device_f32(Y, "Y")
        assert Y.is_contiguous() and Y.shape == X_new.shape
        _check("qgemm_decoder_step", load().qgemm_decoder_step(self._h, X_new.data_ptr(), Y.data_ptr(), pos,
                                                              X_new.shape[0], _stream(X_new.device)))
        return Y

    def begin_slot(self, slot: int, enc_out=None):
        """begin() for one cache slot (qgemm_decoder_begin_slot); slot 0 is begin()'s."""
        enc_ptr, enc_seq = self._enc_args(enc_out)
        _check("qgemm_decoder_begin_slot",
               load().qgemm_decoder_begin_slot(self._h, slot, enc_ptr, enc_seq,
                                               _stream(None if enc_out is None else enc_out.device)))

    def step_slot(self, slot: int, X_new, pos=None, Y=None):
        """step() for one cache slot (qgemm_decoder_step_slot); pos defaults to the slot's filled length."""
        import torch
        _require_device_f32(X_new, "X_new")
        assert X_new.is_contiguous() and X_new.shape[1] == self.d_model
        if pos is None:
            pos = self.slot_filled(slot)
            assert pos is not None, "step_slot() follows begin_slot()"
        Y = torch.empty_like(X_new) if Y is None else Y
        _require_device_f32(Y, "Y")
        assert Y.is_contiguous() and Y.shape == X_new.shape
        _check("qgemm_decoder_step_slot", load().qgemm_decoder_step_slot(self._h, slot, X_new.data_ptr(), Y.data_ptr(),
                                                                        pos, X_new.shape[0], _stream(X_new.device)))
        return Y

    def step_batch(self, slots, X_new, pos=None, rows_per_seq: int = 1, Y=None):
        """One step of len(slots) sequences (qgemm_decoder_step_batch): rows b * rows_per_seq .. of X_new are the new
        rows of slot slots[b] at positions pos[b] .. (pos defaults to every slot's filled length); the rows of Y are,
        bit for bit, what step_slot gives for each sequence alone."""
        import torch
        _require_device_f32(X_new, "X_new")
        slots = [int(v) for v in slots]
        n = len(slots)
        assert X_new.is_contiguous() and X_new.shape == (n * rows_per_seq, self.d_model), \
            "X_new: (len(slots) * rows_per_seq) x d_model, contiguous"
        if pos is None:
            pos = [self.slot_filled(v) for v in slots]
            assert None not in pos, "step_batch() follows every slot's begin_slot()"
        Y = torch.empty_like(X_new) if Y is None else Y
        _require_device_f32(Y, "Y")
        assert Y.is_contiguous() and Y.shape == X_new.shape
        _check("qgemm_decoder_step_batch",
               load().qgemm_decoder_step_batch(self._h, n, _int_array(slots, n, "slots"), _int_array(pos, n, "pos"),
                                               rows_per_seq, X_new.data_ptr(), Y.data_ptr(), _stream(X_new.device)))
        return Y

    def step_varlen(self, slots, X_new, n_rows, pos=None, Y=None):
        """One step of len(slots) sequences with their own row counts (qgemm_decoder_step_varlen): X_new holds the new
        rows packed one after another, n_rows[b] >= 1 of them for slot slots[b] at positions pos[b] .. (pos defaults to
        every slot's filled length) -- a prefill of many slots, or prefills mixed with decoding rows.  The rows of Y
        are, bit for bit, what step_slot gives for each sequence alone."""
        import torch
        _require_device_f32(X_new, "X_new")
        slots, n_rows = [int(v) for v in slots], [int(v) for v in n_rows]
        n = len(slots)
        assert len(n_rows) == n, "n_rows: one entry per slot"
        assert X_new.is_contiguous() and X_new.shape == (sum(n_rows), self.d_model), \
            "X_new: sum(n_rows) x d_model, contiguous"
        if pos is None:
            pos = [self.slot_filled(v) for v in slots]
            assert None not in pos, "step_varlen() follows every slot's begin_slot()"
        Y = torch.empty_like(X_new) if Y is None else Y
        _require_device_f32(Y, "Y")
        assert Y.is_contiguous() and Y.shape == X_new.shape
        _check("qgemm_decoder_step_varlen",
               load().qgemm_decoder_step_varlen(self._h, n, _int_array(slots, n, "slots"), _int_array(pos, n, "pos"),
                                                _int_array(n_rows, n, "n_rows"), X_new.data_ptr(), Y.data_ptr(),
                                                _stream(X_new.device)))
        return Y

    def generate(self, head, slots, tokens_in, n_new: int, pos=None, tokens_out=None):
        """Greedy decoding of the cache slots `slots` for n_new tokens in one enqueued call (qgemm_decoder_generate):
        per step head.embed of the last tokens, step_batch, head.next_tokens, the tokens staying on the device.
        tokens_in: int32[len(slots)] on the device; returns tokens_out, int32[n_new x len(slots)] on the device, row t
        the tokens chosen at step t.  pos defaults to every slot's filled length, an earlier pos rewinds.  It does not
        stop at an end token."""
        import torch
        slots = [int(v) for v in slots]
        n = len(slots)
        _require_device_i32(tokens_in, "tokens_in", n)
        if tokens_out is None:
            tokens_out = torch.empty((n_new, n), dtype=torch.int32, device=tokens_in.device)
        _require_device_i32(tokens_out, "tokens_out", n_new * n)
        _check("qgemm_decoder_generate",
               load().qgemm_decoder_generate(self._h, head._h, n, _int_array(slots, n, "slots"), tokens_in.data_ptr(),
                                             n_new, _int_array(pos, n, "pos"), tokens_out.data_ptr(),
                                             _stream(tokens_in.device)))
        return tokens_out

    def generate_sampled(self, head, slots, tokens_in, n_new: int, top_k: int, top_p: float = 1.0,
                         temperature: float = 1.0, seed: int = 0, streams=None, eos=None, pos=None, tokens_out=None):
        """generate() with head.sample_tokens in head.next_tokens' place (qgemm_decoder_generate_sampled): sequence b
        draws at step t with the counter (streams[b] << 32) + pos[b] + t (streams defaults to the slots), so its tokens
        depend neither on its batch neighbours nor on how n_new is split over calls, and a rewind repeats its draws.
        With an end token eos, a sequence that has produced it keeps producing it while its steps run on."""
        import torch
        slots = [int(v) for v in slots]
        n = len(slots)
        _require_device_i32(tokens_in, "tokens_in", n)
        if tokens_out is None:
            tokens_out = torch.empty((n_new, n), dtype=torch.int32, device=tokens_in.device)
        _require_device_i32(tokens_out, "tokens_out", n_new * n)
        _check("qgemm_decoder_generate_sampled",
               load().qgemm_decoder_generate_sampled(self._h, head._h, n, _int_array(slots, n, "slots"),
                                                     tokens_in.data_ptr(), n_new, _int_array(pos, n, "pos"), top_k,
                                                     top_p, temperature, seed, _uint_array(streams, n, "streams", 32),
                                                     -1 if eos is None else int(eos), tokens_out.data_ptr(),
                                                     _stream(tokens_in.device)))
        return tokens_out

    def copy_slot(self, dst: int, src: int):
        """Fork a sequence (qgemm_decoder_copy_slot): slot dst continues slot src's sequence on its own."""
        _check("qgemm_decoder_copy_slot", load().qgemm_decoder_copy_slot(self._h, dst, src, _stream()))

    def gather_slots(self, dst_slots, src_slots, parents, n_rows, beams: int):
        """Reorder KV caches by a permutation on the device (qgemm_decoder_gather_slots): slot dst_slots[g * beams + i]
        takes the K and V thirds of self-cache rows 0 .. n_rows[g] - 1 of slot src_slots[g * beams + parents[g * beams +
        i]].  parents: int32 on the device; the slot lists and n_rows (one entry per group) are host values.  A parent
        outside [0, beams) gives that destination rows of quiet NaNs."""
        dst_slots, src_slots = [int(v) for v in dst_slots], [int(v) for v in src_slots]
        rows = len(dst_slots)
        assert beams >= 1 and rows % beams == 0 and len(src_slots) == rows, "beams slots per group in both lists"
        _require_device_i32(parents, "parents", rows)
        n = rows // beams
        _check("qgemm_decoder_gather_slots",
               load().qgemm_decoder_gather_slots(self._h, n, beams, _int_array(dst_slots, rows, "dst_slots"),
                                                 _int_array(src_slots, rows, "src_slots"), parents.data_ptr(),
                                                 _int_array(n_rows, n, "n_rows"), _stream(parents.device)))

    def read_slot(self, block: int, slot: int):
        """(self, cross): copies of block `block`'s cache slabs of one slot as they are (qgemm_decoder_read_slot),
        max_seq x 3 d_model rows [Q | K | V] and max_enc_seq x 2 d_model rows [K2 | V2], for inspection."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        self_rows = torch.empty((self.max_seq, 3 * self.d_model), dtype=torch.float32, device=dev)
        cross_rows = torch.empty((self.max_enc_seq, 2 * self.d_model), dtype=torch.float32, device=dev)
        # (decoder-only: no cross slab, 0 rows back)
        cross_ptr = None if getattr(self, "decoder_only", False) else cross_rows.data_ptr()
        _check("qgemm_decoder_read_slot", load().qgemm_decoder_read_slot(self._h, block, slot, self_rows.data_ptr(),
                                                                        cross_ptr, _stream(dev)))
        return self_rows, cross_rows

    def beam_fork(self, slot: int, slots_a, slots_b):
        """Start a group's beams from the sequence in `slot` (copy_slot into every other slot of the two sets): they
        then share its cross cache, which generate_beam needs, and its self cache so far."""
        for dst in list(slots_a) + list(slots_b):
            if int(dst) != int(slot):
                self.copy_slot(int(dst), int(slot))

    def generate_beam(self, head, slots_a, slots_b, tokens_in, n_new: int, beams: int, pos=None, scores_in=None,
                      eos: int = -1, out=None):
        """Beam search for n_new tokens in one enqueued call (qgemm_decoder_generate_beam): per step head.embed,
        step_batch on the slot set that holds the beams, head.beam_step, gather_slots into the other set by the
        parents just chosen.  slots_a / slots_b: two sets of n_groups * beams distinct begun slots (beam_fork makes
        them); the beams' caches are in slots_a.  tokens_in: int32[rows] on the device, or [n_groups] (every beam of a
        group then starts from the same token).  scores_in None: the start (beam 0 of each group alone is live).  pos:
        one host int per group, default the filled length of the group's first slot.  Returns (tokens, parents,
        scores), each n_new x rows on the device; afterwards the caches are in slots_a for an even n_new, else in
        slots_b.  A second call with the sets in their new roles, tokens[-1] and scores[-1] continues bit for bit."""
        import torch
        slots_a, slots_b = [int(v) for v in slots_a], [int(v) for v in slots_b]
        rows = len(slots_a)
        assert beams >= 1 and rows % beams == 0 and len(slots_b) == rows, "beams slots per group in both sets"
        n = rows // beams
        assert isinstance(tokens_in, torch.Tensor), "tokens_in: an int32 device tensor"
        if tokens_in.numel() == n and n != rows:
            tokens_in = tokens_in.repeat_interleave(beams).contiguous()
        _require_device_i32(tokens_in, "tokens_in", rows)
        if scores_in is not None:
            assert scores_in.is_cuda and scores_in.dtype == torch.float32 and scores_in.is_contiguous() and \
                scores_in.numel() == rows, "scores_in: float32[rows] on the device"
        if out is None:
            out = (torch.empty((n_new, rows), dtype=torch.int32, device=tokens_in.device),
                   torch.empty((n_new, rows), dtype=torch.int32, device=tokens_in.device),
                   torch.empty((n_new, rows), dtype=torch.float32, device=tokens_in.device))
        tokens, parents, scores = out
        _require_device_i32(tokens, "tokens", n_new * rows)
        _require_device_i32(parents, "parents", n_new * rows)
        assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and \
            scores.numel() == n_new * rows, "scores: float32[n_new x rows] on the device"
        _check("qgemm_decoder_generate_beam",
               load().qgemm_decoder_generate_beam(self._h, head._h, n, beams, _int_array(slots_a, rows, "slots_a"),
                                                  _int_array(slots_b, rows, "slots_b"), tokens_in.data_ptr(), n_new,
                                                  _int_array(pos, n, "pos"),
                                                  None if scores_in is None else scores_in.data_ptr(), int(eos),
                                                  tokens.data_ptr(), parents.data_ptr(), scores.data_ptr(),
                                                  _stream(tokens_in.device)))
        return tokens, parents, scores

    def beam_begin(self, slots, src_slots, pos, beams: int):
        """Start the copy-free search's beams (qgemm_decoder_beam_begin): the slots slots[g * beams + q]
        of group g get row-table entries 0 .. pos[g] - 1 = src_slots[g], the slot that holds the group's prompt, its
        enc_seq and filled = pos[g].  Nothing is copied; the slots need not have been begun, and slots[g * beams] may
        be src_slots[g].  pos None: every prompt's filled length."""
        slots, src_slots = [int(v) for v in slots], [int(v) for v in src_slots]
        rows, n = len(slots), len(src_slots)
        assert beams >= 1 and rows == n * beams, "beams slots per group, one prompt slot per group"
        if pos is None:
            pos = [self.slot_filled(v) for v in src_slots]
            assert None not in pos, "beam_begin() follows every prompt slot's begin_slot()"
        _check("qgemm_decoder_beam_begin",
               load().qgemm_decoder_beam_begin(self._h, n, beams, _int_array(slots, rows, "slots"),
                                               _int_array(src_slots, n, "src_slots"), _int_array(pos, n, "pos"),
                                               _stream()))

    def step_batch_indirect(self, slots, cross_slots, X_new, pos=None, rows_per_seq: int = 1, Y=None):
        """step_batch on slots begun by beam_begin (qgemm_decoder_step_batch_indirect): the new K / V rows go into each
        slot's own slab, the row table names them, the self-attention reads through the table and the cross-attention
        uses the cross cache of cross_slots[b] (a group's prompt slot)."""
        import torch
        _require_device_f32(X_new, "X_new")
        slots, cross_slots = [int(v) for v in slots], [int(v) for v in cross_slots]
        n = len(slots)
        assert len(cross_slots) == n, "cross_slots: one entry per slot"
        assert X_new.is_contiguous() and X_new.shape == (n * rows_per_seq, self.d_model), \
            "X_new: (len(slots) * rows_per_seq) x d_model, contiguous"
        if pos is None:
            pos = [self.slot_filled(v) for v in slots]
            assert None not in pos, "step_batch_indirect() follows beam_begin()"
        Y = torch.empty_like(X_new) if Y is None else Y
        _require_device_f32(Y, "Y")
        assert Y.is_contiguous() and Y.shape == X_new.shape
        _check("qgemm_decoder_step_batch_indirect",
               load().qgemm_decoder_step_batch_indirect(self._h, n, _int_array(slots, n, "slots"),
                                                        _int_array(cross_slots, n, "cross_slots"),
                                                        _int_array(pos, n, "pos"), rows_per_seq, X_new.data_ptr(),
                                                        Y.data_ptr(), _stream(X_new.device)))
        return Y

    def beam_reindex(self, slots, parents, n_rows, beams: int):
        """The search's reorder on the decoder's row table, in place (qgemm_decoder_beam_reindex): slot
        slots[g * beams + q] continues the hypothesis of slots[g * beams + parents[g * beams + q]] over its first
        n_rows[g] positions.  parents: int32 on the device; only table bytes move."""
        slots = [int(v) for v in slots]
        rows = len(slots)
        assert beams >= 1 and rows % beams == 0, "beams slots per group"
        _require_device_i32(parents, "parents", rows)
        n = rows // beams
        _check("qgemm_decoder_beam_reindex",
               load().qgemm_decoder_beam_reindex(self._h, n, beams, _int_array(slots, rows, "slots"),
                                                 parents.data_ptr(), _int_array(n_rows, n, "n_rows"),
                                                 _stream(parents.device)))

    def beam_table(self):
        """A copy of the decoder's row table as it is, uint8 [n_slots, max_seq] on the device
        (qgemm_decoder_read_beam_table): entry [s][j] is the slot whose slab holds row j of slot s's sequence."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((self.n_slots, self.max_seq), dtype=torch.uint8, device=dev)
        _check("qgemm_decoder_read_beam_table", load().qgemm_decoder_read_beam_table(self._h, out.data_ptr(),
                                                                                    _stream(dev)))
        return out

    def generate_beam_indirect(self, head, slots, src_slots, tokens_in, n_new: int, beams: int, pos=None,
                               scores_in=None, eos: int = -1, out=None):
        """generate_beam over ONE slot set without copying a cache row (qgemm_decoder_generate_beam_indirect): per step
        head.embed, step_batch_indirect (cross slots: the groups' prompt slots src_slots), head.beam_step, beam_reindex
        by the parents just chosen.  slots: n_groups * beams slots begun by beam_begin from src_slots; up to 64 rows.
        tokens_in, scores_in, pos, eos and the returned (tokens, parents, scores) are generate_beam's, bit for bit; a
        second call with tokens[-1] and scores[-1] continues, without another beam_begin."""
        import torch
        slots, src_slots = [int(v) for v in slots], [int(v) for v in src_slots]
        rows, n = len(slots), len(src_slots)
        assert beams >= 1 and rows == n * beams, "beams slots per group, one prompt slot per group"
        assert isinstance(tokens_in, torch.Tensor), "tokens_in: an int32 device tensor"
        if tokens_in.numel() == n and n != rows:
            tokens_in = tokens_in.repeat_interleave(beams).contiguous()
        _require_device_i32(tokens_in, "tokens_in", rows)
        if scores_in is not None:
            assert scores_in.is_cuda and scores_in.dtype == torch.float32 and scores_in.is_contiguous() and \
                scores_in.numel() == rows, "scores_in: float32[rows] on the device"
        if out is None:
            out = (torch.empty((n_new, rows), dtype=torch.int32, device=tokens_in.device),
                   torch.empty((n_new, rows), dtype=torch.int32, device=tokens_in.device),
                   torch.empty((n_new, rows), dtype=torch.float32, device=tokens_in.device))
        tokens, parents, scores = out
        _require_device_i32(tokens, "tokens", n_new * rows)
        _require_device_i32(parents, "parents", n_new * rows)
        assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and \
            scores.numel() == n_new * rows, "scores: float32[n_new x rows] on the device"
        _check("qgemm_decoder_generate_beam_indirect",
               load().qgemm_decoder_generate_beam_indirect(self._h, head._h, n, beams, _int_array(slots, rows, "slots"),
                                                           _int_array(src_slots, n, "src_slots"), tokens_in.data_ptr(),
                                                           n_new, _int_array(pos, n, "pos"),
                                                           None if scores_in is None else scores_in.data_ptr(),
                                                           int(eos), tokens.data_ptr(), parents.data_ptr(),
                                                           scores.data_ptr(), _stream(tokens_in.device)))
        return tokens, parents, scores

    def close(self):
        if getattr(self, "_h", None):
            load().qgemm_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _require_device_i32(t, name, count: int):
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), \
        f"{name}: a contiguous int32 device tensor"
    assert t.numel() == count, f"{name}: {count} entries"


def _require_rows_f32(t, name, cols=None):
    """A 2-D fp32 device tensor or view with unit inner stride and a row stride of at least its width."""
    _require_device_f32(t, name)
    assert t.stride(1) == 1 or t.shape[1] == 1, f"{name} must have unit inner stride"
    assert t.shape[0] <= 1 or t.stride(0) >= t.shape[1], f"{name}: the row stride covers a row"
    assert cols is None or t.shape[1] == cols, f"{name}: {cols} columns"
    return max(t.stride(0), t.shape[1])  # a one-row view may report any row stride


def argmax_rows_plan(rows: int, w: int) -> int:
    """The number of workgroups argmax_rows() gives each row (qgemm_argmax_rows_plan): 1, or more for few, wide rows.
    Needs no GPU; raises QGemmError for rows < 0, w < 1 or w > 2**24."""
    parts = ctypes.c_int()
    _check("qgemm_argmax_rows_plan", load().qgemm_argmax_rows_plan(rows, w, ctypes.byref(parts)))
    return parts.value


def argmax_rows(S, idx=None, val=None):
    """Row-wise argmax of a 2-D fp32 device tensor or view with unit inner stride (qgemm_argmax_rows), the reference's
    op_argmax chain: the lowest index among equal maxima, a NaN past column 0 never wins, a NaN at column 0 is never
    beaten.  Returns (idx, val): int32 indices and the winners' values, bit for bit.  S is not written."""
    import torch
    stride = _require_rows_f32(S, "S")
    rows, w = S.shape
    if idx is None:
        idx = torch.empty(rows, dtype=torch.int32, device=S.device)
    if val is None:
        val = torch.empty(rows, dtype=torch.float32, device=S.device)
    _require_device_i32(idx, "idx", rows)
    assert val.is_cuda and val.dtype == torch.float32 and val.is_contiguous() and val.numel() == rows, "val: as idx"
    L = load()
    need = L.qgemm_argmax_rows_workspace_size(rows, w)
    ws = torch.empty(need, dtype=torch.uint8, device=S.device) if need else None
    _check("qgemm_argmax_rows", L.qgemm_argmax_rows(S.data_ptr(), stride, rows, w, idx.data_ptr(), val.data_ptr(),
                                                    ws.data_ptr() if need else None, need, _stream(S.device)))
    return idx, val


def _uint_array(values, n: int, name: str, bits: int):
    """A host array of n unsigned 32- or 64-bit entries for the C-ABI (None stays NULL)."""
    if values is None:
        return None
    values = [int(v) for v in values]
    assert len(values) == n and all(0 <= v < 1 << bits for v in values), f"{name}: {n} unsigned {bits}-bit entries"
    return ((ctypes.c_uint32 if bits == 32 else ctypes.c_uint64) * max(1, n))(*values)


def sample_rows_plan(rows: int, w: int, top_k: int) -> int:
    """The number of workgroups sample_rows() gives each row in its first launch (qgemm_sample_rows_plan): 1, or more
    for few, wide rows.  Needs no GPU; raises QGemmError for rows < 0, w outside 1 .. 2**24 or top_k outside 1 .. 1024."""
    parts = ctypes.c_int()
    _check("qgemm_sample_rows_plan", load().qgemm_sample_rows_plan(rows, w, top_k, ctypes.byref(parts)))
    return parts.value


def sample_rows(S, top_k: int, top_p: float = 1.0, temperature: float = 1.0, seed: int = 0, counter0: int = 0,
                counters=None, prev=None, eos=None, idx=None, return_top: bool = False):
    """One seeded draw per row of a 2-D fp32 device tensor or view with unit inner stride (qgemm_sample_rows): the top_k
    best columns in argmax_rows' order (NaN and -inf never among them), their softmax_rows at scale 1 / temperature, the
    nucleus top_p inside that list, and the draw of counter counters[r] (host ints, at most 64 rows) or
    counter0 + (r << 32).  temperature 0 is greedy.  With prev (int32 on the device) and eos, a row whose prev is eos
    gets eos.  Returns idx (int32 tokens), or with return_top (idx, top_idx, top_prob, n_kept): the sorted list, its
    probabilities bit for bit (-1 / +0 past the candidates) and the length of the nucleus.  S is not written."""
    import torch
    stride = _require_rows_f32(S, "S")
    rows, w = S.shape
    if idx is None:
        idx = torch.empty(rows, dtype=torch.int32, device=S.device)
    _require_device_i32(idx, "idx", rows)
    if prev is not None:
        _require_device_i32(prev, "prev", rows)
    top_idx = top_prob = n_kept = None
    if return_top:
        top_idx = torch.empty((rows, top_k), dtype=torch.int32, device=S.device)
        top_prob = torch.empty((rows, top_k), dtype=torch.float32, device=S.device)
        n_kept = torch.empty(rows, dtype=torch.int32, device=S.device)
    L = load()
    need = L.qgemm_sample_rows_workspace_size(rows, w, top_k)
    ws = torch.empty(need, dtype=torch.uint8, device=S.device) if need else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _check("qgemm_sample_rows",
           L.qgemm_sample_rows(S.data_ptr(), stride, rows, w, top_k, top_p, temperature, seed, counter0,
                               _uint_array(counters, rows, "counters", 64), ptr(prev), -1 if eos is None else int(eos),
                               idx.data_ptr(), ptr(top_idx), ptr(top_prob), ptr(n_kept), ptr(ws), need,
                               _stream(S.device)))
    return (idx, top_idx, top_prob, n_kept) if return_top else idx


def logsumexp_rows_plan(rows: int, w: int) -> int:
    """The number of workgroups logsumexp_rows() gives each row (qgemm_logsumexp_rows_plan): 1, or more for few, wide
    rows, each a run of whole 1024-column blocks.  Needs no GPU; raises QGemmError for rows < 0 or w outside 1 .. 2**24."""
    parts = ctypes.c_int()
    _check("qgemm_logsumexp_rows_plan", load().qgemm_logsumexp_rows_plan(rows, w, ctypes.byref(parts)))
    return parts.value


def logsumexp_rows(S, mx=None, logz=None):
    """(mx, logz) of every row of a 2-D fp32 device tensor or view with unit inner stride (qgemm_logsumexp_rows): mx the
    greatest candidate (S[i] > -inf) in argmax_rows' order, logz = fl32(log(sum)) with the sum of the correctly rounded
    exp(S[i] - mx) over the candidates taken by one fixed binary tree, so that every bit is predictable and independent
    of the launch plan.  The log-probability of column i is fl(fl(S[i] - mx) - logz).  S is not written."""
    import torch
    stride = _require_rows_f32(S, "S")
    rows, w = S.shape
    if mx is None:
        mx = torch.empty(rows, dtype=torch.float32, device=S.device)
    if logz is None:
        logz = torch.empty(rows, dtype=torch.float32, device=S.device)
    for t, name in ((mx, "mx"), (logz, "logz")):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows, \
            f"{name}: float32[rows] on the device"
    L = load()
    need = L.qgemm_logsumexp_rows_workspace_size(rows, w)
    ws = torch.empty(need, dtype=torch.uint8, device=S.device) if need else None
    _check("qgemm_logsumexp_rows", L.qgemm_logsumexp_rows(S.data_ptr(), stride, rows, w, mx.data_ptr(), logz.data_ptr(),
                                                          ws.data_ptr() if need else None, need, _stream(S.device)))
    return mx, logz


def beam_step_plan(n_groups: int, beams: int, w: int) -> tuple:
    """(select_parts, lse_parts) of beam_step() (qgemm_beam_step_plan): the workgroups a row gets in the selection's
    first launch and in the log-sum-exp's.  Needs no GPU; raises QGemmError outside 1 <= beams <= 8,
    n_groups * beams <= 64, 1 <= w <= 2**24."""
    sp, lp = ctypes.c_int(), ctypes.c_int()
    _check("qgemm_beam_step_plan", load().qgemm_beam_step_plan(n_groups, beams, w, ctypes.byref(sp), ctypes.byref(lp)))
    return sp.value, lp.value


def _beam_outputs(rows, device, out):
    import torch
    if out is None:
        out = (torch.empty(rows, dtype=torch.int32, device=device), torch.empty(rows, dtype=torch.int32, device=device),
               torch.empty(rows, dtype=torch.float32, device=device))
    parents, tokens, scores = out
    _require_device_i32(parents, "parents", rows)
    _require_device_i32(tokens, "tokens", rows)
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.numel() == rows, \
        "scores: float32[rows] on the device"
    return parents, tokens, scores


def _beam_inputs(rows, scores_in, prev):
    import torch
    if scores_in is not None:
        assert scores_in.is_cuda and scores_in.dtype == torch.float32 and scores_in.is_contiguous() and \
            scores_in.numel() == rows, "scores_in: float32[rows] on the device"
    if prev is not None:
        _require_device_i32(prev, "prev", rows)
    return (None if scores_in is None else scores_in.data_ptr()), (None if prev is None else prev.data_ptr())


def beam_step(S, beams: int, scores_in=None, prev=None, eos: int = -1, out=None):
    """One step of beam search on the logits S, a 2-D fp32 device tensor or view of n_groups * beams rows
    (qgemm_beam_step): every live beam's best `beams` columns scored as fl(score + log-probability), finished beams
    (prev == eos) held with their score, dead beams (score not > -inf) dropped, and the best `beams` candidates of every
    group chosen -- greater score first, the lower beam * beams + rank among equal scores.  scores_in None: the start.
    Returns (parents, tokens, scores): int32, int32 and float32 [rows] on the device."""
    stride = _require_rows_f32(S, "S")
    rows, w = S.shape
    assert beams >= 1 and rows % beams == 0, "S: beams rows per group"
    parents, tokens, scores = _beam_outputs(rows, S.device, out)
    sc, pv = _beam_inputs(rows, scores_in, prev)
    import torch
    L = load()
    need = L.qgemm_beam_step_workspace_size(rows // beams, beams, w)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=S.device)
    _check("qgemm_beam_step", L.qgemm_beam_step(S.data_ptr(), stride, rows // beams, beams, w, sc, pv, int(eos),
                                                parents.data_ptr(), tokens.data_ptr(), scores.data_ptr(), ws.data_ptr(),
                                                need, _stream(S.device)))
    return parents, tokens, scores


def beam_hypotheses(tokens, parents, scores, eos: int = -1, beams=None):
    """Backtrack a finished search on the host: tokens / parents / scores are generate_beam's outputs (n_new x rows;
    several calls' outputs concatenated along the first axis are fine).  beams defaults to rows (one group).  Returns,
    for every final place, (token list, score): the tokens along its parent chain, cut after the first eos; a dead
    place (score -inf) has an empty list."""
    import numpy as np
    tok, par, sc = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (tokens, parents, scores))
    steps, rows = tok.shape
    beams = rows if beams is None else int(beams)
    assert rows % beams == 0, "beams rows per group"
    out = []
    for r in range(rows):
        score = float(sc[-1, r]) if steps else 0.0
        if not score > float("-inf"):
            out.append(([], score))
            continue
        seq, at = [], r
        for t in range(steps - 1, -1, -1):
            seq.append(int(tok[t, at]))
            at = at // beams * beams + int(par[t, at])
        seq.reverse()
        if eos >= 0 and eos in seq:
            seq = seq[:seq.index(eos) + 1]
        out.append((seq, score))
    return out


def embed_rows(E, tokens, P=None, pos=None, rows_per_seq: int = 1, Y=None):
    """Y[r] = E[tokens[r]] (+ P[pos[r // rows_per_seq] + r % rows_per_seq], one fp32 add): the token embedding gather
    (qgemm_embed_rows).  tokens: int32 on the device, rows_per_seq per sequence; pos: one host int per sequence.  E, P
    and Y may be row-strided views.  A token outside the vocabulary gives a row of quiet NaNs."""
    import torch
    es = _require_rows_f32(E, "E")
    vocab, d = E.shape
    assert isinstance(tokens, torch.Tensor), "tokens: an int32 device tensor"
    rows = tokens.numel()
    _require_device_i32(tokens, "tokens", rows)
    assert rows_per_seq >= 1 and rows % rows_per_seq == 0, "tokens holds rows_per_seq entries per sequence"
    n = rows // rows_per_seq
    ps = 0
    if P is not None:
        ps = _require_rows_f32(P, "P", d)
        assert pos is not None, "a position table needs pos"
    if Y is None:
        Y = torch.empty((rows, d), dtype=torch.float32, device=E.device)
    ys = _require_rows_f32(Y, "Y", d)
    assert Y.shape[0] == rows
    _check("qgemm_embed_rows",
           load().qgemm_embed_rows(E.data_ptr(), es, vocab, d, tokens.data_ptr(), None if P is None else P.data_ptr(),
                                   ps, 0 if P is None else P.shape[0],
                                   _int_array(pos if P is not None else None, n, "pos"), n, rows_per_seq, Y.data_ptr(),
                                   ys, _stream(E.device)))
    return Y


class Head:
    """The vocabulary head (qgemm_head_*): logits() is linear(H, pw, bias) onto the vocabulary, next_tokens() its
    row-wise argmax, embed() the token (+ position) embedding that feeds the next decoder step -- what
    Decoder.generate() chains on the device.  pw: a d_model x vocab weight packed by pack_b (a tied head:
    pack_b(E.t())); bias, E (vocab x d_model) and P (max_pos x d_model) are optional.  The head keeps references to
    them and owns its logits buffer, row buffers and workspaces for up to max_rows rows."""

    def __init__(self, pw: Packed, vocab: int, bias=None, E=None, P=None, max_rows: int = 64):
        import torch
        assert pw.rows == vocab, "pw: d_model x vocab, packed by pack_b"
        assert pw.range == DEFAULT_RANGE, f"the head needs a weight packed with range {DEFAULT_RANGE}"
        self.d_model, self.vocab, self.max_rows = pw.k, vocab, int(max_rows)
        es = ps = 0
        if bias is not None:
            assert bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == vocab
        if E is not None:
            es = _require_rows_f32(E, "E", self.d_model)
            assert E.shape[0] == vocab, "E: vocab x d_model"
        if P is not None:
            assert E is not None, "a position table belongs to an embedding table"
            ps = _require_rows_f32(P, "P", self.d_model)
        self._keep = (pw, bias, E, P)  # borrowed by the C object
        self.has_positions = P is not None
        h = ctypes.c_void_p()
        _check("qgemm_head_create",
               load().qgemm_head_create(pw.buf.data_ptr(), self.d_model, vocab, None if bias is None else bias.data_ptr(),
                                        None if E is None else E.data_ptr(), es, None if P is None else P.data_ptr(),
                                        ps, 0 if P is None else P.shape[0], self.max_rows, ctypes.byref(h)))
        self._h = h

    def logits(self, H, out=None):
        """linear(H, pw, bias) without relu, bit for bit (qgemm_head_logits): rows x vocab, fp32."""
        import torch
        hs = _require_rows_f32(H, "H", self.d_model)
        if out is None:
            out = torch.empty((H.shape[0], self.vocab), dtype=torch.float32, device=H.device)
        os_ = _require_rows_f32(out, "out", self.vocab)
        assert out.shape[0] == H.shape[0]
        _check("qgemm_head_logits", load().qgemm_head_logits(self._h, H.data_ptr(), hs, H.shape[0], out.data_ptr(), os_,
                                                            _stream(H.device)))
        return out

    def next_tokens(self, H, tokens=None):
        """The argmax over the vocabulary of every row's logits (qgemm_head_next_tokens): int32 on the device."""
        import torch
        hs = _require_rows_f32(H, "H", self.d_model)
        if tokens is None:
            tokens = torch.empty(H.shape[0], dtype=torch.int32, device=H.device)
        _require_device_i32(tokens, "tokens", H.shape[0])
        _check("qgemm_head_next_tokens", load().qgemm_head_next_tokens(self._h, H.data_ptr(), hs, H.shape[0],
                                                                      tokens.data_ptr(), _stream(H.device)))
        return tokens

    def sample_tokens(self, H, top_k: int, top_p: float = 1.0, temperature: float = 1.0, seed: int = 0,
                      counter0: int = 0, counters=None, prev=None, eos=None, tokens=None):
        """One draw per row from the row's logits (qgemm_head_sample_tokens): sample_rows in next_tokens' argmax's
        place, with its arguments; int32 on the device."""
        import torch
        hs = _require_rows_f32(H, "H", self.d_model)
        rows = H.shape[0]
        if tokens is None:
            tokens = torch.empty(rows, dtype=torch.int32, device=H.device)
        _require_device_i32(tokens, "tokens", rows)
        if prev is not None:
            _require_device_i32(prev, "prev", rows)
        _check("qgemm_head_sample_tokens",
               load().qgemm_head_sample_tokens(self._h, H.data_ptr(), hs, rows, top_k, top_p, temperature, seed,
                                               counter0, _uint_array(counters, rows, "counters", 64),
                                               None if prev is None else prev.data_ptr(),
                                               -1 if eos is None else int(eos), tokens.data_ptr(), _stream(H.device)))
        return tokens

    def beam_step(self, H, beams: int, scores_in=None, prev=None, eos: int = -1, out=None):
        """beam_step on the logits of H's rows (qgemm_head_beam_step): logits into the head's buffer, then the step,
        with its arguments; returns (parents, tokens, scores) on the device."""
        hs = _require_rows_f32(H, "H", self.d_model)
        rows = H.shape[0]
        assert beams >= 1 and rows % beams == 0, "H: beams rows per group"
        parents, tokens, scores = _beam_outputs(rows, H.device, out)
        sc, pv = _beam_inputs(rows, scores_in, prev)
        _check("qgemm_head_beam_step",
               load().qgemm_head_beam_step(self._h, H.data_ptr(), hs, rows // beams, beams, sc, pv, int(eos),
                                           parents.data_ptr(), tokens.data_ptr(), scores.data_ptr(), _stream(H.device)))
        return parents, tokens, scores

    def embed(self, tokens, pos=None, rows_per_seq: int = 1, Y=None):
        """embed_rows on the head's tables (qgemm_head_embed); pos is needed with a position table."""
        import torch
        assert isinstance(tokens, torch.Tensor), "tokens: an int32 device tensor"
        rows = tokens.numel()
        _require_device_i32(tokens, "tokens", rows)
        assert rows_per_seq >= 1 and rows % rows_per_seq == 0, "tokens holds rows_per_seq entries per sequence"
        n = rows // rows_per_seq
        assert pos is not None or not self.has_positions, "a head with a position table needs pos"
        if Y is None:
            Y = torch.empty((rows, self.d_model), dtype=torch.float32, device=tokens.device)
        ys = _require_rows_f32(Y, "Y", self.d_model)
        assert Y.shape[0] == rows
        _check("qgemm_head_embed", load().qgemm_head_embed(self._h, tokens.data_ptr(), _int_array(pos, n, "pos"), n,
                                                          rows_per_seq, Y.data_ptr(), ys, _stream(tokens.device)))
        return Y

    def close(self):
        if getattr(self, "_h", None):
            load().qgemm_head_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_uniform(t, seed: int, lo: float = -1.0, hi: float = 1.0):
    """Seeded U[lo,hi) fill of a contiguous fp32 device tensor (bit-identical to the oracle's)."""
    assert t.is_contiguous()
    _check("qgemm_fill_uniform", load().qgemm_fill_uniform(t.data_ptr(), t.numel(), seed, lo, hi, _stream(t.device)))
    return t


