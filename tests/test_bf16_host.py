"""The bf16 entry points (qgemm_pack_a_dt / qgemm_mm_packed_dt / qgemm_linear_dt) without a GPU: declarations,
argument checks ahead of any launch, the wrappers' dtype rule, and the source hash."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "qgemm.h")
DT = ("qgemm_pack_a_dt", "qgemm_mm_packed_dt", "qgemm_linear_dt")
BAD_TAG = 2


def test_header_declares_the_entry_points_and_tags():
    text = open(HEADER).read()
    fns = re.findall(r"^QGEMM_API\s+[\w\s\*]+?\b((?:op_|qgemm_)\w+)\s*\(", text, flags=re.M)
    for f in DT:
        assert f in fns, f
    m = re.search(r"enum\s*\{([^}]*)\}", text)
    assert m, "the element-type tags are an enum"
    tags = dict(re.findall(r"(QGEMM_\w+)\s*=\s*(\d+)", m.group(1)))
    assert tags == {"QGEMM_F32": "0", "QGEMM_BF16": "1"}
    flat = " ".join(text.split())
    assert ("int qgemm_pack_a_dt(const void *A, int a_dtype, int64_t a_stride_h, int64_t a_stride_w, int m, int k, "
            "float range, void *packed_a, void *stream);") in flat
    assert ("int qgemm_mm_packed_dt(const void *packed_a, const void *packed_b, void *C, int c_dtype, int64_t c_stride_h, "
            "int64_t c_stride_w, int m, int n, int k, float range, void *stream);") in flat
    assert ("int qgemm_linear_dt(const void *X, int x_dtype, int64_t x_stride_h, int m, int k, const void *packed_w, int n, "
            "const float *bias, int relu, void *Y, int y_dtype, int64_t y_stride_h, void *workspace, size_t ws_bytes, "
            "void *stream);") in flat


def test_library_and_mirror_carry_the_entry_points(qg):
    out = subprocess.run(["nm", "-D", "--defined-only", qg.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in DT:
        assert f in exported and f in qg.EXPORTED_SYMBOLS, f
    assert (qg.QGEMM_F32, qg.QGEMM_BF16) == (0, 1)


@pytest.mark.parametrize("tag", [0, 1])
def test_invalid_arguments_return_invalid_value(qg, tag):
    """Null pointers, bad sizes and an undersized workspace are refused before any launch (no GPU is touched: the
    pointers are small integers that are never dereferenced on the host)."""
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    assert L.qgemm_pack_a_dt(None, tag, 4, 1, 4, 4, 127.0, 8, None) == bad
    assert L.qgemm_pack_a_dt(8, tag, 4, 1, 4, 4, 127.0, None, None) == bad
    assert L.qgemm_pack_a_dt(8, tag, 4, 1, 4, 0, 127.0, 8, None) == bad
    assert L.qgemm_pack_a_dt(8, tag, 4, 1, -1, 4, 127.0, 8, None) == bad
    assert L.qgemm_mm_packed_dt(None, 8, 8, tag, 4, 1, 4, 4, 4, 127.0, None) == bad
    assert L.qgemm_mm_packed_dt(8, None, 8, tag, 4, 1, 4, 4, 4, 127.0, None) == bad
    assert L.qgemm_mm_packed_dt(8, 8, None, tag, 4, 1, 4, 4, 4, 127.0, None) == bad
    assert L.qgemm_mm_packed_dt(8, 8, 8, tag, 4, 1, 4, 4, 0, 127.0, None) == bad
    need = L.qgemm_linear_workspace_size(4, 4, 4)
    assert need > 0
    for xt, yt in ((tag, 0), (tag, 1)):
        assert L.qgemm_linear_dt(None, xt, 4, 4, 4, 8, 4, None, 0, 8, yt, 4, 8, need, None) == bad
        assert L.qgemm_linear_dt(8, xt, 4, 4, 4, None, 4, None, 0, 8, yt, 4, 8, need, None) == bad
        assert L.qgemm_linear_dt(8, xt, 4, 4, 4, 8, 4, None, 0, None, yt, 4, 8, need, None) == bad
        assert L.qgemm_linear_dt(8, xt, 4, 4, 4, 8, 4, None, 1, 8, yt, 4, 8, need, None) == bad    # relu needs a bias
        assert L.qgemm_linear_dt(8, xt, 4, 4, 4, 8, 4, None, 0, 8, yt, 4, None, need, None) == bad  # no workspace
        assert L.qgemm_linear_dt(8, xt, 4, 4, 4, 8, 4, None, 0, 8, yt, 4, 8, need - 1, None) == bad  # too small
        assert L.qgemm_linear_dt(8, xt, 4, 4, 0, 8, 4, None, 0, 8, yt, 4, 8, need, None) == bad    # k = 0


def test_unknown_tag_returns_invalid_value(qg):
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    need = L.qgemm_linear_workspace_size(4, 4, 4)
    for t in (BAD_TAG, -1, 7):
        assert L.qgemm_pack_a_dt(8, t, 4, 1, 4, 4, 127.0, 8, None) == bad
        assert L.qgemm_mm_packed_dt(8, 8, 8, t, 4, 1, 4, 4, 4, 127.0, None) == bad
        assert L.qgemm_linear_dt(8, t, 4, 4, 4, 8, 4, None, 0, 8, 0, 4, 8, need, None) == bad
        assert L.qgemm_linear_dt(8, 1, 4, 4, 4, 8, 4, None, 0, 8, t, 4, 8, need, None) == bad
        # ahead of the empty-output shortcut too
        assert L.qgemm_linear_dt(8, t, 4, 0, 4, 8, 4, None, 0, 8, 1, 4, 8, need, None) == bad
        assert L.qgemm_mm_packed_dt(8, 8, 8, t, 4, 1, 0, 4, 4, 127.0, None) == bad


def test_empty_outputs_are_noops(qg):
    L = qg.load()
    for xt, yt in ((1, 1), (0, 1), (1, 0), (0, 0)):
        assert L.qgemm_linear_dt(8, xt, 4, 0, 4, 8, 4, None, 0, 8, yt, 4, 8, 1 << 20, None) == 0
        assert L.qgemm_linear_dt(8, xt, 4, 4, 4, 8, 0, None, 0, 8, yt, 4, 8, 1 << 20, None) == 0
    assert L.qgemm_pack_a_dt(8, 1, 4, 1, 0, 4, 127.0, 8, None) == 0
    assert L.qgemm_mm_packed_dt(8, 8, 8, 1, 4, 1, 0, 4, 4, 127.0, None) == 0
    assert L.qgemm_mm_packed_dt(8, 8, 8, 1, 4, 1, 4, 0, 4, 127.0, None) == 0


def test_linear_workspace_size_does_not_depend_on_the_types(qg):
    """One size function serves every type combination: [split-K scratch][packed A], both type-independent."""
    L = qg.load()
    for m, n, k in ((4096, 4096, 4096), (2048, 4096, 16384), (512, 1024, 1024), (3, 5, 7)):
        assert L.qgemm_linear_workspace_size(m, n, k) == L.op_mm_quantize_prepacked_workspace_size(m, n, k)


def test_wrappers_reject_other_dtypes(qg):
    """fp32 and bf16 only: fp16 (or anything else) still meets the float32 assertion, before any device work."""
    import torch
    h = torch.zeros((4, 8), dtype=torch.float16)
    pw = qg.Packed(None, 8, 8, qg.DEFAULT_RANGE)
    with pytest.raises(AssertionError, match="float32"):
        qg.pack_a(_FakeCuda(h))
    with pytest.raises(AssertionError, match="float32"):
        qg.linear(_FakeCuda(h), pw)
    with pytest.raises(AssertionError, match="float32"):
        qg.mm_packed(pw, pw, C=_FakeCuda(torch.zeros((8, 8), dtype=torch.float16)))
    with pytest.raises(AssertionError, match="out_dtype"):
        qg.mm_packed(pw, pw, out_dtype=torch.float16)
    # a CPU bf16 tensor is refused by the residency assert, as a CPU fp32 tensor is
    with pytest.raises(AssertionError, match="on_device"):
        qg.pack_a(torch.zeros((4, 8), dtype=torch.bfloat16))
    with pytest.raises(AssertionError, match="on_device"):
        qg.pack_a(torch.zeros((4, 8), dtype=torch.float32))


def _FakeCuda(t):
    """A CPU tensor that claims to be on the device, so the dtype assertion is what refuses it (no GPU here)."""
    import torch

    class T(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    return t.as_subclass(T)


def test_source_hash_matches_a_fresh_build(qg):
    """The new sources are part of the hash the binary carries."""
    h = qg.source_hash()
    assert qg.file_hash() == h and f"src={h}" in qg.version()
    assert qg.check_binary() == h
