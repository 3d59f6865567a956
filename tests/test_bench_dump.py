"""bench.py's --full / --dump-outputs plumbing on the CPU (no GPU): the options parse, the row sample is a
function of the shape alone and keeps a file under the size limit, and dump_outputs writes float32 .npy files."""
import os

import numpy as np
import torch

import bench


def test_full_is_off_by_default_and_dump_takes_a_directory():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    b = bench.parse(["--full", "--dump-outputs", "some/dir"])
    assert b.full is True and b.dump_outputs == "some/dir"


def test_dump_rows_is_fixed_and_fits_the_limit():
    assert bench.DUMP_LIMIT_BYTES <= 64_000_000 - 4096  # room for the .npy header
    for M, N in [(4096, 4096), (2048, 16384), (8192, 4096)]:  # the GEMM configs' outputs, all above the limit
        rows = bench.dump_rows(M, N * 4)
        assert rows is not None and len(rows) * N * 4 <= bench.DUMP_LIMIT_BYTES < (len(rows) + 1) * N * 4
        assert len(np.unique(rows)) == len(rows) and (np.diff(rows) > 0).all()
        assert rows.min() >= 0 and rows.max() < M
        assert np.array_equal(rows, bench.dump_rows(M, N * 4))
    assert bench.dump_rows(512, 1024 * 4) is None  # c5_encoder's Y fits whole
    assert bench.dump_rows(10, 4, limit=40) is None and len(bench.dump_rows(11, 4, limit=40)) == 10


def test_dump_outputs_writes_float32_npy(tmp_path, monkeypatch):
    out = tmp_path / "nested" / "dir"
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    rep = bench.dump_outputs(str(out), {"O": small})
    got = np.load(out / "O.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy()) and rep["O"]["rows"] == "all"
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 16)  # room for two of the three rows
    rep = bench.dump_outputs(str(out), {"O": small})
    got = np.load(out / "O.npy")
    rows = bench.dump_rows(3, 16, 32)
    assert got.shape == (2, 4) and np.array_equal(got, small.numpy()[rows]) and rep["O"]["shape"] == [2, 4]
    assert sorted(os.listdir(out)) == ["O.npy"]
