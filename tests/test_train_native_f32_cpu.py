"""The fp32 native training step's host side (csrc/train.hip: sdn_train_layout_f32, sdn_train_step_f32): workspace arithmetic, the
argument checks made before any launch, and the exported, declared symbols.  No GPU needed."""
import ctypes
import os
import re

import numpy as np


def _offsets():
    off = (ctypes.c_int32 * 17)()
    rows, res = 0, [int(np.ceil(16 * np.exp2(np.log2(2048 / 16) / 15) ** i)) for i in range(16)]
    for i, r in enumerate(res):
        off[i] = rows
        rows += int(np.ceil(min(2 ** 19, (r + 1) ** 3) / 8) * 8)
    off[16] = rows
    return off, rows


def test_fp32_layout_is_aligned_inside_the_block_and_grows_with_the_batch():
    import sdn_backend as B
    off, rows = _offsets()
    small, big = B.SdnTrainLayout(), B.SdnTrainLayout()
    assert B.lib.sdn_train_layout_f32(4096, 9216, 1024, off, ctypes.byref(small)) == 0
    assert B.lib.sdn_train_layout_f32(8192, 18432, 1024, off, ctypes.byref(big)) == 0
    named = [f for f, _ in B.SdnTrainLayout._fields_ if f not in ("total_bytes", "sample_set_stride", "found_inf", "dirs", "deltas")]
    for f in named:
        v = getattr(small, f)
        assert v % 256 == 0 and v < small.total_bytes, f
    # no parameter copies exist in fp32
    assert all(getattr(small, f) == 0 for f in ("w_table", "w_deform", "w_sigma0", "w_sigma1", "w_color"))
    assert small.total_bytes < big.total_bytes and small.sample_set_stride % 256 == 0
    assert small.xyzs + small.sample_set_stride < small.total_bytes
    assert small.rays + small.sample_set_stride < small.total_bytes
    # the fp32 table gradient (rows x 2 floats) fits in front of the next buffer; the MLP gradients hold their flat fp32 shapes
    others = sorted(getattr(small, f) for f in named if getattr(small, f) > small.g_table)
    assert others[0] - small.g_table >= rows * 2 * 4
    assert small.g_sigma0 - small.g_deform >= (128 * 80 + 6 * 128 * 128 + 16 * 128) * 4
    assert small.g_sigma1 - small.g_sigma0 >= 64 * 32 * 4 and small.g_color - small.g_sigma1 >= 16 * 64 * 4
    assert small.total_bytes - small.g_color >= (64 * 32 + 64 * 64 + 16 * 64) * 4
    assert small.found_inf < small.total_bytes
    # N = 0, M = 0 and a missing offset table are refused
    assert B.lib.sdn_train_layout_f32(0, 9216, 1024, off, ctypes.byref(small)) == -1
    assert B.lib.sdn_train_layout_f32(4096, 0, 1024, off, ctypes.byref(small)) == -1
    assert B.lib.sdn_train_layout_f32(4096, 9216, 1024, None, ctypes.byref(small)) == -1


def test_fp32_step_refuses_a_record_it_cannot_run_before_any_launch():
    import sdn_backend as B
    rec = B.SdnTrainStep()
    assert B.lib.sdn_train_step_f32(ctypes.byref(rec), None) == -1
    assert B.lib.sdn_train_refresh_f32(ctypes.byref(rec), None) == -1
    # a record that is complete but for an unsupported option: optimizer-only mode (data parallelism) and the second table stream
    off, rows = _offsets()
    rec.workspace, rec.N, rec.M, rec.max_steps, rec.bound = 256, 16, 128, 1024, 1.0
    for i in range(17):
        rec.grid_offsets[i] = off[i]
    rec.mode = 2
    assert B.lib.sdn_train_step_f32(ctypes.byref(rec), None) == -1
    rec.mode, rec.table_stream = 0, 1
    assert B.lib.sdn_train_step_f32(ctypes.byref(rec), None) == -1


def test_fp32_symbols_are_exported_and_declared():
    import sdn_backend as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sdn_hip.h")).read(), flags=re.S)
    for name in ("sdn_train_layout_f32", "sdn_train_refresh_f32", "sdn_train_step_f32"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(B.lib, name) and name in B.PROTOTYPES, name
