"""The error-map sampling and update (csrc/error_map.hip, the compositing launch of csrc/train.hip) as far as they can be checked
without a device: the numpy restatement the GPU tests compare against, `get_rays` without the native draw, argument validation, and
the layout of the three fields the training record gained."""
import os
import re

import numpy as np
import pytest
import torch

import error_map_support as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_draw_orders_by_key_with_ties_and_zeros_to_the_lower_cell():
    w = np.array([0.0, 2.0, 1.0, 0.0, 1.0, 4.0, 0.5], np.float32)
    u = np.full(7, np.exp(-1.0), np.float32)                       # q = 1: the keys are the weights
    order, keys = E.restated_draw(w, u, 7)
    assert order.tolist() == [5, 1, 2, 4, 6, 0, 3]                   # 2 before 4 (equal keys), the zeros last, 0 before 3
    np.testing.assert_allclose(keys, w, rtol=1e-6)
    assert E.restated_draw(w, u, 3)[0].tolist() == [5, 1, 2]
    # a smaller u means a larger q and a smaller key
    u2 = u.copy()
    u2[5] = 1e-6
    assert E.restated_draw(w, u2, 1)[0].tolist() == [1]


def test_restated_draw_has_at_most_two_cells_in_the_threshold_band_and_fp32_keys_pick_the_same_set():
    """The 36 seeded cases of the GPU test: the band that excuses a cell from the comparison holds at most BAND_MAX cells, and an
    fp32 evaluation of the keys (what the kernel computes) differs from the float64 draw by band cells only."""
    for kind in E.DRAW_MAPS:
        for seed in E.DRAW_SEEDS:
            for N in E.DRAW_NS:
                w, u, _ = E.draw_case(kind, seed, N)
                assert (u > 0).all() and (u < 1).all()
                want, keys = E.restated_draw(w, u, N)
                band = E.threshold_band(keys, N)
                assert band.size <= E.BAND_MAX, (kind, seed, N, band)
                got32, _ = E.restated_draw(w, u, N, dtype=np.float32)
                E.assert_same_draw(got32, w, u, N)


def test_fine_pixel_formula_in_fp32():
    # 800 x 800 over 128 cells: sx = 6.25; cell (3, 127) with r = (0.5, 0.999) -> x = int(18.75 + 3.125) = 21, y = int(793.75 + 6.24375) = 799
    assert E.fine_pixels([3 * 128 + 127], 128, 800, 800, [0.5], [0.999]).tolist() == [21 * 800 + 799]
    # 100 x 75: sx = 0.78125, sy = 0.5859375 < 1; the last cell lands on the last pixel, never past it
    r = np.float32(1 - 2.0 ** -24)
    assert E.fine_pixels([128 * 128 - 1], 128, 100, 75, [r], [r]).tolist() == [99 * 75 + 74]
    assert E.fine_pixels([0], 128, 100, 75, [0.0], [0.0]).tolist() == [0]
    x = E.fine_pixels(np.arange(128 * 128), 128, 100, 75, np.zeros(128 * 128), np.zeros(128 * 128))
    assert x.min() == 0 and x.max() == 99 * 75 + 74


def test_get_rays_without_the_native_draw_is_unchanged():
    """`native_error_map=False` (the default), and `True` with a map that is not on the GPU, draw with the reference's expressions:
    the same indices as those expressions under the same torch seed."""
    from dnerf_amd.utils import get_rays
    H, W, N = 40, 30, 200
    poses = torch.eye(4)[None]
    intr = np.array([35.0, 35.0, W / 2, H / 2])
    error_map = torch.rand(1, 128 * 128, generator=torch.Generator().manual_seed(1)) + 0.01
    for kw in ({}, {"native_error_map": False}, {"native_error_map": True}):
        torch.manual_seed(3)
        got = get_rays(poses, intr, H, W, N, error_map, **kw)
        torch.manual_seed(3)
        inds_coarse = torch.multinomial(error_map, N, replacement=False)
        sx, sy = H / 128, W / 128
        inds_x = ((inds_coarse // 128) * sx + torch.rand(1, N) * sx).long().clamp(max=H - 1)
        inds_y = ((inds_coarse % 128) * sy + torch.rand(1, N) * sy).long().clamp(max=W - 1)
        assert torch.equal(got["inds_coarse"], inds_coarse) and got["inds_coarse"].dtype == torch.int64
        assert torch.equal(got["inds"], inds_x * W + inds_y)
        assert got["rays_o"].shape == (1, N, 3) and got["rays_d"].shape == (1, N, 3)
        # every pixel lies in the image area of its cell
        cx, cy = (inds_coarse // 128).numpy(), (inds_coarse % 128).numpy()
        assert ((inds_x.numpy() >= np.floor(cx * sx)) & (inds_x.numpy() <= np.minimum(np.floor((cx + 1) * sx), H - 1))).all()
        assert ((inds_y.numpy() >= np.floor(cy * sy)) & (inds_y.numpy() <= np.minimum(np.floor((cy + 1) * sy), W - 1))).all()


def test_sample_error_map_validates_before_it_needs_a_device():
    from dnerf_amd.utils import sample_error_map
    row = torch.ones(128 * 128)
    bad = [
        dict(error_row=torch.ones(128 * 128, dtype=torch.float64), N=8, H=8, W=8),          # dtype
        dict(error_row=torch.ones(2, 64), N=8, H=8, W=8),                                   # a row, not a map
        dict(error_row=torch.ones(2 * 128 * 128)[::2], N=8, H=8, W=8),                      # strided
        dict(error_row=torch.ones(60), N=8, H=8, W=8),                                      # not a square
        dict(error_row=torch.ones(256 * 256), N=8, H=8, W=8),                               # larger than 128 x 128
        dict(error_row=row, N=0, H=8, W=8),
        dict(error_row=row, N=128 * 128 + 1, H=8, W=8),
        dict(error_row=row, N=8, H=0, W=8),
        dict(error_row=row, N=8, H=65536, W=65536),
        dict(error_row=row, N=8, H=8, W=8, u_key=torch.rand(100)),
        dict(error_row=row, N=8, H=8, W=8, u_fine=torch.rand(8)),
        dict(error_row=row, N=8, H=8, W=8, u_key=torch.rand(128 * 128, dtype=torch.float64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            sample_error_map(**kw)
    if not torch.cuda.is_available():
        from sdn_backend import SdnError
        with pytest.raises(SdnError):                   # valid arguments, no device: an error, not a torch fall-back
            sample_error_map(row, 8, 8, 8)


def test_native_train_step_validates_the_error_map_arguments():
    from dnerf_amd.train_native import NativeTrainStep
    check = NativeTrainStep.check_error_map_args
    n = 16
    emap, cells = torch.ones(4, 64), torch.arange(n, dtype=torch.int32)
    assert check(emap, 2, cells, n, "cpu") == (2, 64)
    assert check(emap, [3], cells.long()[None], n, "cpu") == (3, 64)
    assert check(emap, np.int64(0), cells, n, "cpu") == (0, 64)
    bad = [
        (None, 1, cells), (emap, None, cells), (emap, 1, None),                     # all three or none
        (emap.double(), 1, cells), (emap[0], 1, cells),                             # dtype, rank
        (torch.ones(4, 128)[:, ::2], 1, cells),                                     # strided: would need a copy
        (emap, [0, 1], cells), (emap, [], cells), (emap, 1.0, cells), (emap, True, cells), (emap, 4, cells), (emap, -1, cells),
        (emap, 1, cells.float()), (emap, 1, cells[:-1]), (emap, 1, cells.view(4, 4)), (emap, 1, cells[None, None]),
        (emap, 1, cells.tolist()),
    ]
    for em, idx, ic in bad:
        with pytest.raises(ValueError):
            check(em, idx, ic, n, "cpu")
    with pytest.raises(ValueError, match="device"):                                 # a map the kernels cannot reach is not copied silently
        check(emap, 1, cells, n, "cuda")
    with pytest.raises(ValueError, match="device"):
        check(emap, 1, cells, n, torch.device("cuda", 0))


def test_header_appends_the_three_fields_after_det_scratch():
    text = open(os.path.join(ROOT, "include", "sdn_hip.h")).read()
    body = re.search(r"typedef struct SdnTrainStep \{(.*?)\} SdnTrainStep;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [re.sub(r"\[.*\]", "", part).replace("*", " ").split()[-1] for part in decl.split(",")]
        fields += names
    assert fields[-4:] == ["det_scratch", "error_row", "inds_coarse", "ray_loss_out"], fields[-6:]
    assert re.search(r"float \*error_row;", body) and re.search(r"const int32_t \*inds_coarse;", body) and re.search(r"float \*ray_loss_out;", body)
    import sdn_backend as B
    assert [f[0] for f in B.SdnTrainStep._fields_][-4:] == fields[-4:]
    assert "sdn_error_map_sample" in B.PROTOTYPES and hasattr(B.lib, "sdn_error_map_sample")
