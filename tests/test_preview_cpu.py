"""Preview frames, the part that needs no GPU: tests/golden/caller_preview.npz -- the reference's own `run_cuda(perturb=True)`,
`F.interpolate(mode='nearest')` and `linear_to_srgb`, recorded by tests/golden/gen_preview_fixture.py -- against the restatements the
GPU tests compare the kernels with (tests/preview_support.py), and the argument checks that refuse before any launch."""
import ctypes

import numpy as np
import pytest

import preview_support as PS
from caller_fixtures import fixture_model, fixture_scene


@pytest.fixture(scope="module")
def fx():
    return PS.load()


def test_fixture_noises_are_the_seeded_draw_with_both_ends_pinned(fx):
    z = fx["noises"]
    assert z.dtype == np.float32 and z.shape == (64 * 64,)
    assert np.array_equal(z, PS.draw_noises(64 * 64, PS.FRAME_SEED))
    assert (z == 0).sum() >= 40 and (z == PS.ONE_BELOW).sum() >= 40 and z.min() >= 0 and z.max() < 1


def test_oracle_loop_with_first_march_noises_reproduces_the_reference(fx):
    """oracle/render.py's loop restated with `noises` in iteration 0 against the reference's run_cuda(perturb=True): trace and sample
    count exact, floats within 2e-5 (the bar of the other caller fixtures)."""
    sc = fixture_scene("cpu", model_bits=fixture_model("cpu"))
    out = PS.render_loop_oracle(sc, noises=fx["noises"])
    assert [tuple(r) for r in fx["trace"].tolist()] == [tuple(r) for r in out["trace"]]
    assert out["n_samples"] == int(fx["n_samples"])
    np.testing.assert_allclose(out["weights_sum"], fx["weights_sum"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(out["image"], fx["image"], rtol=0, atol=2e-5)
    miss = np.isnan(fx["depth"])
    assert np.array_equal(miss, np.isnan(out["depth"]))
    np.testing.assert_allclose(out["depth"][~miss], fx["depth"][~miss], rtol=0, atol=2e-5)
    # and the jitter is not a no-op: the unperturbed loop takes other samples
    plain = PS.render_loop_oracle(sc, noises=None)
    assert plain["n_samples"] != out["n_samples"] or np.abs(plain["image"] - out["image"]).max() > 1e-4


def test_nearest_rule_is_torchs(fx):
    rH, rW, H, W = PS.NEAREST_CASE
    assert np.array_equal(PS.source_index(rH, rW, H, W), fx["nearest_index"])
    assert np.array_equal(PS.source_index(5, 7, 5, 7), np.arange(35).reshape(5, 7))       # identity
    assert np.array_equal(PS.source_index(1, 1, 1, 1), np.zeros((1, 1), np.int64))


def test_srgb_restatement_rounds_to_the_references_fp32(fx):
    """float64 restatement rounded to fp32 against torch's fp32 `linear_to_srgb`: the linear branch exactly, the power branch within
    4e-7 relative on the pow term (torch's fp32 pow is not correctly rounded); the ramp has values on both sides of 0.0031308."""
    x, want = fx["srgb_in"], fx["srgb_out"]
    assert (x < np.float32(PS.SRGB_EDGE)).sum() >= 10 and (x >= np.float32(PS.SRGB_EDGE)).sum() >= 10
    got = PS.linear_to_srgb64(x)
    lin = x < np.float32(PS.SRGB_EDGE)
    assert np.array_equal(np.float32(12.92) * x[lin], want[lin])                   # one fp32 multiplication, as the kernel does it
    assert np.abs(got[lin].astype(np.float32) - want[lin]).max() <= 1e-8
    pow_want = (want[~lin].astype(np.float64) + 0.055) / 1.055
    pow_got = (got[~lin] + 0.055) / 1.055
    assert np.abs(pow_want / pow_got - 1).max() <= 4e-7
    assert np.abs(got.astype(np.float32) - want).max() <= 1e-6


def test_finishing_pass_restatement_running_mean_and_nan_to_num():
    """The numpy restatement on a tiny frame with NaN / inf depths, against the expressions of test_gui / gui.py written out."""
    rng = np.random.default_rng(5)
    n = 6
    acc = dict(image=rng.random((n, 3), dtype=np.float32) * 0.5, weights_sum=rng.random(n, dtype=np.float32),
               depth=np.array([0.5, np.nan, np.inf, -np.inf, 2.0, 0.1], np.float32), nears=np.full(n, 0.2, np.float32),
               fars=np.full(n, 1.7, np.float32), rays_o=rng.random((n, 3), dtype=np.float32), rays_d=rng.random((n, 3), dtype=np.float32))
    r = PS.finish_numpy(acc, 2, 3, 2, 3, normalize=False, pos=True, accum=np.full((2, 3, 3), np.nan, np.float32), spp=0)
    fmax = np.finfo(np.float32).max
    assert np.array_equal(r["depth"].reshape(-1), np.array([0.5, 0.0, fmax, -fmax, 2.0, 0.1], np.float32))
    assert np.array_equal(r["accum"], r["image"])                                 # spp == 0 overwrites, whatever the buffer held
    assert np.array_equal(r["pos"].reshape(-1, 3)[0], (acc["rays_o"][0] + np.float32(0.5) * acc["rays_d"][0]).astype(np.float32))
    r2 = PS.finish_numpy(acc, 2, 3, 2, 3, normalize=True, accum=r["accum"], spp=3)
    want = ((r["accum"] * np.float32(3)).astype(np.float32) + r2["image"]) / np.float32(4)
    assert np.array_equal(r2["accum"], want.astype(np.float32))
    d = r2["depth"].reshape(-1)
    assert d[0] == np.float32(np.float32(0.5 - np.float32(0.2)) / np.float32(np.float32(1.7) - np.float32(0.2)))
    assert d[1] == 0 and d[2] == fmax and d[3] == 0 and d[5] == 0               # NaN -> 0 (fmaxf drops it), +inf, clamp(-inf), clamp(< near)


# ----------------------------------------------------------------------------------------------------------------------
# refusals, before any launch (no device here: a launch would fail differently)
# ----------------------------------------------------------------------------------------------------------------------
def _fake_ctx(B, n):
    c = B.SdnRenderCtx()
    for name in ("rays_o", "rays_d", "nears", "fars", "bitfield", "cull_bits", "alive_a", "alive_b", "rays_t", "weights_sum", "depth",
                 "image", "state", "live_counts"):
        setattr(c, name, 0x1000)                       # never dereferenced: every call below is refused first
    c.N = n
    return c


def test_preview_finish_refuses_bad_arguments():
    import sdn_backend as B
    c = _fake_ctx(B, 18 * 26)
    bg = (ctypes.c_float * 3)(1, 1, 1)
    out = 0x2000
    call = lambda *a: B.lib.sdn_preview_finish(*a)  # noqa: E731
    assert call(ctypes.byref(c), 18, 26, 37, 53, bg, None, 1, 0, out, out, out, None, 0, None) == -1      # pos_out with rH != H
    assert call(ctypes.byref(c), 18, 26, 37, 53, bg, None, 1, 0, None, out, None, None, 0, None) == -1    # NULL image_out
    assert call(ctypes.byref(c), 18, 26, 37, 53, bg, None, 1, 0, out, None, None, None, 0, None) == -1    # NULL depth_out
    assert call(None, 18, 26, 37, 53, bg, None, 1, 0, out, out, None, None, 0, None) == -1
    assert call(ctypes.byref(c), 18, 25, 37, 53, bg, None, 1, 0, out, out, None, None, 0, None) == -1     # rH * rW != N
    assert call(ctypes.byref(c), 18, 26, 0, 53, bg, None, 1, 0, out, out, None, None, 0, None) == -1
    assert call(ctypes.byref(c), 18, 26, 37, 53, None, None, 1, 0, out, out, None, None, 0, None) == -1   # no background at all
    assert call(ctypes.byref(c), 18, 26, 37, 53, bg, None, 1, 0, out, out, None, out, -1, None) == -1     # accum with spp < 0
    with pytest.raises(B.SdnError):
        B.check(-1, "preview_finish")


def test_native_drivers_refuse_noises_outside_one_frame_per_loop():
    import sdn_backend as B
    c = _fake_ctx(B, 64)
    c.noises = 0x3000
    c.n_group_frames, c.rays_per_frame, c.slot_frame = 2, 32, 0x1000
    c.frame_bitfield[0] = c.frame_bitfield[1] = 0x1000
    assert B.lib.sdn_render_begin(ctypes.byref(c), None) == -2                    # frame group
    c.n_group_frames = c.rays_per_frame = 0
    c.aabb = 0x1000
    ctxs = (ctypes.POINTER(B.SdnRenderCtx) * 1)(ctypes.pointer(c))
    one = (ctypes.c_void_p * 1)(0x1000)
    four = (ctypes.c_void_p * 4)(*([0x1000] * 4))
    snap = (ctypes.c_int32 * 8)()
    rc = B.lib.sdn_render_frames_pipelined_f16(ctxs, 1, 1, one, one, one, one, 1.0, 1, one, one, four, four, snap, None, 0, None, None, None, None)
    assert rc == -2                                                               # pipelined frames


def test_python_loops_refuse_noises_where_they_are_not_built():
    import torch
    from dnerf_amd.renderer import DeviceLoop, PipelinedDeviceLoop, RayBatchRenderer
    z = torch.zeros(8)
    group = object.__new__(DeviceLoop)
    group.frames = 2
    for kw in (dict(noises=z), dict(perturb=True)):
        with pytest.raises(NotImplementedError):
            group.render(None, None, 0.5, **kw)
        with pytest.raises(NotImplementedError):
            object.__new__(PipelinedDeviceLoop).render_frames([None], [None], 0.5, **kw)
        with pytest.raises(NotImplementedError):
            object.__new__(RayBatchRenderer).render(None, None, 0.5, **kw)


def test_preview_symbol_is_exported_and_declared_and_the_record_carries_noises():
    import sdn_backend as B
    assert "sdn_preview_finish" in B.PROTOTYPES and hasattr(B.lib, "sdn_preview_finish")
    assert len(B.PROTOTYPES["sdn_preview_finish"]) == 15
    names = [f for f, _ in B.SdnRenderCtx._fields_]
    assert "noises" in names and B.SdnRenderCtx.noises.size == ctypes.sizeof(ctypes.c_void_p)
