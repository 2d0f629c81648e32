"""Several jittered samples of one view in one loop, the part that needs no GPU: the new symbol, the argument checks of
`DeviceLoop.render_samples` and the fold count / spp bookkeeping of `PreviewRenderer.accumulate_group` (native call stubbed)."""
import ctypes
import os
import re

import pytest
import torch

import preview_group_support as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_finish_symbol_is_exported_and_declared():
    import sdn_backend as B
    assert "sdn_preview_finish_group" in B.PROTOTYPES and hasattr(B.lib, "sdn_preview_finish_group")
    assert len(B.PROTOTYPES["sdn_preview_finish_group"]) == 16
    assert B.PROTOTYPES["sdn_preview_finish_group"][:14] == B.PROTOTYPES["sdn_preview_finish"][:14]      # + n_fold, stream
    with open(os.path.join(ROOT, "include", "sdn_hip.h")) as f:
        header = f.read()
    decl = re.search(r"int sdn_preview_finish_group\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == 16 and "uint32_t n_fold" in decl.group(1)


def test_group_finish_refuses_before_any_launch():
    import sdn_backend as B
    c = B.SdnRenderCtx()
    for name in ("image", "weights_sum", "depth", "nears", "fars", "rays_o", "rays_d"):
        setattr(c, name, 0x1000)                       # never dereferenced: every call below is refused first
    c.N, c.n_group_frames, c.rays_per_frame = 4 * 35, 4, 35
    bg = (ctypes.c_float * 3)(1, 1, 1)
    out = 0x2000
    call = lambda *a: B.lib.sdn_preview_finish_group(*a)  # noqa: E731
    assert call(ctypes.byref(c), 5, 7, 5, 7, bg, None, 1, 0, out, out, None, out, 0, 5, None) == -1       # n_fold > n_group_frames
    assert call(ctypes.byref(c), 5, 7, 5, 7, bg, None, 1, 0, out, out, None, out, 0, 0, None) == -1       # nothing to fold
    assert call(ctypes.byref(c), 5, 7, 5, 7, bg, None, 1, 0, out, out, None, None, 0, 4, None) == -1      # no buffer to fold into
    assert call(ctypes.byref(c), 5, 7, 5, 7, bg, None, 1, 0, out, out, None, out, -1, 4, None) == -1      # spp < 0
    assert call(ctypes.byref(c), 5, 6, 5, 6, bg, None, 1, 0, out, out, None, out, 0, 4, None) == -1       # rH * rW != rays_per_frame
    assert call(ctypes.byref(c), 5, 7, 9, 9, bg, None, 1, 0, out, out, out, out, 0, 4, None) == -1        # pos_out with rH != H
    assert call(None, 5, 7, 5, 7, bg, None, 1, 0, out, out, None, out, 0, 4, None) == -1
    c.n_group_frames = c.rays_per_frame = 0
    c.N = 35
    assert call(ctypes.byref(c), 5, 7, 5, 7, bg, None, 1, 0, out, out, None, out, 0, 1, None) == -1       # not a group context


def _stub_loop(frames, N):
    from dnerf_amd.renderer import DeviceLoop
    loop = object.__new__(DeviceLoop)
    loop.frames, loop.N = frames, N
    return loop


def test_render_samples_argument_checks():
    ro = torch.zeros(35, 3)
    z = torch.zeros(4, 35)
    with pytest.raises(ValueError, match="frames = F >= 2"):
        _stub_loop(1, 35).render_samples(ro, ro, 0.5, z[:1])                    # a one-frame loop
    loop = _stub_loop(4, 4 * 35)
    for bad in (torch.zeros(4 * 35), torch.zeros(3, 35), torch.zeros(4, 36), torch.zeros(35, 4), z.double(), z.half(), None, z.numpy()):
        with pytest.raises(ValueError, match="noises must be"):
            loop.render_samples(ro, ro, 0.5, bad)
    with pytest.raises(ValueError, match="samples of 35 rays"):
        loop.render_samples(torch.zeros(4 * 35, 3), torch.zeros(4 * 35, 3), 0.5, z)       # the group's rays instead of the view's
    with pytest.raises(ValueError, match="one time stamp"):
        loop.render_samples(ro, ro, [0.5] * 4, z)
    # the one-frame entry keeps refusing a group (pinned by tests/test_preview_cpu.py as well)
    with pytest.raises(NotImplementedError):
        loop.render(None, None, 0.5, noises=z)


def _stubbed_renderer(monkeypatch, H=5, W=7):
    import sdn_backend as B
    from dnerf_amd.preview import PreviewRenderer
    pv = PreviewRenderer(None, None, W, H, "cpu")
    loop = GS.FakeGroupLoop(B.SdnRenderCtx())
    folds = []
    pv._view_rays = lambda pose, intr, down, pos: (H, W, torch.zeros(H * W, 3), torch.zeros(H * W, 3))
    pv.group_loop_for = lambda n, samples: loop
    monkeypatch.setattr(B, "ptr", lambda t, *a: None if t is None else t.data_ptr())
    monkeypatch.setattr(B, "stream", lambda: None)
    monkeypatch.setattr(B.lib, "sdn_preview_finish_group", lambda *a: folds.append((a[13], a[14])) or 0)
    return pv, loop, folds


def test_accumulate_group_fold_count_and_spp(monkeypatch):
    """max_spp no multiple of samples: the last group renders `samples` frames and folds the rest; full, nothing is rendered."""
    pv, loop, folds = _stubbed_renderer(monkeypatch)
    for _ in range(4):
        assert pv.accumulate_group(None, None, 0.5, max_spp=6, samples=4) is pv.render_buffer
    assert folds == [(0, 4), (4, 2)] and pv.spp == 6                       # (spp before the launch, n_fold)
    assert [c[0] for c in loop.calls] == [(4, 35), (4, 35)]                # both groups rendered all 4 samples
    assert all(c[1] == dict(want_stats=False, finish=False) for c in loop.calls)
    del folds[:]
    pv.accumulate_group(None, None, 0.5, need_update=True, max_spp=7, samples=3)
    for _ in range(3):
        pv.accumulate_group(None, None, 0.5, max_spp=7, samples=3)
    assert folds == [(0, 3), (3, 3), (6, 1)] and pv.spp == 7
    del folds[:]
    pv.accumulate_group(None, None, 0.5, need_update=True, max_spp=2, samples=8)      # fewer wanted than one group holds
    assert folds == [(0, 2)] and pv.spp == 2
    # mixed with the one-frame path's count: accumulate_group continues where `accumulate` stopped
    pv.spp = 5
    del folds[:]
    pv.accumulate_group(None, None, 0.5, samples=2)
    assert folds == [(5, 2)] and pv.spp == 7
    for bad in (1, 0, 17):
        with pytest.raises(ValueError, match="samples must be"):
            pv.accumulate_group(None, None, 0.5, samples=bad)


def test_preview_renderer_keeps_one_frame_per_loop_and_its_own_group_cache():
    from dnerf_amd.preview import PreviewRenderer
    with pytest.raises(NotImplementedError):
        PreviewRenderer(None, None, 7, 5, "cpu", frames=2)
    pv = PreviewRenderer(None, None, 7, 5, "cpu")
    assert pv.loops == {} and pv.group_loops == {}

    class Loop:
        def __init__(self, refuse):
            self.refuse, self.mapper = refuse, None

        def set_mapper(self, m):
            if self.refuse and m == "anchor":
                raise NotImplementedError
            self.mapper = m
    pv.loops[35] = Loop(False)
    pv.group_loops[(35, 4)] = Loop(True)
    pv.set_mapper("bbox")
    assert pv.loops[35].mapper == "bbox" and pv.group_loops[(35, 4)].mapper == "bbox"
    pv.set_mapper("anchor")                                # the one-frame loop takes it; the group loop is dropped and rebuilt (and refused) on demand
    assert pv.loops[35].mapper == "anchor" and pv.group_loops == {}
