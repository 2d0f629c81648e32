"""Error-map ray sampling and the map's update on the device: `sdn_error_map_sample` (csrc/error_map.hip) against the numpy restatement
of torch.multinomial's rule (tests/error_map_support.py), the update inside the native training steps' compositing launch (csrc/train.hip)
against the reference's expressions (dnerf/utils.py:85, :109-110), and the round trip through the dataset provider."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import error_map_support as E

pytestmark = pytest.mark.gpu

S = E.S_REF
CELLS = S * S


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _draw(w, N, H, W, u_key=None, u_fine=None, seed=None):
    from dnerf_amd.utils import sample_error_map
    ic, fi = sample_error_map(_dev(w) if isinstance(w, np.ndarray) else w, N, H, W, None if u_key is None else _dev(u_key),
                              None if u_fine is None else _dev(u_fine), seed)
    assert ic.dtype == torch.int32 and fi.dtype == torch.int32 and ic.shape == (N,) and fi.shape == (N,) and ic.is_cuda
    return ic.cpu().numpy(), fi.cpu().numpy()


# ---- the draw against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.DRAW_NS)
@pytest.mark.parametrize("kind", E.DRAW_MAPS)
def test_draw_is_the_float64_top_n_and_the_pixels_follow_the_formula(kind, N):
    """Replayed uniforms, S = 128, four seeds: the drawn cells are the float64 top-N (cells within 1e-5 relative of the midpoint between
    the N-th and (N+1)-th key excused, at most 2 per case), N distinct cells, and `inds` is the fp32 pixel formula exactly for three
    image sizes."""
    for seed in E.DRAW_SEEDS:
        w, u_key, u_fine = E.draw_case(kind, seed, N)
        for H, W in E.IMAGE_SIZES:
            cells, pix = _draw(w, N, H, W, u_key, u_fine)
            E.assert_same_draw(cells, w, u_key, N)
            assert np.array_equal(pix, E.fine_pixels(cells, S, H, W, u_fine[:N], u_fine[N:])), (kind, N, seed, H, W)
            assert pix.min() >= 0 and pix.max() < H * W


# ---- edge cases of the draw ------------------------------------------------------------------------------------------------------------
def test_draw_of_every_cell_and_of_one_cell():
    w, u_key, u_fine = E.draw_case("skewed", 0, CELLS)
    cells, pix = _draw(w, CELLS, 800, 800, u_key, u_fine)
    assert np.array_equal(np.sort(cells), np.arange(CELLS))
    assert np.array_equal(pix, E.fine_pixels(cells, S, 800, 800, u_fine[:CELLS], u_fine[CELLS:]))
    cells, pix = _draw(w, 1, 800, 800, u_key, u_fine[:2])
    assert cells.tolist() == E.restated_draw(w, u_key, 1)[0].tolist()
    assert pix.tolist() == E.fine_pixels(cells, S, 800, 800, u_fine[:1], u_fine[1:2]).tolist()


def test_draw_from_the_smallest_map():
    """S = 8, N = 5: 64 cells in 4 of the workgroup's 1024 threads, the rest padding."""
    rng = np.random.default_rng(5)
    for _ in range(4):
        w = (rng.random(64) + 0.05).astype(np.float32)
        u_key = np.clip(rng.random(64, dtype=np.float32), 2.0 ** -24, 1 - 2.0 ** -24).astype(np.float32)
        u_fine = rng.random(10, dtype=np.float32)
        cells, pix = _draw(w, 5, 20, 12, u_key, u_fine)
        assert sorted(cells.tolist()) == sorted(E.restated_draw(w, u_key, 5)[0].tolist())
        assert np.array_equal(pix, E.fine_pixels(cells, 8, 20, 12, u_fine[:5], u_fine[5:]))
    cells, _ = _draw(w, 64, 20, 12, u_key, rng.random(128, dtype=np.float32))
    assert np.array_equal(np.sort(cells), np.arange(64))


def test_zero_weights_are_drawn_last_and_ties_go_to_the_lower_cell():
    rng = np.random.default_rng(6)
    N = 1000
    u_key = np.clip(rng.random(CELLS, dtype=np.float32), 2.0 ** -24, 1 - 2.0 ** -24).astype(np.float32)
    u_fine = rng.random(2 * N + 2, dtype=np.float32)
    # exactly N positive cells, some of them tiny: exactly those are drawn
    positive = rng.choice(CELLS, N, replace=False)
    w = np.zeros(CELLS, np.float32)
    w[positive] = rng.random(N).astype(np.float32) + 1e-3
    w[positive[:10]] = 1e-30
    cells, _ = _draw(w, N, 800, 800, u_key, u_fine[:2 * N])
    assert np.array_equal(np.sort(cells), np.sort(positive))
    # one more than the positive cells: the lowest-indexed zero cell joins them
    cells, _ = _draw(w, N + 1, 800, 800, u_key, u_fine)
    first_zero = int(np.nonzero(w == 0)[0][0])
    assert np.array_equal(np.sort(cells), np.sort(np.append(positive, first_zero)))
    # equal weight and equal u on two cells across the threshold: the lower index is kept
    w = np.ones(CELLS, np.float32)
    order, _ = E.restated_draw(w, u_key, CELLS)
    lo, hi = sorted((int(order[N - 1]), int(order[-1])))
    u2 = u_key.copy()
    u2[lo] = u2[hi] = u_key[order[N - 1]]          # the N-th cell and the last one now both carry the N-th key; N - 1 cells lie above it
    cells, _ = _draw(w, N, 800, 800, u2, u_fine[:2 * N])
    assert lo in cells.tolist() and hi not in cells.tolist()
    assert np.array_equal(np.sort(cells), np.sort(E.restated_draw(w, u2, N)[0]))


def test_bad_arguments_are_refused():
    import sdn_backend as B
    row = torch.ones(CELLS, device="cuda")
    a, b = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")

    def rc(error_row=row.data_ptr(), S=128, N=8, H=8, W=8, ic=a.data_ptr(), fi=b.data_ptr()):
        return B.lib.sdn_error_map_sample(error_row, S, N, H, W, None, None, 1, ic, fi, B.stream())
    assert rc() == 0
    for kw in (dict(error_row=None), dict(ic=None), dict(fi=None), dict(S=0), dict(S=129), dict(N=0), dict(N=CELLS + 1), dict(S=2, N=5),
               dict(H=0), dict(W=0), dict(H=65536, W=65536)):
        assert rc(**kw) == -1, kw          # SDN_E_BADARG
    torch.cuda.synchronize()


# ---- the generator path ------------------------------------------------------------------------------------------------------------------
def test_generator_draws_repeat_with_the_seed_and_follow_the_weights():
    """Same seed, same draw; another seed, another draw; and the share of picks that fall on the heavy cells of a map that is 8 where
    cell % 4 == 0 and 1 elsewhere (N = 1024, 32 seeds) lies within 5 standard errors of the restatement's share over as many draws with
    numpy's uniforms.  Standard error: that of the difference of two binomial shares over 32 * 1024 picks each -- an upper bound, since
    picks without replacement vary less."""
    w = np.where(np.arange(CELLS) % 4 == 0, 8.0, 1.0).astype(np.float32)
    wd = _dev(w)
    N, seeds = 1024, 32
    a = _draw(wd, N, 800, 800, seed=11)
    b = _draw(wd, N, 800, 800, seed=11)
    c = _draw(wd, N, 800, 800, seed=12)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    for cells, pix in (a, c):                         # pixels lie inside their cells' 6.25-pixel squares
        assert np.unique(cells).size == N
        x, y = pix // 800, pix % 800
        assert ((x >= np.floor((cells // S) * 6.25)) & (x <= np.floor((cells // S + 1) * 6.25))).all()
        assert ((y >= np.floor((cells % S) * 6.25)) & (y <= np.floor((cells % S + 1) * 6.25))).all()
    heavy_dev = heavy_np = 0
    rng = np.random.default_rng(0)
    for seed in range(seeds):
        cells, _ = _draw(wd, N, 800, 800, seed=1000 + seed)
        assert np.unique(cells).size == N
        heavy_dev += int((cells % 4 == 0).sum())
        want, _ = E.restated_draw(w, np.clip(rng.random(CELLS), 2.0 ** -53, 1 - 2.0 ** -53), N)
        heavy_np += int((want % 4 == 0).sum())
    n = N * seeds
    p_dev, p_np = heavy_dev / n, heavy_np / n
    se = np.sqrt(2 * p_np * (1 - p_np) / n)
    print(f"heavy share: device {p_dev:.4f}, restatement {p_np:.4f}, standard error {se:.4f}")
    assert 0.3 < p_np < 0.95                          # (unweighted picks would give 0.25)
    assert abs(p_dev - p_np) <= 5 * se, (p_dev, p_np, se)


# ---- the update inside the training step -------------------------------------------------------------------------------------------------
N_RAYS = 1024
FRAMES, FRAME = 3, 1


def _map(seed=0):
    return (torch.rand(FRAMES, CELLS, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.01).cuda()


def _cells(emap, seed):
    from dnerf_amd.utils import sample_error_map
    cells, _ = sample_error_map(emap[FRAME], N_RAYS, 32, 32, seed=seed)
    host = cells.cpu().numpy()
    assert host.min() >= 0 and host.max() < CELLS and np.unique(host).size == N_RAYS       # the step's precondition
    return cells


def _assert_row_updated(new_row, old_row, cells, ray_loss):
    """new == 0.1 * old + 0.9 * loss at the drawn cells to 1 ulp of fp32; bit-identical to old everywhere else."""
    new_row, old_row, cells = new_row.cpu().numpy(), old_row.cpu().numpy(), cells.reshape(-1).cpu().numpy().astype(np.int64)
    want = E.ema(old_row[cells], ray_loss.cpu().numpy())
    assert (np.abs(new_row[cells] - want) <= np.spacing(np.abs(want))).all(), float(np.abs(new_row[cells] - want).max())
    rest = np.ones(new_row.size, bool)
    rest[cells] = False
    assert np.array_equal(new_row[rest].view(np.uint32), old_row[rest].view(np.uint32))


@pytest.mark.parametrize("fp32", [False, True], ids=["f16", "f32"])
def test_step_updates_the_map_and_nothing_else(fp32):
    """One deterministic native step with the three arguments and one without, from the same state: `ray_loss` is torch's
    ((image_out - target)^2).mean(-1) and its mean the step's loss (1e-6 relative), row `index` of the map is the EMA at the drawn
    cells (1 ulp) and untouched elsewhere, the other rows are untouched, and every parameter ends bit-identical in both runs.  The
    batch has rays longer than one 64-sample chunk and rays without a sample."""
    from dnerf_amd.train_native import NativeTrainStep
    emap = _map()
    old = emap.clone()
    cells = _cells(emap, seed=7)
    sc, model, opt, scaler, target = E.train_scene(fp32)
    step = NativeTrainStep(model, opt, scaler, N_RAYS, "cuda", perturb=False, deterministic=True)
    version = emap._version
    loss = step(sc.rays_o, sc.rays_d, target, sc.time, error_map=emap, index=[FRAME], inds_coarse=cells)
    torch.cuda.synchronize()
    counts = step.view("rays", torch.int32, (N_RAYS, 3))[:, 2]
    assert int(counts.max()) > 64 and int((counts == 0).sum()) > 0, (int(counts.max()), int((counts == 0).sum()))
    assert emap._version > version and step.ray_loss.shape == (N_RAYS,)
    want = ((step.image - target) ** 2).mean(-1)
    np.testing.assert_allclose(step.ray_loss.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(float(step.ray_loss.double().mean()), float(loss), rtol=1e-6)
    _assert_row_updated(emap[FRAME], old[FRAME], cells, step.ray_loss)
    for f in range(FRAMES):
        if f != FRAME:
            assert torch.equal(emap[f].view(torch.int32), old[f].view(torch.int32))
    # the same step without the update
    sc2, model2, opt2, scaler2, target2 = E.train_scene(fp32)
    step2 = NativeTrainStep(model2, opt2, scaler2, N_RAYS, "cuda", perturb=False, deterministic=True)
    loss2 = step2(sc2.rays_o, sc2.rays_d, target2, sc2.time)
    torch.cuda.synchronize()
    assert float(loss2) == float(loss)
    for (k, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), k
    assert float((model.sigma_net[0].weight.detach() - sc.model.sigma_net[0].weight.detach()).abs().max()) > 0       # (the step did train)


def test_forward_only_call_updates_and_optimizer_only_call_does_not():
    """mode 1 (forward + backward) folds the losses in; the optimizer-only call that follows (mode 2, the record still naming the map)
    leaves it bit-identical.  int64 [1, N] cells give the same map as int32 [N]."""
    import sdn_backend as B
    from dnerf_amd.train_native import NativeTrainStep
    emap = _map(1)
    old = emap.clone()
    cells = _cells(emap, seed=8)
    sc, model, opt, scaler, target = E.train_scene(False)
    step = NativeTrainStep(model, opt, scaler, N_RAYS, "cuda", perturb=False)
    step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True, error_map=emap, index=FRAME, inds_coarse=cells)
    torch.cuda.synchronize()
    _assert_row_updated(emap[FRAME], old[FRAME], cells, step.ray_loss)
    after = emap.clone()
    rec = step._rec
    assert rec.error_row == emap.data_ptr() + FRAME * CELLS * 4
    rec.mode = 2
    B.check(B.lib.sdn_train_step_f16(ctypes.byref(rec), B.stream()), "train_step_f16 (optimizer only)")
    torch.cuda.synchronize()
    assert torch.equal(emap.view(torch.int32), after.view(torch.int32))
    assert float(step.adam_steps[0]) == 1.0                                  # (the optimizer pass did run)
    # the parameters moved, so compare the two index types on forward-only calls from here
    step.refresh()
    m32, m64 = old.clone(), old.clone()
    step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True, error_map=m32, index=FRAME, inds_coarse=cells)
    held = step._inds32.data_ptr()
    step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True, error_map=m64, index=[FRAME], inds_coarse=cells.long()[None])
    torch.cuda.synchronize()
    assert step._inds32.data_ptr() == held                                   # (the step's own buffer, not a new one)
    assert torch.equal(m32.view(torch.int32), m64.view(torch.int32)) and not torch.equal(m32[FRAME], old[FRAME])
    # a call without the arguments after one with them updates nothing
    keep = m64.clone()
    step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True)
    torch.cuda.synchronize()
    assert torch.equal(m64, keep)


def test_two_steps_on_one_frame_apply_the_ema_twice_where_the_draws_overlap():
    from dnerf_amd.train_native import NativeTrainStep
    emap = _map(2)
    sc, model, opt, scaler, target = E.train_scene(False)
    step = NativeTrainStep(model, opt, scaler, N_RAYS, "cuda", perturb=False)
    want = emap[FRAME].cpu().numpy().copy()
    drawn = []
    for it in range(2):
        cells = _cells(emap, seed=20 + it)                    # a fresh draw from the map as it stands
        before = emap[FRAME].clone()
        step(sc.rays_o, sc.rays_d, target, sc.time, error_map=emap, index=FRAME, inds_coarse=cells)
        torch.cuda.synchronize()
        _assert_row_updated(emap[FRAME], before, cells, step.ray_loss)
        c = cells.cpu().numpy()
        want[c] = E.ema(want[c], step.ray_loss.cpu().numpy())
        drawn.append(c)
    both = np.intersect1d(drawn[0], drawn[1])
    assert both.size > 0                                      # (1024 of 16 384 cells twice: ~64 expected)
    got = emap[FRAME].cpu().numpy()
    assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want))).all()
    once = np.setdiff1d(np.union1d(drawn[0], drawn[1]), both)
    assert (np.abs(got[once] - want[once]) <= np.spacing(np.abs(want[once]))).all()


# ---- through the provider ----------------------------------------------------------------------------------------------------------------
def test_provider_round_trip(tmp_path):
    """A 4-frame synthetic dataset with `error_map` and `native_error_map`, preloaded: `collate` hands over int32 cells consistent with the
    pixels it gathered, and three native steps driven from its batches change exactly the drawn cells of the drawn frames."""
    from dnerf_amd.provider import NeRFDataset
    from dnerf_amd.train_native import NativeTrainStep
    E.write_blender_dataset(str(tmp_path), n=4, side=8)
    opt_ns = SimpleNamespace(path=str(tmp_path), preload=True, scale=0.33, offset=[0, 0, 0], bound=1, fp16=False, num_rays=50, rand_pose=-1,
                             error_map=True, native_error_map=True, color_space="srgb")
    ds = NeRFDataset(opt_ns, "cuda", type="train")
    assert ds.error_map.is_cuda and ds.error_map.shape == (4, CELLS)
    n = 50
    sc, model, opt, scaler, _ = E.train_scene(False)
    step = NativeTrainStep(model, opt, scaler, n, "cuda", perturb=False)
    expect_changed = torch.zeros(4, CELLS, dtype=torch.bool, device="cuda")
    torch.manual_seed(0)
    for frame in (2, 0, 2):
        batch = ds.collate([frame])
        cells = batch["inds_coarse"]
        assert cells.dtype == torch.int32 and cells.shape == (1, n) and batch["index"] == [frame]
        assert batch["rays_o"].shape == (1, n, 3) and batch["images"].shape == (1, n, 4)
        c = cells[0].cpu().numpy().astype(np.int64)
        assert np.unique(c).size == n and c.min() >= 0 and c.max() < CELLS
        # the gathered colours are those of pixels inside the drawn cells: 8 x 8 pixels under 128 x 128 cells, pixel = cell // 16 per axis
        pix = (c // S // 16) * 8 + (c % S) // 16
        assert torch.equal(batch["images"][0], ds.images[frame].view(64, 4)[torch.from_numpy(pix).cuda()])
        rgba = batch["images"][0]
        target = (rgba[:, :3] * rgba[:, 3:] + (1 - rgba[:, 3:])).contiguous()
        step(batch["rays_o"][0].contiguous(), batch["rays_d"][0].contiguous(), target, batch["time"], error_map=ds.error_map,
             index=batch["index"], inds_coarse=cells)
        expect_changed[frame, torch.from_numpy(c).cuda()] = True
    torch.cuda.synchronize()
    assert torch.equal(ds.error_map != 1, expect_changed)
