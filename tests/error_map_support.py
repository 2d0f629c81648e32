"""What the error-map tests compare the kernels against, restated in numpy (nerf/utils.py:105-118, dnerf/utils.py:91-113), and the
small inputs they share.

The draw: torch.multinomial(w, N, replacement=False) keeps the N largest w_i / q_i with q_i ~ Exp(1); with q_i = -log(u_i) that is
`restated_draw` -- float64 keys, stable descending order (equal keys: the lower cell first; a zero weight has key zero and comes
after every positive one).  The pixel inside a drawn cell: `fine_pixels`, the reference's expressions in fp32."""
import json
import os

import numpy as np

S_REF = 128                      # the reference's fixed map side
DRAW_SEEDS = (0, 1, 2, 3)
DRAW_NS = (64, 1000, 4096)
DRAW_MAPS = ("ones", "skewed", "mostly_tiny")
IMAGE_SIZES = ((800, 800), (100, 75), (128, 128))      # 100 x 75: sx < 1, the clamp is exercised
BAND_REL, BAND_MAX = 1e-5, 2


def draw_case(kind, seed, N, cells=S_REF * S_REF):
    """(weights, u_key, u_fine) of one seeded case, fp32; u_key clipped into [2^-24, 1 - 2^-24]."""
    rng = np.random.default_rng(seed)
    if kind == "ones":
        w = np.ones(cells, np.float32)
    elif kind == "skewed":
        w = (rng.random(cells) ** 4 + 1e-6).astype(np.float32)
    elif kind == "mostly_tiny":
        w = rng.random(cells).astype(np.float32)
        w[rng.random(cells) < 0.7] = 1e-4
    else:
        raise KeyError(kind)
    u_key = np.clip(rng.random(cells, dtype=np.float32), np.float32(2.0 ** -24), np.float32(1 - 2.0 ** -24))
    u_fine = rng.random(2 * N, dtype=np.float32)
    return w, u_key, u_fine


def draw_keys(w, u, dtype=np.float64):
    w, u = np.asarray(w, dtype), np.asarray(u, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0, w / -np.log(u), 0).astype(dtype)


def restated_draw(w, u, N, dtype=np.float64):
    """(the N drawn cells in rank order, every cell's key)."""
    keys = draw_keys(w, u, dtype)
    return np.argsort(-keys, kind="stable")[:N], keys


def threshold_band(keys, N, rel=BAND_REL):
    """Cells whose key lies within `rel` (relative) of the midpoint between the N-th and the (N+1)-th largest key: the only cells an
    fp32 evaluation of the keys may rank on the other side of the cut."""
    if N >= keys.size:
        return np.zeros(0, np.int64)
    ranked = np.sort(keys)[::-1]
    mid = 0.5 * (ranked[N - 1] + ranked[N])
    return np.nonzero(np.abs(keys - mid) <= rel * mid)[0]


def assert_same_draw(got_cells, w, u, N):
    """The device's cell set against the float64 top-N, cells in the threshold band left out (at most BAND_MAX of them)."""
    got_cells = np.asarray(got_cells, np.int64)
    assert got_cells.shape == (N,) and np.unique(got_cells).size == N, "N distinct cells"
    assert got_cells.min() >= 0 and got_cells.max() < np.asarray(w).size
    want, keys = restated_draw(w, u, N)
    band = threshold_band(keys, N)
    assert band.size <= BAND_MAX, band
    differ = np.setxor1d(got_cells, want)
    stray = np.setdiff1d(differ, band)
    assert stray.size == 0, (stray[:8], keys[stray[:8]], np.sort(keys)[::-1][N - 1:N + 1])


def fine_pixels(cells, S, H, W, r0, r1):
    """nerf/utils.py:108-112 in fp32: (inds_x * sx + rand * sx).long().clamp(max=H - 1), the same for y, inds = x * W + y."""
    c = np.asarray(cells, np.int64)
    sx, sy = np.float32(H) / np.float32(S), np.float32(W) / np.float32(S)
    x = ((c // S).astype(np.float32) * sx + np.asarray(r0, np.float32) * sx).astype(np.int64)
    y = ((c % S).astype(np.float32) * sy + np.asarray(r1, np.float32) * sy).astype(np.int64)
    return np.minimum(x, H - 1) * W + np.minimum(y, W - 1)


def ema(old, loss):
    """dnerf/utils.py:109-110 in fp32."""
    return np.float32(0.1) * np.asarray(old, np.float32) + np.float32(0.9) * np.asarray(loss, np.float32)


def train_scene(fp32=False, n_rays=1024):
    """The small training scene of tests/test_gpu_train_native.py / _f32.py (`_setup` there): the 32 x 32 camera of the bench scene,
    a fresh network with its weights, Adam, a GradScaler (disabled for the fp32 step), a random target, the sample budget taken from
    one op-by-op render.  Returns (scene, model, optimizer, scaler, target [n_rays, 3])."""
    import torch
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network import NeRFNetwork
    sc = build_scene(H=32, W=32, device="cuda", seed=0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    opt = torch.optim.Adam(model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", enabled=not fp32)
    target = torch.rand(n_rays, 3, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=not fp32):
        model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1, force_all_rays=False)
    model.mean_count = int(model.step_counter[0, 0].item()) + 256
    model.local_step = 0
    model.step_counter.zero_()
    return sc, model, opt, scaler, target


def write_blender_dataset(root, n=4, side=8):
    """A synthetic D-NeRF (blender) dataset of n training frames of side x side RGBA noise, cameras on a circle looking at the origin."""
    from PIL import Image
    from dnerf_amd.scene import look_at_pose
    rng = np.random.default_rng(0)
    for split, count in (("train", n), ("val", 1), ("test", 1)):
        frames = []
        os.makedirs(os.path.join(root, split), exist_ok=True)
        for k in range(count):
            img = rng.integers(0, 256, (side, side, 4), dtype=np.uint8)
            Image.fromarray(img, "RGBA").save(os.path.join(root, split, f"r_{k:03d}.png"))
            frames.append({"file_path": f"./{split}/r_{k:03d}", "time": k / max(count - 1, 1),
                           "transform_matrix": np.asarray(look_at_pose(40.0 * k, 20.0, 3.0), np.float32).tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911, "frames": frames}, f)
