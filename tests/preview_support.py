"""Shared by the preview tests and the fixture generator (tests/golden/gen_preview_fixture.py): the seeded inputs behind
tests/golden/caller_preview.npz, a restatement of oracle/render.py's inference loop with the reference's perturbed first march
(`march_rays(..., perturb if step == 0 else False)`, dnerf/renderer.py:350-353), and a numpy restatement of the preview's finishing
pass (`Trainer.test_gui`, SealDNeRF/utils.py:174-240, plus the GUI's running mean, SealDNeRF/gui.py:241-267)."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_preview.npz")
FRAME_SEED = 77
NEAREST_CASE = (18, 26, 37, 53)          # rH, rW -> H, W
SRGB_EDGE = 0.0031308
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))


def load():
    return np.load(FIXTURE)


def draw_noises(n, seed):
    """[n] fp32 offsets in [0, 1): seeded, with 0 and the largest float below 1 pinned into the first entries and spread further in."""
    z = np.random.default_rng(seed).random(n, dtype=np.float32)
    z[0::97] = 0.0
    z[1::89] = ONE_BELOW
    return z


def srgb_ramp():
    lo = np.linspace(0.0, 2 * SRGB_EDGE, 41, dtype=np.float32)
    edge = np.array([np.nextafter(np.float32(SRGB_EDGE), np.float32(0)), np.float32(SRGB_EDGE), np.nextafter(np.float32(SRGB_EDGE), np.float32(1))],
                    np.float32)
    return np.concatenate([lo, edge, np.linspace(0.01, 1.0, 64, dtype=np.float32)]).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the loop (oracle/render.py:render_frame_oracle, plus `noises` in iteration 0)
# ----------------------------------------------------------------------------------------------------------------------
def render_loop_oracle(sc, noises=None, mode="fp32", T_thresh=1e-2, max_steps=1024, dt_gamma=0.0, bg_color=1.0, mapper=None,
                       normalize_depth=True):
    from oracle import oracle as O
    from oracle.field import FieldOracle
    from oracle.render import state_of
    model = sc.model
    field = FieldOracle(state_of(model), bound=model.bound, density_scale=model.density_scale, mode=mode)
    ro = sc.rays_o.detach().cpu().numpy().reshape(-1, 3)
    rd = sc.rays_d.detach().cpu().numpy().reshape(-1, 3)
    t = float(sc.time.reshape(-1)[0])
    bf = np.ascontiguousarray(sc.bitfield)
    N = ro.shape[0]
    aabb = np.array([-model.bound] * 3 + [model.bound] * 3, np.float32)
    nears, fars = O.near_far_from_aabb(ro, rd, aabb, model.min_near)
    ws, dp, im = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    alive = np.arange(N, dtype=np.int32)
    rays_t = nears.copy()
    step, n_samples, trace = 0, 0, []
    while step < max_steps:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        first = step == 0 and noises is not None        # iteration 0 walks arange(N): noises[n] is ray n's offset
        xyzs, dirs, deltas = O.march_rays(n_alive, n_step, alive, rays_t, ro, rd, float(model.bound), bf, model.cascade, model.grid_size,
                                          nears, fars, align=128, perturb=first, dt_gamma=dt_gamma, max_steps=max_steps,
                                          noises=np.asarray(noises, np.float32) if first else None)
        live = deltas[:, 0] > 0
        n_samples += int(live.sum())
        sig = np.zeros(xyzs.shape[0], np.float32)
        rgb = np.zeros((xyzs.shape[0], 3), np.float32)
        if live.any():
            qx, qd, mapped = xyzs[live], dirs[live], None
            if mapper is not None:
                import torch
                px, pd, mapped = mapper.map_to_origin(torch.from_numpy(qx.copy()), torch.from_numpy(qd.copy()))
                qx, qd, mapped = px.numpy(), pd.numpy(), mapped.numpy()
            s, c, _ = field.forward(qx, qd, t)
            if mapped is not None and mapped.any():
                import torch
                c = c.copy()
                c[mapped] = mapper.map_color(torch.from_numpy(qx[mapped]), torch.from_numpy(qd[mapped]), torch.from_numpy(c[mapped])).numpy()
            sig[live], rgb[live] = s, c
        O.composite_rays(n_alive, n_step, alive, rays_t, sig, rgb, deltas, ws, dp, im, T_thresh)
        trace.append((n_alive, n_step, xyzs.shape[0]))
        alive = alive[alive >= 0]
        step += n_step
    image = im + (1 - ws)[:, None] * np.float32(bg_color)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.clip(dp - nears, 0, None) / (fars - nears) if normalize_depth else dp
    return {"image": image.astype(np.float32), "depth": depth.astype(np.float32), "weights_sum": ws, "trace": trace, "n_samples": n_samples,
            "raw_image": im, "raw_depth": dp, "nears": nears, "fars": fars}


# ----------------------------------------------------------------------------------------------------------------------
# the finishing pass
# ----------------------------------------------------------------------------------------------------------------------
def nearest_index(n_out, n_in):
    """torch's `nearest` rule: src = min(int(floor(dst * scale)), in - 1), scale = in / out in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def source_index(rH, rW, H, W):
    """[H, W] flat index of the source ray of every output pixel."""
    return nearest_index(H, rH)[:, None] * rW + nearest_index(W, rW)[None, :]


def linear_to_srgb64(x):
    """nerf/utils.py:44-45 in float64 on fp32 inputs (the branch is taken on the fp32 value, as torch takes it)."""
    x32 = np.asarray(x, np.float32)
    x64 = x32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x32 < np.float32(SRGB_EDGE), 12.92 * x64, 1.055 * np.power(x64, 0.41666) - 0.055)


def finish_numpy(acc, rH, rW, H, W, bg=(1.0, 1.0, 1.0), bg_rays=None, normalize=True, to_srgb=False, pos=False, accum=None, spp=0):
    """acc: dict of per-ray fp32 arrays image [n,3], weights_sum, depth, nears, fars, rays_o, rays_d (n = rH * rW).  Every fp32 step
    is rounded on its own, in the kernel's order; sRGB is evaluated in float64 (`image64`) AND rounded to fp32 (`image`)."""
    f32 = np.float32
    s = source_index(rH, rW, H, W).reshape(-1)
    w = (f32(1) - acc["weights_sum"][s]).astype(f32)
    b = bg_rays[s].astype(f32) if bg_rays is not None else np.broadcast_to(np.asarray(bg, f32), (s.shape[0], 3))
    rgb = (acc["image"][s] + (w[:, None] * b).astype(f32)).astype(f32)
    out = {"index": s.reshape(H, W), "linear": rgb.reshape(H, W, 3)}
    rgb64 = rgb.astype(np.float64)
    if to_srgb:
        rgb64 = linear_to_srgb64(rgb)
        rgb = rgb64.astype(f32)
    d = acc["depth"][s].astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if normalize:
            near = acc["nears"][s]
            diff = (d - near).astype(f32)
            num = np.where(np.isnan(diff), f32(0), np.maximum(diff, f32(0))).astype(f32)      # fmaxf(NaN, 0) = 0; np.maximum would keep the NaN
            d = (num / (acc["fars"][s] - near).astype(f32)).astype(f32)
        d = np.nan_to_num(d, nan=0.0, posinf=np.finfo(f32).max, neginf=-np.finfo(f32).max).astype(f32)
        out["image"], out["image64"], out["depth"] = rgb.reshape(H, W, 3), rgb64.reshape(H, W, 3), d.reshape(H, W)
        if pos:
            out["pos"] = (acc["rays_o"][s] + (d[:, None] * acc["rays_d"][s]).astype(f32)).astype(f32).reshape(H, W, 3)
        if accum is not None:
            a = rgb if spp == 0 else (((accum.reshape(-1, 3) * f32(spp)).astype(f32) + rgb).astype(f32) / f32(spp + 1)).astype(f32)
            out["accum"] = a.reshape(H, W, 3)
    return out
