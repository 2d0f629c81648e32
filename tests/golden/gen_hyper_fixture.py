#!/usr/bin/env python3
"""Generates tests/golden/caller_hyper.npz by EXECUTING THE REFERENCE'S OWN ambient-dimension model -- dnerf/network_hyper.py
`NeRFNetwork` (what `main_dnerf.py --hyper` selects) under dnerf/renderer.py `run_cuda` -- imported from the reference checkout, never
copied, over the oracle-backed operator shims of tests/ref_shims/, the way gen_basis_fixture.py makes the temporal-basis fixture.

Model: the reference's class constructed under torch.manual_seed(G.SEED) with the bench scene's recipe (tests/hyper_support.py states
it once for both sides): embeddings x 1e3, the bench scene's occupancy bits, the last ambient layer scaled by ONE float32 factor so
that the ambient coordinate moves across grid cells between the three times (the seeded ambient_net moves it by a few 1e-3 only),
and row 0 of the last sigma layer -- the density logit -- scaled by ONE float32 factor so that the median of log sigma on the probe
points of slice 32 at time 0.5 is LOG_SIGMA_SHARE of the one gen_caller_fixtures calibrates to (see there why).  Both factors are recorded (scalars; no weights are):
the mirror built from the seed and the factors must reproduce every state-dict digest.

Recorded: the digests, `forward` (sigma, rgb) and `density` (sigma, geo_feat) on 2048 seeded points and the ambient value at each of
the three times, and a 64 x 64 `run_cuda` frame at each time (trace, image, depth, weights_sum).

Run in the build container only:   python tests/golden/gen_hyper_fixture.py
"""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import gen_caller_fixtures as G  # noqa: E402  (installs the stubs and the operator shims)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hyper_support as HS  # noqa: E402

AMBIENT_SPREAD = 2.0     # the pre-tanh ambient values of the three times span this much after scaling
# The seeded colour net's logits are of the order 1e-3: every sample's rgb is 0.5 whatever the time, and a frame depends on the time
# stamp through opacity alone.  Calibrated to the other fixtures' median (sigma dt = MEDIAN_SIGMA_DT) every ray that enters the
# occupancy is opaque at every time and only the silhouette's ~80 pixels move; with the median of log sigma at a quarter of that log
# (median sigma about 2 instead of 15) the object is semi-transparent and its pixels follow the density of their time.
LOG_SIGMA_SHARE = 0.25


def ambient_raw(model, t):
    """ambient_net(encoder_time(t)) before the tanh, from the reference's own layers (network_hyper.py:127-134 restated as calls)."""
    h = model.encoder_time(torch.tensor([[t]], dtype=torch.float32))
    for l in range(model.num_layers_ambient):
        h = model.ambient_net[l](h)
        if l != model.num_layers_ambient - 1:
            h = torch.relu(h)
    return h


def build_reference_model():
    import dnerf.network_hyper as ref_hyper
    torch.manual_seed(G.SEED)
    model = ref_hyper.NeRFNetwork(**HS.MODEL_KW)
    model.encoder.embeddings.mul_(1e3)
    model.eval()
    bits = HS.occupancy_bits(model.time_size, model.grid_size, G.scene)
    model.density_bitfield.copy_(torch.from_numpy(bits))
    raw = np.array([float(ambient_raw(model, t)[0, 0]) for t in HS.TIMES])
    ambient_scale = np.float32(AMBIENT_SPREAD / (raw.max() - raw.min()))
    # density calibration on slice 32 at time 0.5 with the reference's own density(): log sigma is linear in row 0
    HS.scale_rows(model, 1.0, ambient_scale)
    pts = torch.from_numpy(G.probe_points(bits[32][: model.grid_size ** 3 // 8], 8192, G.SEED))
    med = float(torch.log(model.density(pts, torch.tensor([[0.5]]))["sigma"]).median())
    assert med != 0
    sigma_scale = np.float32(LOG_SIGMA_SHARE * math.log(G.MEDIAN_SIGMA_DT / (2 * math.sqrt(3) / 1024)) / med)
    HS.scale_rows(model, sigma_scale, 1.0)
    return model, bits, sigma_scale, ambient_scale


def main():
    model, bits, sigma_scale, ambient_scale = build_reference_model()
    digests = G.state_digests(model)
    out = dict(seed=np.int32(G.SEED), times=np.array(HS.TIMES, np.float32), sigma_scale=sigma_scale, ambient_scale=ambient_scale,
               digest_keys=np.array(sorted(digests)), digest_vals=np.array([digests[k] for k in sorted(digests)]),
               bitfield_sha=np.array([G.sha(bits[HS.slice_of(t, model.time_size)]) for t in HS.TIMES]))
    x, d = HS.seeded_points()
    out["x"], out["d"] = x, d
    ro, rd, _ = G.camera_rays(64, 64)
    geo = HS.Geometry4(1)
    for t in HS.TIMES:
        tt = torch.tensor([[t]], dtype=torch.float32)
        s, c, _ = model(torch.from_numpy(x), torch.from_numpy(d), tt)
        dens = model.density(torch.from_numpy(x), tt)
        out[f"t{t}_sigma"], out[f"t{t}_rgb"] = s.numpy().copy(), c.numpy().copy()
        out[f"t{t}_density_sigma"], out[f"t{t}_density_geo"] = dens["sigma"].numpy().copy(), dens["geo_feat"].numpy().copy()
        out[f"t{t}_ambient"] = (torch.tanh(ambient_raw(model, t)) * model.bound).numpy().copy().reshape(-1)
        r = G.run_infer(model, ro, rd, t)
        for k, v in r.items():
            out[f"t{t}_{k}"] = v
        print(f"[hyper t={t}] ambient {out[f't{t}_ambient']}, iterations {len(r['trace'])}, first rows {r['trace'][:3].tolist()}, "
              f"image mean {r['image'].mean():.6f}, median log sigma {float(np.median(np.log(out[f't{t}_sigma']))):.3f}")
        assert len(r["trace"]) >= 4, "the frame must take at least 4 loop iterations"
    a, b = out[f"t{HS.TIMES[0]}_image"], out[f"t{HS.TIMES[-1]}_image"]
    moved = int((np.abs(a - b).max(1) > 1e-2).sum())
    print(f"pixels that differ by more than 1e-2 between t = {HS.TIMES[0]} and t = {HS.TIMES[-1]}: {moved}")
    assert moved >= 100, "the frames must depend on the time stamp"
    out["moved_pixels"] = np.int32(moved)
    for l in (0, 4):
        cells = {geo.cell_w(float(out[f"t{t}_ambient"][0]), l) for t in HS.TIMES}
        print(f"level {l}: the ambient coordinates fall in cells {sorted(cells)}")
        assert len(cells) >= 2, f"the three ambient values must fall in at least two cells of level {l}"
    np.savez_compressed(HS.FIXTURE, **out)
    print("wrote", HS.FIXTURE, f"{os.path.getsize(HS.FIXTURE) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
