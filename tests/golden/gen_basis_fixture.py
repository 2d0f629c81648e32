#!/usr/bin/env python3
"""Generates tests/golden/caller_basis.npz by EXECUTING THE REFERENCE'S OWN temporal-basis model -- dnerf/network_basis.py
`NeRFNetwork` (what `main_dnerf.py --basis` selects) under dnerf/renderer.py `run_cuda` -- imported from /root/reference, never
copied, over the oracle-backed operator shims of tests/ref_shims/, the way gen_caller_fixtures.py makes the other caller fixtures.

Model: the reference's class constructed under torch.manual_seed(G.SEED) with the bench scene's recipe (tests/basis_support.py states
it once for both sides): embeddings x 1e3, the bench scene's occupancy bits, and the first 32 rows of the last sigma layer -- the
density coefficients -- scaled by ONE float32 factor so that the median of log sigma on the probe points of slice 32 at time 0.5 is
the one gen_caller_fixtures calibrates to.  The factor is recorded (a scalar; no weights are): the mirror built from the seed and the
factor must reproduce every state-dict digest.

Recorded: the digests, `forward` (sigma, rgb) and `density` (sigma, geo_feat) on 2048 seeded points and the basis row at each of the
three times, and a 64 x 64 `run_cuda` frame at each time (trace, image, depth, weights_sum).

Run in the build container only:   python tests/golden/gen_basis_fixture.py
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

import basis_support as BS  # noqa: E402


def build_reference_model():
    import dnerf.network_basis as ref_basis
    torch.manual_seed(G.SEED)
    model = ref_basis.NeRFNetwork(**BS.MODEL_KW)
    model.encoder.embeddings.mul_(1e3)
    model.eval()
    bits = BS.occupancy_bits(model.time_size, model.grid_size, G.scene)
    model.density_bitfield.copy_(torch.from_numpy(bits))
    # density calibration on slice 32 at time 0.5 with the reference's own density(): log sigma is linear in the coefficient rows
    pts = torch.from_numpy(G.probe_points(bits[32][: model.grid_size ** 3 // 8], 8192, G.SEED))
    med = float(torch.log(model.density(pts, torch.tensor([[0.5]]))["sigma"]).median())
    assert med != 0
    scale = np.float32(math.log(G.MEDIAN_SIGMA_DT / (2 * math.sqrt(3) / 1024)) / med)
    BS.scale_density_rows(model, scale)
    return model, bits, scale


def basis_row(model, t):
    """The 32 + 8 basis weights of time t from the reference's own layers (network_basis.py:128-137 restated as calls of them)."""
    h = model.encoder_time(torch.tensor([[t]], dtype=torch.float32))
    for l in range(model.num_layers_basis):
        h = model.basis_net[l](h)
        if l != model.num_layers_basis - 1:
            h = torch.relu(h)
    return h[0].numpy().copy()


def main():
    model, bits, scale = build_reference_model()
    digests = G.state_digests(model)
    out = dict(seed=np.int32(G.SEED), times=np.array(BS.TIMES, np.float32), sigma_scale=scale, digest_keys=np.array(sorted(digests)),
               digest_vals=np.array([digests[k] for k in sorted(digests)]),
               bitfield_sha=np.array([G.sha(bits[BS.slice_of(t, model.time_size)]) for t in BS.TIMES]))
    x, d = BS.seeded_points()
    out["x"], out["d"] = x, d
    ro, rd, _ = G.camera_rays(64, 64)
    for t in BS.TIMES:
        tt = torch.tensor([[t]], dtype=torch.float32)
        s, c, _ = model(torch.from_numpy(x), torch.from_numpy(d), tt)
        dens = model.density(torch.from_numpy(x), tt)
        out[f"t{t}_sigma"], out[f"t{t}_rgb"] = s.numpy().copy(), c.numpy().copy()
        out[f"t{t}_density_sigma"], out[f"t{t}_density_geo"] = dens["sigma"].numpy().copy(), dens["geo_feat"].numpy().copy()
        out[f"t{t}_basis"] = basis_row(model, t)
        r = G.run_infer(model, ro, rd, t)
        for k, v in r.items():
            out[f"t{t}_{k}"] = v
        print(f"[basis t={t}] iterations {len(r['trace'])}, first rows {r['trace'][:3].tolist()}, image mean {r['image'].mean():.6f}, "
              f"median log sigma {float(np.median(np.log(out[f't{t}_sigma']))):.3f}")
        assert len(r["trace"]) >= 4, "the frame must take at least 4 loop iterations"
    a, b = out[f"t{BS.TIMES[0]}_image"], out[f"t{BS.TIMES[-1]}_image"]
    moved = int((np.abs(a - b).max(1) > 1e-2).sum())
    print(f"pixels that differ by more than 1e-2 between t = {BS.TIMES[0]} and t = {BS.TIMES[-1]}: {moved}")
    assert moved >= 100, "the frames must depend on the time stamp"
    np.savez_compressed(BS.FIXTURE, **out)
    print("wrote", BS.FIXTURE, f"{os.path.getsize(BS.FIXTURE) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
