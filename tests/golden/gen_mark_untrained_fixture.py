#!/usr/bin/env python3
"""Generates tests/golden/caller_mark_untrained.npz by EXECUTING THE REFERENCE'S OWN `NeRFRenderer.mark_untrained_grid`
(dnerf/renderer.py:389-451, imported from /root/reference, never copied) on the CPU, over the oracle-backed operator shims of
tests/ref_shims/ -- the way gen_caller_fixtures.py makes the other caller fixtures.  The only operator the method touches is
`raymarching.morton3D`.

Cases (tests/mark_untrained_support.py holds the inputs): three narrow look-at cameras at bound 1 (one cascade) and at bound 2
(two cascades), and one camera behind the grid looking away (every cell marked).  The reference renderer is built at its own size
(128^3) and its density grid cut to ONE time slice before the call: the method treats every slice alike (:449).

Per case the file holds data only: poses, intrinsic, bound, cascade, grid_size, the per-cascade count of marked cells, the unseen
mask bit-packed in Morton order (bit i % 8 of byte i / 8), and the share of borderline cells per cascade -- the generator refuses
to write a fixture whose share exceeds the tests' cap.

Run in the build container only:   python tests/golden/gen_mark_untrained_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref_shims"))
import stubs  # noqa: E402

stubs.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mark_untrained_support as MU  # noqa: E402


def main():
    import dnerf.renderer as ref_renderer
    out = {}
    for name, bound in MU.CASES.items():
        poses = MU.case_poses(name)
        model = ref_renderer.NeRFRenderer(bound=bound, cuda_ray=True)
        model.density_grid = torch.zeros_like(model.density_grid[:1])
        model.mark_untrained_grid(poses, MU.INTRINSIC)
        unseen = (model.density_grid[0] == -1).numpy()
        assert ((model.density_grid[0] == 0).numpy() | unseen).all()
        border = MU.borderline(model.grid_size, bound, model.cascade, poses, MU.INTRINSIC)        # asserts the cap
        # the float64 evaluation agrees with the reference's fp32 one off the borderline cells: the rule means what it says
        exact = ~(MU.margins64(model.grid_size, bound, model.cascade, poses, MU.INTRINSIC) > 0).any(axis=1)
        MU.assert_same_marks(unseen, exact, border, name)
        out.update({f"{name}_poses": poses, f"{name}_intrinsic": np.array(MU.INTRINSIC, np.float64), f"{name}_bound": np.float32(bound),
                    f"{name}_cascade": np.int32(model.cascade), f"{name}_grid_size": np.int32(model.grid_size),
                    f"{name}_marked": unseen.sum(axis=1).astype(np.int64),
                    f"{name}_unseen_bits": np.packbits(unseen, axis=1, bitorder="little"),
                    f"{name}_borderline_share": border.mean(axis=1)})
        print(f"[{name}] unseen share per cascade {unseen.mean(axis=1).round(4).tolist()}, borderline share {border.mean(axis=1).tolist()}")
    path = MU.FIXTURE
    np.savez_compressed(path, **out)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
