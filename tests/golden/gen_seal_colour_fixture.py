#!/usr/bin/env python3
"""Generates tests/golden/seal_colour_edges.npz by EXECUTING THE REFERENCE'S OWN colour code on the CPU, imported from the reference tree,
never copied: SealNeRF/color_utils.py (rgb2hsv_torch, :31-44, by file path, as gen_golden_color.py does) and SealNeRF/seal_utils.py
(modify_hsv :747-758, modify_rgb :761-777, through the import environment of tests/ref_shims, as gen_caller_fixtures.py does).

The inputs are the ones tests/seal_colour_support.py states -- the lattice of ties, greys and subnormals, the sextant boundaries, seeded
colours; modifications that make the hue negative and push h * 6 past 256; grey, black, white and tied tint targets; light offsets that
drive the brightness to either clamp -- and the file holds inputs and outputs only:
  colours [N,3], constant_v [512,3], mods [11,3], targets [5,3], light_offsets [4]
  modify_hsv [11,N,3]                 modify_hsv(colours, mods[k])
  rgb2hsv [N,3]                       rgb2hsv_torch(colours)
  modify_rgb_random [5,4,512,3]       modify_rgb(the random block of colours, targets[t], light_offsets[o])
  modify_rgb_constant_v [5,4,512,3]   the same on constant_v
The archive is written with fixed member dates: running the generator again gives the same bytes.

Run in the build container only:   python tests/golden/gen_seal_colour_fixture.py
"""
import importlib.util
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests", "ref_shims"))
import stubs  # noqa: E402

stubs.install()
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import seal_colour_support as CS  # noqa: E402

torch.set_grad_enabled(False)


def write_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01, in the order given."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    spec = importlib.util.spec_from_file_location("ref_color_utils", os.path.join(stubs.REF, "SealNeRF", "color_utils.py"))
    ref_colour = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_colour)
    import SealNeRF.seal_utils as SU

    colours, constant_v = CS.colour_set(), CS.constant_v_set()
    out = dict(colours=colours, constant_v=constant_v, mods=CS.MODS, targets=CS.TARGETS, light_offsets=np.array(CS.LIGHT_OFFSETS, dtype=np.float32))
    t = torch.from_numpy(colours)
    out["modify_hsv"] = np.stack([SU.modify_hsv(t.clone(), torch.from_numpy(m.copy())).numpy().copy() for m in CS.MODS])
    out["rgb2hsv"] = ref_colour.rgb2hsv_torch(t.clone().view(-1, 3, 1)).view(-1, 3).numpy().copy()
    for name, cols in (("random", CS.random_block(colours)), ("constant_v", constant_v)):
        c = torch.from_numpy(np.ascontiguousarray(cols))
        out[f"modify_rgb_{name}"] = np.stack([np.stack([SU.modify_rgb(c.clone(), torch.from_numpy(tg.copy()), off).numpy().copy() for off in CS.LIGHT_OFFSETS])
                                              for tg in CS.TARGETS])
    for k, v in out.items():
        assert v.dtype == np.float32 and not np.isnan(v).any(), k
    write_npz(CS.FIXTURE, out)
    size = os.path.getsize(CS.FIXTURE)
    print("wrote", CS.FIXTURE, f"{size / 1024:.0f} KiB;", colours.shape[0], "colours")
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()
