"""The brush's texture stamp (`imageConfig`, dnerf_amd/seal_mapper.py) on the CPU: the constructor's loader, and the torch restatement of
map_color's `image` branch against what the reference's own map_color produced (tests/golden/caller_seald_image.npz, made by
gen_image_fixture.py from the reference's code, data only).

Texel indices are compared on the fixture's clear points -- both float64 texel coordinates at least 1e-3 texel from every integer
1..W-1 / 1..H-1 (0 of 389 are unclear) -- and are read off the output colours of an index texture (column in the hue, row in the
saturation).  Colours: the project's fp32 bar, 1e-4 (observed: 0 -- the restatement runs the reference's statements on the same library)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import seal_image_support as IS
from dnerf_amd import seal_mapper as SM


@pytest.fixture(scope="module")
def fx():
    return np.load(IS.FIXTURE)


@pytest.fixture(scope="module")
def pngs(tmp_path_factory):
    d = tmp_path_factory.mktemp("stamp")
    return dict(dir=str(d), rgba=IS.write_png(d / "stamp_rgba.png", IS.stamp_texture()), rgb=IS.write_png(d / "stamp_rgb.png", IS.stamp_texture()[:, :, :3].copy()),
                index=IS.write_png(d / "index.png", IS.index_texture()))


def test_constructor_loads_the_texture(pngs):
    tex = IS.stamp_texture()
    m = SM.SealBrushMapper(IS.point_config(pngs["rgba"]))
    md = m.map_data
    assert md["image"].dtype == torch.float32 and md["image"].shape == (IS.H, IS.W, 3) and md["image_mask"].shape == (IS.H, IS.W)
    assert np.array_equal(md["image"].numpy(), tex[:, :, :3].astype(np.float32) / 255)
    assert np.array_equal(md["image_mask"].numpy(), (tex[:, :, 3] / 255).astype(np.float32))
    assert set(np.unique(md["image_mask"].numpy()).tolist()) >= {0.0, 1.0} and ((md["image_mask"] > 0) & (md["image_mask"] < 1)).sum() == 4 * IS.H
    for k, c in (("v_image_o", "o"), ("v_image_w", "w"), ("v_image_h", "h")):
        np.testing.assert_allclose(md[k].numpy(), np.asarray(IS.RECT[c], np.float32), rtol=0, atol=0)
    n = md["v_image_norm"].double().numpy()
    o, w, h = (np.asarray(IS.RECT[c]) for c in "owh")
    assert abs(np.linalg.norm(n) - 1) < 1e-6 and abs(n @ (w - o)) < 1e-7 and abs(n @ (h - o)) < 1e-7
    assert float(md["rgb_light_offset"]) == np.float32(IS.LIGHT_OFFSET) and "rgb" not in md
    assert float(SM.SealBrushMapper(dict(IS.point_config(pngs["rgba"]), rgbLightOffset=0)).map_data["rgb_light_offset"]) == 0.0
    # no alpha channel: the mask is all ones
    m3 = SM.SealBrushMapper(IS.point_config(pngs["rgb"]))
    assert np.array_equal(m3.map_data["image"].numpy(), md["image"].numpy()) and bool((m3.map_data["image_mask"] == 1).all())
    assert isinstance(SM.get_seal_mapper(IS.point_config(pngs["rgba"])), SM.SealBrushMapper)


def test_path_resolution_and_what_cannot_be_loaded(pngs, tmp_path, monkeypatch):
    name = os.path.basename(pngs["rgba"])
    with pytest.raises(NotImplementedError, match=name):            # relative, no config_path: not found
        SM.SealBrushMapper(IS.point_config(name))
    a = SM.SealBrushMapper(IS.point_config(name), config_path=pngs["dir"])                                    # the edit's directory
    b = SM.get_seal_mapper(IS.point_config(name), os.path.join(pngs["dir"], "seal.json"))                     # ... or a file in it
    assert torch.equal(a.map_data["image"], b.map_data["image"]) and a.map_data["image"].shape == (IS.H, IS.W, 3)
    bad = tmp_path / "broken.png"
    bad.write_bytes(b"\x89PNG\r\n\x1a\nthis is not a png")
    with pytest.raises(NotImplementedError, match="broken.png"):
        SM.SealBrushMapper(IS.point_config(str(bad)))
    from PIL import Image
    grey, deep = tmp_path / "grey.png", tmp_path / "deep.png"
    Image.fromarray(IS.stamp_texture()[:, :, 0].copy(), "L").save(grey)
    Image.fromarray((IS.stamp_texture()[:, :, 0].astype(np.uint16) * 257), "I;16").save(deep)
    for p in (grey, deep):
        with pytest.raises(NotImplementedError, match=p.name):
            SM.SealBrushMapper(IS.point_config(str(p)))
    monkeypatch.setattr(SM, "MAX_STAMP_TEXELS", IS.W * IS.H)        # (a real file of 2^28 texels is out of a test's reach)
    with pytest.raises(ValueError, match="texels"):
        SM.SealBrushMapper(IS.point_config(pngs["rgba"]))
    monkeypatch.undo()
    for mode in ("ease-in", "ease-out"):                             # still not built
        with pytest.raises(NotImplementedError):
            SM.SealBrushMapper(dict(IS.point_config(pngs["rgba"]), attenuationMode=mode))
    # the other mappers ignore the key, as the reference does
    from seal_anchor_support import POINTS_CONFIG as ANCHOR_CONFIG
    assert "image" not in SM.get_seal_mapper(dict(ANCHOR_CONFIG, imageConfig=dict(IS.RECT, path="nowhere.png"))).map_data


def test_restatement_reproduces_the_reference_colours(fx, pngs):
    pts, cols = torch.from_numpy(fx["points"]), torch.from_numpy(fx["colors_in"])
    for name, rgb in (("stamp", False), ("rgb_stamp", True)):
        m = SM.SealBrushMapper(IS.point_config(pngs["rgba"], rgb=rgb))
        got = m.map_color(pts, None, cols.clone()).numpy()
        err = float(np.abs(got - fx[f"colors_out_{name}"]).max())
        print(name, "largest colour difference against the reference", err)
        assert err <= 1e-4
        assert float(np.abs(got - fx["colors_in"]).max()) > 0.1
    with pytest.raises(ValueError, match="points"):
        m.map_color(None, None, cols.clone())
    # transparent texels hand the (untinted) colour back, opaque ones the unblended modify_rgb value of their texel
    m = SM.SealBrushMapper(IS.point_config(pngs["rgba"]))
    got = m.map_color(pts, None, cols.clone())
    tex = IS.stamp_texture()
    alpha = tex[fx["idx_h"], fx["idx_w"], 3]
    clear = fx["clear"]
    assert torch.equal(got[torch.from_numpy(clear & (alpha == 0))], cols[torch.from_numpy(clear & (alpha == 0))])
    target = torch.from_numpy(tex[fx["idx_h"], fx["idx_w"], :3].astype(np.float32) / 255)
    whole = SM.modify_rgb(cols.clone(), target, IS.LIGHT_OFFSET)
    opaque = torch.from_numpy(clear & (alpha == 255))
    assert int(opaque.sum()) >= 50 and torch.equal(got[opaque], whole[opaque])


def test_texel_indices_are_exact_on_clear_points(fx, pngs):
    u, v, clear, iw, ih = IS.texel_coordinates64(fx["points"])
    assert np.array_equal(clear, fx["clear"]) and np.array_equal(iw, fx["idx_w"]) and np.array_equal(ih, fx["idx_h"])
    assert (~clear).mean() <= IS.CLEAR_CAP
    assert np.array_equal(fx["ref_idx_w"][clear], iw[clear]) and np.array_equal(fx["ref_idx_h"][clear], ih[clear])
    m = SM.SealBrushMapper(IS.point_config(pngs["index"]))
    got_w, got_h = IS.decode_index(m.map_color(torch.from_numpy(fx["points"]), None, torch.from_numpy(fx["colors_in"]).clone()).numpy())
    print("unclear", int((~clear).sum()), "index mismatches in all", int(((got_w != iw) | (got_h != ih)).sum()))
    assert np.array_equal(got_w[clear], iw[clear]) and np.array_equal(got_h[clear], ih[clear])
    # every side clamps, and the texture is wider than high: a swapped index could not pass
    assert (u < 0).any() and (u >= IS.W).any() and (v < 0).any() and (v >= IS.H).any() and iw.max() == IS.W - 1 > ih.max() == IS.H - 1


def test_the_mean_spans_the_whole_call(fx, pngs):
    """modify_rgb's mean brightness is taken over ALL colours of the call: changing only the colours that land on transparent texels --
    which come back unchanged themselves -- changes the results on opaque texels."""
    m = SM.SealBrushMapper(IS.point_config(pngs["rgba"]))
    pts, cols = torch.from_numpy(fx["points"]), torch.from_numpy(fx["colors_in"])
    alpha = IS.stamp_texture()[fx["idx_h"], fx["idx_w"], 3]
    transparent, opaque = torch.from_numpy(fx["clear"] & (alpha == 0)), torch.from_numpy(fx["clear"] & (alpha == 255))
    darker = cols.clone()
    darker[transparent] *= 0.25
    a, b = m.map_color(pts, None, cols.clone()), m.map_color(pts, None, darker.clone())
    assert torch.equal(b[transparent], darker[transparent])
    shift = float(cols.max(1)[0].mean() - darker.max(1)[0].mean())
    unclamped = opaque & (a.max(1)[0] < 0.99) & (b.max(1)[0] < 0.99) & (a.max(1)[0] > 0.01)
    assert shift > 0.1 and int(unclamped.sum()) >= 20
    np.testing.assert_allclose((b.max(1)[0] - a.max(1)[0])[unclamped].numpy(), shift, rtol=0, atol=1e-5)     # V rises by what the mean fell


def test_map_color_inplace_form_takes_the_points(fx, pngs):
    """`map_color_` on CPU buffers is the restatement on the masked slots; it needs the points buffer."""
    m = SM.SealBrushMapper(IS.point_config(pngs["rgba"]))
    n = fx["points"].shape[0]
    pts, cols, mask = torch.zeros(2 * n, 3), torch.rand(2 * n, 3, generator=torch.Generator().manual_seed(5)), torch.zeros(2 * n, dtype=torch.bool)
    pts[::2], cols[::2], mask[::2] = torch.from_numpy(fx["points"]), torch.from_numpy(fx["colors_in"]), True
    keep = cols.clone()
    got = m.map_color_(cols, mask, points=pts)
    np.testing.assert_allclose(got[::2].numpy(), fx["colors_out_stamp"], rtol=0, atol=1e-4)
    assert torch.equal(got[1::2], keep[1::2])
    with pytest.raises(ValueError, match="points"):
        m.map_color_(cols, mask)


def test_image_records_match_the_c_header(tmp_path):
    """`SdnSealImage` and `SdnSealBrush` (which reaches it through its last field) against include/sdn_hip.h."""
    import sdn_backend as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    records = {"SdnSealImage": B.SdnSealImage, "SdnSealBrush": B.SdnSealBrush}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdn_hip.h"', 'int main(void) {']
    for name, rec in records.items():
        lines.append(f'  printf("{name} size %zu\\n", sizeof({name}));')
        for field, _ in rec._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, field, value = line.split()
        rec = records[name]
        assert int(value) == (ctypes.sizeof(rec) if field == "size" else getattr(rec, field).offset), (name, field)
        seen += 1
    assert seen == sum(len(r._fields_) + 1 for r in records.values())
    assert B.SdnSealBrush._fields_[-1][0] == "image" and B.SEAL_IMAGE_MAX_TEXELS == SM.MAX_STAMP_TEXELS == 1 << 28
