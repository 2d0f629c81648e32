"""SealD-NeRF bounding-box, anchor (control-point) and brush mappers on the device (scope row "next" #1): the objects the teacher /
student renderers hook between the marcher and the field network (`map_to_origin`) and after it (`map_color`).

Mirrors, with the same names and `map_data` keys, the pieces of the reference that sit inside the render loop:
  * `SealMapper.map_mask` / `map_color` (hsv, rgb and the brush's
    `image` texture stamp) / `map_data_conversion`                   SealNeRF/seal_utils.py:40-153
  * `SealBBoxMapper.__init__` / `map_to_origin`                      SealNeRF/seal_utils.py:156-286
  * `SealAnchorMapper.__init__` / `map_to_origin`, `project_points`  SealNeRF/seal_utils.py:464-578, 736-744
  * `SealBrushMapper.__init__` / `map_to_origin`, `get_trimesh_fit`,
    `mesh_surface_points_mask`                                       SealNeRF/seal_utils.py:304-461, 599-631, 720-733
  * `moller_trumbore`, `points_in_mesh`                              SealNeRF/seal_utils.py:638-693
  * `modify_hsv`, `modify_rgb`                                       SealNeRF/seal_utils.py:747-777
  * `rgb2hsv_torch`, `hsv2rgb_torch` ([N,3] form)                    SealNeRF/color_utils.py:31-63
without pytorch3d / trimesh / open3d / scikit-spatial (none is installed here): the bbox mapper's "from" box is the oriented box of the config's `raw`
points, the "to" box its scaled + transformed image, both as 8 vertices / 12 triangles.

One documented difference: trimesh's `bounding_box_oriented` searches a minimum-volume box over the convex hull; here `raw` is
expected to be (what the Seal GUI writes) the 8 corners of a cuboid, which are recognised exactly; any other point set gets its
PCA-aligned box.  Everything is plain torch on whatever device the points live on -- it runs on the sample stream of the HIP
operators; colour conversions are pinned by vectors generated from the reference's pure-torch `color_utils` (tests/golden).
"""
import itertools
import os

import numpy as np
import torch

_TEST_DIR = (0.4395064455, 0.617598629942, 0.652231566745)   # trimesh's "magic" ray direction, seal_utils.py:684-686


# ----------------------------------------------------------------------------------------------------------------------
# colour (color_utils.py:31-63 on [N,3] tensors; seal_utils.py:747-777)
# ----------------------------------------------------------------------------------------------------------------------
def rgb2hsv(rgb):
    cmax, cmax_idx = torch.max(rgb, dim=1, keepdim=True)
    cmin = torch.min(rgb, dim=1, keepdim=True)[0]
    delta = cmax - cmin
    r, g, b = rgb[:, 0:1], rgb[:, 1:2], rgb[:, 2:3]
    safe = torch.where(delta == 0, torch.ones_like(delta), delta)
    h = torch.where(cmax_idx == 0, ((g - b) / safe) % 6, torch.where(cmax_idx == 1, (b - r) / safe + 2, (r - g) / safe + 4))
    h = torch.where(delta == 0, torch.zeros_like(h), h) / 6.0
    s = torch.where(cmax == 0, torch.zeros_like(cmax), delta / torch.where(cmax == 0, torch.ones_like(cmax), cmax))
    return torch.cat([h, s, cmax], dim=1)


def hsv2rgb(hsv):
    h, s, v = hsv[:, 0:1], hsv[:, 1:2], hsv[:, 2:3]
    c = v * s
    x = c * (-torch.abs(h * 6.0 % 2.0 - 1) + 1.0)
    m = v - c
    o = torch.zeros_like(c)
    idx = (h * 6.0).to(torch.uint8) % 6            # the reference's `.type(torch.uint8)` truncation, then % 6
    table = [(c, x, o), (x, c, o), (o, c, x), (o, x, c), (x, o, c), (c, o, x)]
    rgb = torch.zeros_like(hsv)
    for k, (rr, gg, bb) in enumerate(table):
        rgb = torch.where(idx == k, torch.cat([rr, gg, bb], dim=1), rgb)
    return rgb + m


def modify_hsv(rgb, modification):
    if rgb.shape[0] == 0:
        return rgb
    hsv = rgb2hsv(rgb)
    mod = torch.as_tensor(modification, device=rgb.device, dtype=rgb.dtype).view(1, 3)
    return hsv2rgb(hsv + mod)


def modify_rgb(rgb, modification, light_offset=0.0):
    """modification: one target colour [3], or one per sample [N,3] (the texture stamp's texels, seal_utils.py:77-78)."""
    if rgb.shape[0] == 0:
        return rgb
    hsl = rgb2hsv(rgb)
    mod = rgb2hsv(torch.as_tensor(modification, device=rgb.device, dtype=rgb.dtype).view(-1, 3))
    raw_l = hsl[:, 2:3]
    raw_l_offset = raw_l - raw_l.mean()
    out = torch.cat([mod[:, :2].expand(rgb.shape[0], 2), (mod[:, 2:3] + raw_l_offset + light_offset).clamp(0, 1)], dim=1)
    return hsv2rgb(out)


# ----------------------------------------------------------------------------------------------------------------------
# geometry (seal_utils.py:638-693)
# ----------------------------------------------------------------------------------------------------------------------
def moller_trumbore(ray_o, ray_d, tris, eps=1e-8):
    """[m,3] rays x [n,3,3] triangles -> bool [m]: does the ray (t >= 0) hit any triangle."""
    e1 = tris[:, 1] - tris[:, 0]
    e2 = tris[:, 2] - tris[:, 0]
    n = torch.cross(e1, e2, dim=-1)
    invdet = 1.0 / -(torch.einsum("md,nd->mn", ray_d, n) + eps)
    a0 = ray_o[:, None] - tris[None, :, 0]
    da0 = torch.cross(a0, ray_d[:, None].expand(*a0.shape), dim=-1)
    u = torch.einsum("mnd,nd->mn", da0, e2) * invdet
    v = -torch.einsum("mnd,nd->mn", da0, e1) * invdet
    t = torch.einsum("mnd,nd->mn", a0, n) * invdet
    return ((t >= 0.0) & (u >= 0.0) & (v >= 0.0) & ((u + v) <= 1.0)).any(1)


def points_in_mesh(points, triangles, rays_d=None):
    """A point is inside iff both the ray along the test direction and the opposite ray hit the mesh."""
    if rays_d is None:
        rays_d = torch.tensor([_TEST_DIR], device=points.device, dtype=points.dtype)
    d = rays_d.to(points.dtype).repeat(points.shape[0], 1)
    mask = moller_trumbore(torch.cat([points, points]), torch.cat([d, -d]), triangles.to(points.dtype))
    return mask[:points.shape[0]] & mask[-points.shape[0]:]


_BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6],
                       [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int64)   # vertex k = origin + (k&1) e1 + (k>>1&1) e2 + (k>>2) e3


def oriented_box(points):
    """-> (vertices [8,3] float64 in the corner order of _BOX_FACES, centre [3]).  8 cuboid corners are recognised exactly
    (any order); other point sets get their PCA-aligned bounding box."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if p.shape[0] == 8:
        diam = np.linalg.norm(p - p.mean(0), axis=1).max() * 2
        tol = 1e-6 * max(diam, 1e-12)
        rest = list(range(1, 8))
        for trio in itertools.combinations(rest, 3):
            e = p[list(trio)] - p[0]
            if max(abs(e[0] @ e[1]), abs(e[0] @ e[2]), abs(e[1] @ e[2])) > 1e-6 * diam * diam:
                continue
            verts = np.stack([p[0] + (k & 1) * e[0] + ((k >> 1) & 1) * e[1] + (k >> 2) * e[2] for k in range(8)])
            d = np.linalg.norm(verts[:, None] - p[None], axis=-1)
            if (d.min(1) < tol).all() and (d.min(0) < tol).all():
                return verts, verts.mean(0)
    c = p.mean(0)
    _, _, vt = np.linalg.svd(p - c, full_matrices=False)
    q = (p - c) @ vt.T
    lo, hi = q.min(0), q.max(0)
    verts = np.stack([c + (np.array([(hi if (k >> a) & 1 else lo)[a] for a in range(3)])) @ vt for k in range(8)])
    return verts, verts.mean(0)


def _bounds(verts):
    return np.stack([verts.min(0), verts.max(0)])


class SealMapper:
    """seal_utils.py:18-153 (the parts used inside the render loop)."""

    def __init__(self, seal_config):
        self.config = seal_config
        self.device = "cpu"
        self.dtype = torch.float32
        self.map_data = {}
        self.map_triangles = None
        self.map_test_dir = None

    def _read_color_options(self):
        """The config's colour options (seal_utils.py: the tail of every mapper's constructor) into `map_data`."""
        if "hsv" in self.config:
            self.map_data["hsv"] = self.config["hsv"]
        if "rgb" in self.config:
            self.map_data["rgb"] = self.config["rgb"]
            self.map_data["rgb_light_offset"] = self.config.get("rgbLightOffset", 0)

    def map_data_conversion(self, T=None, force=False):
        if T is None and not force:
            return
        if T is not None and (self.device != T.device or self.dtype != T.dtype):
            self.device, self.dtype = T.device, T.dtype
        elif not force:
            return
        for k, v in self.map_data.items():
            if isinstance(v, str):             # (the brush's `attenuation_mode`)
                continue
            self.map_data[k] = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(self.device, self.dtype)
        if self.map_triangles is not None:
            self.map_triangles = self.map_triangles.to(self.device, self.dtype)
        if self.map_test_dir is not None:
            self.map_test_dir = self.map_test_dir.to(self.device, self.dtype)

    def map_mask(self, points):
        bounds = self.map_data["map_bound"]
        if bounds.ndim == 2:
            bounds = bounds[None]
        bound_mask = None
        for i in range(bounds.shape[0]):
            cur = torch.logical_and(points.all(1), torch.logical_and(bounds[i][1] > points, points > bounds[i][0]).all(1))
            bound_mask = cur if bound_mask is None else torch.logical_or(bound_mask, cur)
        if not bound_mask.any():
            return bound_mask
        shape_mask = points_in_mesh(points[bound_mask], self.map_triangles, self.map_test_dir)
        bound_mask[bound_mask.clone()] = shape_mask
        return bound_mask

    def map_color(self, points, dirs, colors):
        if "hsv" in self.map_data:
            colors = modify_hsv(colors, self.map_data["hsv"])
        if "rgb" in self.map_data:
            colors = modify_rgb(colors, self.map_data["rgb"], float(self.map_data["rgb_light_offset"]))
        if "image" in self.map_data:
            # seal_utils.py:58-79, statement by statement.  points: the MAPPED positions of the samples `colors` belongs to
            if points is None:
                raise ValueError("map_color: a mapper with an `image` needs the (mapped) points of the colours")
            image = self.map_data["image"]
            H, W, C = image.shape
            v_norm, v_o, v_w, v_h = (self.map_data[k] for k in ("v_image_norm", "v_image_o", "v_image_w", "v_image_h"))
            projected_points = project_points(v_norm, v_o, points)
            v_op = projected_points - v_o
            v_ow = v_w - v_o
            v_oh = v_h - v_o
            len_ow = torch.norm(v_ow, 2)
            len_oh = torch.norm(v_oh, 2)
            zero = torch.tensor(0., device=points.device)
            idx_w = torch.min(torch.max(zero, torch.floor(v_op @ v_ow.T / len_ow ** 2 * W)), torch.tensor(W - 1, device=points.device)).to(torch.long)
            idx_h = torch.min(torch.max(zero, torch.floor(v_op @ v_oh.T / len_oh ** 2 * H)), torch.tensor(H - 1, device=points.device)).to(torch.long)
            mask = self.map_data["image_mask"][idx_h, idx_w][None].T
            modified_colors = modify_rgb(colors, image[idx_h, idx_w], float(self.map_data["rgb_light_offset"]))    # the mean V: of ALL colours of the call
            colors = mask * modified_colors + (1 - mask) * colors
        return colors

    @torch.no_grad()
    def map_to_origin(self, points, dirs=None):
        """-> (points', dirs', mask): the mapped samples taken back to where their content comes from (each mapper's docstring says how).
        CUDA fp32 inputs take the HIP kernel (on copies, as the reference returns copies); everything else the mapper's torch
        restatement `_map_to_origin_torch`."""
        if self._native_ok(points, dirs):
            self.map_data_conversion(points)
            p, d = points.clone(), dirs.clone()
            return p, d, self.map_to_origin_(p, d)
        return self._map_to_origin_torch(points, dirs)

    def _map_to_origin_torch(self, points, dirs=None):
        raise NotImplementedError()

    @property
    def redirects_source(self):
        """Does `map_to_origin` carry the bbox mapper's `mapSource` redirect?  (Only that mapper's `map_data["map_source"]` is one: the
        anchor mapper stores a flag for pretraining under the same key.)"""
        return False

    # ---- device fast path: csrc/seal.hip, one lane per sample slot, in place ---------------------------------------------
    # (shared by the mappers: the box test's arguments, the colour part and the frame of `map_to_origin_` are the same for all of them;
    #  `_native_map_args` adds a mapper's own `map_to_origin` constants, `_native_map` is its kernel call.  For the device loop's records
    #  (`DeviceLoop.set_mapper`) a mapper states `native_kind`, the name of its `SdnSealBox.kind` in sdn_backend, and `native_box_fields`,
    #  the (name, length) array fields -- length None: a scalar -- of `SdnSealBox` it fills from `_native_args`, beside the box test's)
    native_kind = None
    native_box_fields = ()

    def _native_brush_record(self, a):
        """The mapper's `SdnSealBrush` record from `_native_args`: the brush's; None for every other mapper."""
        return None

    def _native_box_record(self, a):
        """The mapper's `SdnSealBox` record from `_native_args`: the box test's bounds and triangles, the mapper's own
        `native_box_fields`, the hsv / rgb colour edit and the bbox mapper's mapSource.  `scratch` stays empty: the loop that takes the
        record owns those bytes (and keeps `a`, which the record points into, alive)."""
        import sdn_backend
        box = sdn_backend.SdnSealBox()
        for k in range(6 * a["n_bounds"]):
            box.bounds[k] = a["bounds"][k]
        box.n_bounds, box.n_tris, box.tris = a["n_bounds"], a["n_tris"], a["tris"].data_ptr()
        box.kind = getattr(sdn_backend, self.native_kind)
        for name, n in self.native_box_fields:
            if n is None:
                setattr(box, name, a[name])
            for k in range(n or 0):
                getattr(box, name)[k] = a[name][k]
        if "hsv" in self.map_data:
            h = [float(v) for v in self.map_data["hsv"].reshape(-1).tolist()]
            box.hsv[0], box.hsv[1], box.hsv[2], box.modify_hsv = h[0], h[1], h[2], 1
        if "rgb" in a:
            box.rgb[0], box.rgb[1], box.rgb[2], box.rgb_light_offset, box.modify_rgb = a["rgb"][0], a["rgb"][1], a["rgb"][2], a["rgb_light_offset"], 1
        if self.redirects_source:
            for k in range(6):
                box.source_bound[k] = a["source_bound"][k]
            for k in range(3):
                box.map_source[k] = a["map_source"][k]
            box.has_map_source = 1
        return box

    def _native_ok(self, points, dirs):
        return (points.is_cuda and dirs is not None and points.dtype == torch.float32 and dirs.dtype == torch.float32
                and points.is_contiguous() and dirs.is_contiguous())

    def _native_map_args(self, md, f32, cfl):
        raise NotImplementedError()

    def _native_args(self, device):
        import ctypes
        key = str(device)
        if getattr(self, "_native_key", None) != key:
            f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))  # noqa: E731
            cfl = lambda a: (ctypes.c_float * a.size)(*a.reshape(-1).tolist())                          # noqa: E731
            md = {k: (v.detach().cpu().double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64))
                  for k, v in self.map_data.items() if not isinstance(v, str)}
            tri = self.map_triangles.detach().cpu().double().numpy()
            e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            tris12 = np.concatenate([tri[:, 0], e1, e2, np.cross(e1, e2)], axis=1)
            bounds = md["map_bound"].reshape(-1, 2, 3)
            self._native = dict(tris=torch.from_numpy(f32(tris12)).to(device), n_tris=int(tris12.shape[0]),
                                bounds=cfl(f32(bounds.reshape(-1, 6))), n_bounds=int(bounds.shape[0]),
                                test_dir=cfl(f32(_TEST_DIR if self.map_test_dir is None else self.map_test_dir.cpu().numpy())),
                                # [0..15] modify_rgb's sum / count, [16..19] the "did this call map anything" flag word (only ever raised),
                                # zeroed once; used by the in-place calls (a DeviceLoop keeps its own: loops on other streams share the mapper)
                                scratch=torch.zeros(32, dtype=torch.uint8, device=device))
            self._native.update(self._native_map_args(md, f32, cfl))
            if "rgb" in md:
                self._native["rgb"] = [float(v) for v in f32(md["rgb"].reshape(3))]
                self._native["rgb_light_offset"] = float(np.float32(md["rgb_light_offset"]))
            if "image" in md:
                self._native.update(self._native_image_args(md, f32, device))
            self._native_key = key
        return self._native

    def _native_image_args(self, md, f32, device):
        """The texture stamp's device record (`SdnSealImage`): the texels as 16-byte records {hue / 6, saturation, value, alpha} -- converted
        once, on the device, by the helper the kernels convert colours with -- and the plane constants, each taken in fp32 as the
        reference's statements take it (v_w - v_o, torch.norm(.)**2, plane_norm @ plane_norm on fp32 tensors).  Also 16 bytes of scratch
        of the stamp's own (its sum / count is not the tint's)."""
        from sdn_backend import SdnSealImage, lib, check, ptr, stream
        H, W = md["image"].shape[:2]
        texels = torch.from_numpy(np.concatenate([f32(md["image"]), f32(md["image_mask"])[..., None]], axis=-1).reshape(-1, 4)).to(device).contiguous()
        check(lib.sdn_seal_image_texels(ptr(texels), H * W, stream()), "seal_image_texels")
        torch.cuda.current_stream().synchronize()        # once per mapper and device: later calls may come on other streams
        v_o, v_w, v_h, v_n = (torch.from_numpy(f32(md[k].reshape(3))) for k in ("v_image_o", "v_image_w", "v_image_h", "v_image_norm"))
        v_ow, v_oh = v_w - v_o, v_h - v_o
        rec = SdnSealImage()
        rec.texels, rec.W, rec.H = texels.data_ptr(), W, H
        for k in range(3):
            rec.v_o[k], rec.v_norm[k], rec.v_ow[k], rec.v_oh[k] = float(v_o[k]), float(v_n[k]), float(v_ow[k]), float(v_oh[k])
        rec.norm_sq, rec.len_ow_sq, rec.len_oh_sq = float(v_n @ v_n), float(torch.norm(v_ow, 2) ** 2), float(torch.norm(v_oh, 2) ** 2)
        rec.light_offset = float(np.float32(md["rgb_light_offset"]))
        return dict(image=rec, image_texels=texels, image_scratch=torch.zeros(16, dtype=torch.uint8, device=device))

    def _native_map(self, lib, a, points, dirs, M, mask):
        """The mapper's one `lib.sdn_seal_*_map` call on the sample buffers -> (the call's name for the error text, its return code)."""
        raise NotImplementedError()

    @torch.no_grad()
    def map_to_origin_(self, points, dirs):
        """In-place `map_to_origin` on the sample buffers (CUDA fp32 contiguous) -> bool mask [M]; the mapper's kernel of csrc/seal.hip.
        Every slot of the buffers is a sample of the call."""
        from sdn_backend import lib, check
        a = self._native_args(points.device)
        M = points.shape[0]
        mask = torch.empty(M, dtype=torch.uint8, device=points.device)
        what, rc = self._native_map(lib, a, points, dirs, M, mask)
        check(rc, what)
        return mask.view(torch.bool)

    @torch.no_grad()
    def map_color_(self, rgbs, mask, whole_rays=None, points=None):
        """In-place `map_color` of the masked samples (seal_utils.py:48-79: the hsv modification, then the rgb tint, then the brush's
        texture stamp): HIP kernels on CUDA fp32 buffers, the torch restatement otherwise.

        points: the MAPPED positions [M,3] of the samples (the buffer `map_to_origin_` ran on; the reference's `mapped_xyzs`), required
        when the mapper carries an `image`: the stamp looks its texel up by position.

        whole_rays: the buffers hold EVERY sample of a ray batch (march_rays_train's layout; `RayBatchRenderer`), not one loop iteration's:
        the record of that list -- rays [N,3], sigmas, deltas, N, T_thresh, max_steps and the renderer's work buffers scratch, ray_stop,
        slot_iter, n_iter (`sdn_seal_modify_rgb_whole_rays`) -- so that the tint re-centres each sample on the mean brightness of the
        loop iteration it would have been part of.  Only the tint and the stamp look at it (both take one mean per iteration); there is no
        torch restatement of that form."""
        stamp = "image" in self.map_data
        if stamp and points is None:
            raise ValueError("map_color_: a mapper with an `image` needs the (mapped) points of the samples")
        native = rgbs.is_cuda and rgbs.dtype == torch.float32 and rgbs.is_contiguous()
        if stamp:
            if points.shape[0] != rgbs.shape[0]:
                raise ValueError(f"map_color_: {points.shape[0]} points for {rgbs.shape[0]} colours")
            native = native and points.is_cuda and points.dtype == torch.float32 and points.is_contiguous()
        if native:
            import ctypes
            from sdn_backend import lib, check, ptr, stream
            m8 = mask.view(torch.uint8)
            M, w = rgbs.shape[0], whole_rays
            if w is not None:      # the whole-ray calls' arguments around the edit's own (target colour or image record, scratch)
                w_list = (ptr(w.rays, torch.int32, "rays"), ptr(w.sigmas, torch.float32, "sigmas"), ptr(w.deltas, torch.float32, "deltas"), M, w.N, w.T_thresh,
                          w.max_steps)
                w_work = (ptr(w.ray_stop, torch.int32, "ray_stop"), ptr(w.slot_iter, torch.int32, "slot_iter"), ptr(w.n_iter, torch.int32, "n_iter"), stream())
            if "hsv" in self.map_data:
                h = [float(v) for v in self.map_data["hsv"].reshape(-1).tolist()]
                check(lib.sdn_seal_modify_hsv(ptr(rgbs), ptr(m8), M, h[0], h[1], h[2], stream()), "seal_modify_hsv")
            if "rgb" in self.map_data:
                a = self._native_args(rgbs.device)
                c = a["rgb"]
                if w is not None:
                    check(lib.sdn_seal_modify_rgb_whole_rays(ptr(rgbs), ptr(m8), *w_list, c[0], c[1], c[2], a["rgb_light_offset"], ptr(w.scratch), *w_work),
                          "seal_modify_rgb_whole_rays")
                else:
                    check(lib.sdn_seal_modify_rgb(ptr(rgbs), ptr(m8), M, c[0], c[1], c[2], a["rgb_light_offset"], ptr(a["scratch"]),
                                                  None, None, None, stream()), "seal_modify_rgb")
            if stamp:         # after the tint, on the tinted colours; its sum / count in scratch of its own
                a = self._native_args(rgbs.device)
                rec = ctypes.addressof(a["image"])
                if w is not None:
                    check(lib.sdn_seal_modify_image_whole_rays(ptr(rgbs), ptr(points), ptr(m8), *w_list, rec, ptr(w.image_scratch), *w_work),
                          "seal_modify_image_whole_rays")
                else:
                    check(lib.sdn_seal_modify_image(ptr(rgbs), ptr(points), ptr(m8), M, rec, ptr(a["image_scratch"]), None, None, None, stream()),
                          "seal_modify_image")
        elif whole_rays is not None and ("rgb" in self.map_data or stamp):
            raise NotImplementedError("the whole-ray rgb tint / texture stamp is a device kernel (CUDA fp32 contiguous colours and points)")
        elif bool(mask.any()):
            rgbs[mask] = self.map_color(points[mask] if stamp else None, None, rgbs[mask]).to(rgbs.dtype)
        return rgbs


class SealBBoxMapper(SealMapper):
    """seal_utils.py:156-286.  seal_config: {type: 'bbox', raw: [N,3], transform: [4,4], scale: [3], boundType: 'from' | 'to' |
    'both', hsv / rgb / rgbLightOffset / mapSource optional}."""

    def __init__(self, seal_config, config_path=None):
        super().__init__(seal_config)
        T = np.array(seal_config["transform"], dtype=np.float64)
        R = T[:3, :3]
        scale = np.array(seal_config["scale"], dtype=np.float64)
        from_verts, from_center = oriented_box(seal_config["raw"])
        to_verts = (from_verts - from_center) * scale + from_center
        to_verts = to_verts @ R.T + T[:3, 3]
        to_center = to_verts.mean(0)
        self.from_vertices, self.to_vertices = from_verts, to_verts
        bound_type = seal_config.get("boundType", "to")
        fill_bounds = np.stack([_bounds(to_verts), _bounds(from_verts)])       # [2, 2, 3] like Meshes.get_bounding_boxes().transpose(1, 2)
        if bound_type == "to":
            bounds, tri = _bounds(to_verts), to_verts[_BOX_FACES]
        elif bound_type == "from":
            bounds, tri = _bounds(from_verts), from_verts[_BOX_FACES]
        elif bound_type == "both":
            bounds, tri = fill_bounds, np.concatenate([to_verts[_BOX_FACES], from_verts[_BOX_FACES]])
        else:
            raise ValueError(f"boundType {bound_type!r}")
        self.map_triangles = torch.from_numpy(tri)
        self.map_data = {
            "force_fill_bound": fill_bounds,
            "map_bound": bounds,
            "pose_center": (from_center + to_center) / 2,
            "pose_radius": np.linalg.norm(from_center - to_center, 2) * 10,
            "transform": np.linalg.inv(T),
            "rotation": np.linalg.inv(R),
            "scale": 1 / scale,
            "center": from_center,
        }
        self._read_color_options()
        if seal_config.get("mapSource"):
            self.map_data["empty_bound"] = _bounds(from_verts)
            self.map_data["map_source"] = seal_config["mapSource"]
        self.map_data_conversion(force=True)

    @property
    def redirects_source(self):
        return "map_source" in self.map_data

    def _native_map_args(self, md, f32, cfl):
        a = dict(tinv=cfl(f32(md["transform"][:3, :4])), rinv=cfl(f32(md["rotation"])), scale=cfl(f32(md["scale"])), center=cfl(f32(md["center"])))
        if self.redirects_source:
            a["source_bound"] = cfl(f32(md["empty_bound"].reshape(2, 3)))
            a["map_source"] = cfl(f32(md["map_source"].reshape(3)))
        return a

    native_kind = "SEAL_BBOX"
    native_box_fields = (("test_dir", 3), ("tinv", 12), ("rinv", 9), ("scale", 3), ("center", 3))

    def _native_map(self, lib, a, points, dirs, M, mask):
        from sdn_backend import ptr, stream
        if "map_source" in a:
            # (`mapSource`, seal_utils.py:269-273: the call's unmapped samples inside the source box move to one point -- if the call maps
            #  any sample at all, :251-252; every slot of the buffers is a sample of the call here)
            return "seal_bbox_map_source", lib.sdn_seal_bbox_map_source(
                ptr(points), ptr(dirs), M, a["bounds"], a["n_bounds"], ptr(a["tris"]), a["n_tris"], a["test_dir"], a["tinv"], a["rinv"], a["scale"],
                a["center"], a["source_bound"], a["map_source"], a["scratch"].data_ptr() + 16, ptr(mask), None, None, None, stream())
        return "seal_bbox_map", lib.sdn_seal_bbox_map(ptr(points), ptr(dirs), M, a["bounds"], a["n_bounds"], ptr(a["tris"]), a["n_tris"], a["test_dir"],
                                                      a["tinv"], a["rinv"], a["scale"], a["center"], ptr(mask), stream())

    @torch.no_grad()
    def _map_to_origin_torch(self, points, dirs=None):
        """Samples inside the target box are taken back to where their content comes from: inverse transform, inverse scale
        about the source centre, directions by the inverse rotation."""
        with torch.autocast(points.device.type if points.device.type != "cpu" else "cpu", enabled=False):
            self.map_data_conversion(points)
            has_dirs = dirs is not None
            mask = self.map_mask(points)
            if not mask.any():
                return points, dirs, mask
            inner = points[mask]
            n = inner.shape[0]
            hom = torch.vstack([inner.T, torch.ones([1, n], device=inner.device, dtype=inner.dtype)])
            moved = torch.matmul(self.map_data["transform"], hom).T[:, :3]
            origin = (moved - self.map_data["center"]) * self.map_data["scale"] + self.map_data["center"]
            points_copy = points.clone()
            dirs_copy = dirs.clone() if has_dirs else None
            if "map_source" in self.map_data:
                sb = self.map_data["empty_bound"]
                source_mask = torch.logical_and(sb[1] > points, points > sb[0]).all(1)
                points_copy[source_mask] = self.map_data["map_source"]
            points_copy[mask] = origin
            if has_dirs:
                dirs_copy[mask] = torch.matmul(self.map_data["rotation"], dirs[mask].T).T
            return points_copy, dirs_copy, mask


def best_fit_plane(points):
    """skspatial's `Plane.best_fit` in numpy -> (point, unit normal): the centroid, and the left singular vector of the centred
    points (as 3 x N) with the smallest singular value.  The normal's sign is the SVD's."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    c = p.mean(0)
    u, _, _ = np.linalg.svd((p - c).T, full_matrices=False)
    return c, u[:, -1]


def uv_sphere_points(radius, count=32):
    """`count` x `count` latitude / longitude points of a sphere about the origin (both poles included)."""
    theta = np.linspace(0.0, np.pi, count)
    phi = np.linspace(0.0, 2.0 * np.pi, count, endpoint=False)
    st = np.sin(theta)[:, None]
    return radius * np.stack([st * np.cos(phi)[None], st * np.sin(phi)[None], np.cos(theta)[:, None] * np.ones_like(phi)[None]], -1).reshape(-1, 3)


def project_points(plane_norm, plane_point, target_points):
    """seal_utils.py:736-744."""
    v_target_to_plane = target_points - plane_point
    v_projection = (v_target_to_plane @ plane_norm).unsqueeze(1) / (plane_norm @ plane_norm) * plane_norm
    return target_points - v_projection


class SealAnchorMapper(SealMapper):
    """seal_utils.py:464-578, the control-point (anchor) tool: the surface around an anchor is pulled along a vector.  seal_config:
    {type: 'anchor', raw: [N,3] points that determine the anchor plane (their mean is the anchor), translation: [3], radius: the
    affected radius in the plane, scale: [3], hsv / rgb / rgbLightOffset optional}.

    The deformed region is a cone: its base the disk of `radius` around the anchor in the plane, its apex at anchor + 1.1 *
    translation.  `map_to_origin` takes a sample of the cone back to the undeformed content: sheared back onto the plane's normal
    through the anchor, then squeezed towards the plane (a tenth of its remaining height is kept), then scaled about the anchor.

    The box (`to_mesh`) is the oriented box of the reference's point set: a sphere of 1.1 * radius about the anchor, the same sphere
    moved by -0.1 * translation, and anchor + 1.1 * translation.  The sphere is a 32 x 32 latitude / longitude point set (trimesh's
    `uv_sphere` is not available) and the box is `oriented_box`'s PCA-aligned one, so it may differ from trimesh's minimum-volume
    `bounding_box_oriented`.  What the box decides: `force_fill_bound` (the occupancy cells an edit render marks), and the early return
    of `map_to_origin` -- a call none of whose points lies in the box returns its inputs.  What it does not decide: WHICH points are
    mapped.  In a call that passes the gate the cone and plane-side tests run over all points, inside the box or not; the box
    contains the cone, so for two boxes that both do, the mapped sets differ only in calls that hold no point of the smaller box.
    `map_triangles`, `map_bound` and `force_fill_bound` all come from this one box.

    A translation that lies in the anchor plane has no height (`len_h == 0`, which the reference divides by): ValueError."""

    def __init__(self, seal_config, config_path=None):
        super().__init__(seal_config)
        v_translation = np.array(seal_config["translation"], dtype=np.float64)
        len_translation = np.linalg.norm(v_translation, 2)
        raw = np.asarray(seal_config["raw"], dtype=np.float64).reshape(-1, 3)
        v_anchor = raw.mean(0)
        radius = float(seal_config["radius"])
        plane_point, normal = best_fit_plane(raw)
        v_translated_anchor = v_anchor + v_translation
        v_projected_translated_anchor = v_translated_anchor - ((v_translated_anchor - plane_point) @ normal) * normal
        v_offset = v_projected_translated_anchor - v_anchor
        v_h = v_projected_translated_anchor - v_translated_anchor          # = -(translation . n) n: the same for either sign of n
        len_h = np.linalg.norm(v_h, 2)
        if not len_h > 1e-9 * len_translation:
            raise ValueError("the anchor's translation lies in the plane of its `raw` points (len_h == 0): there is no height to deform along")
        sphere = uv_sphere_points(radius * 1.1) + v_anchor
        self.to_vertices, to_center = oriented_box(np.vstack([sphere, v_anchor + 1.1 * v_translation, sphere - 0.1 * v_translation]))
        self.map_triangles = torch.from_numpy(self.to_vertices[_BOX_FACES])
        self.map_data = {
            "force_fill_bound": _bounds(self.to_vertices),
            "map_bound": _bounds(self.to_vertices),
            "pose_center": to_center,
            "pose_radius": len_translation * 10,
            "v_anchor": v_anchor,
            "v_offset": v_offset,
            "v_h": v_h,
            "len_h": len_h,
            "radius": radius,
            "scale": seal_config["scale"],
            "map_source": True,         # the reference's flag for pretraining (:512-513), NOT a bbox `mapSource` redirect: nothing here reads it
        }
        self._read_color_options()
        self.map_data_conversion(force=True)

    def _native_map_args(self, md, f32, cfl):
        return dict(v_anchor=cfl(f32(md["v_anchor"])), v_offset=cfl(f32(md["v_offset"])), v_h=cfl(f32(md["v_h"])), scale=cfl(f32(md["scale"])),
                    len_h=float(np.float32(md["len_h"])), radius=float(np.float32(md["radius"])))

    native_kind = "SEAL_ANCHOR"
    native_box_fields = (("test_dir", 3), ("scale", 3), ("v_anchor", 3), ("v_offset", 3), ("v_h", 3), ("len_h", None), ("radius", None))

    def _native_map(self, lib, a, points, dirs, M, mask):
        """`sdn_seal_anchor_map`: `dirs` are left as they are, as in the reference."""
        from sdn_backend import ptr, stream
        return "seal_anchor_map", lib.sdn_seal_anchor_map(
            ptr(points), ptr(dirs), M, a["bounds"], a["n_bounds"], ptr(a["tris"]), a["n_tris"], a["test_dir"], a["v_anchor"], a["v_offset"], a["v_h"],
            a["len_h"], a["radius"], a["scale"], a["scratch"].data_ptr() + 16, ptr(mask), None, None, None, stream())

    @torch.no_grad()
    def _map_to_origin_torch(self, points, dirs=None):
        """seal_utils.py:522-578, statement by statement."""
        with torch.autocast(points.device.type if points.device.type != "cpu" else "cpu", enabled=False):
            self.map_data_conversion(points)
            md = self.map_data
            map_mask = self.map_mask(points)
            if not map_mask.any():
                return points, dirs, map_mask
            projected_points = project_points(md["v_h"], md["v_anchor"], points)
            v_points_to_plane = projected_points - points
            points_plane_dist = torch.norm(v_points_to_plane, 2, 1)
            offset_scale = points_plane_dist.unsqueeze(1) / md["len_h"]
            scaled_offset = offset_scale * md["v_offset"]
            projected_offset_points = projected_points - scaled_offset
            pop_anchor_dist = torch.norm(projected_offset_points - md["v_anchor"], 2, 1)
            is_points_in_affected_cone = torch.logical_and(
                pop_anchor_dist <= md["radius"], points_plane_dist / (md["radius"] - pop_anchor_dist) < md["len_h"] / md["radius"] * 1.1)
            is_points_in_valid_side = v_points_to_plane @ md["v_h"] > 0
            valid_mask = torch.logical_and(is_points_in_affected_cone, is_points_in_valid_side)      # (not ANDed with map_mask)
            valid_points_plane_dist = points_plane_dist[valid_mask]
            v_map = -((md["len_h"] - valid_points_plane_dist) / 10)[None].T @ md["v_h"][None] / md["len_h"]
            mapped_points = projected_offset_points[valid_mask] - v_map
            mapped_points = (mapped_points - md["v_anchor"]) * md["scale"] + md["v_anchor"]
            points_copy = points.clone()
            points_copy[valid_mask] = mapped_points
            return points_copy, dirs, valid_mask


def knn_prism_faces(points, k=10):
    """The faces of `get_trimesh_fit` (seal_utils.py:603-617) for N points -> int64 [N * (k-1)(k-2)/2 * 4, 3] over the 2N vertices
    (bottom copy 0..N-1, top copy N..2N-1): each point with every pair of its k-1 nearest neighbours spans a bottom triangle, the top
    triangle above it and two triangles of the wall over the edge to the first neighbour of the pair.  The neighbours are found by
    brute force (no scikit-learn), ordered by (distance, index), the point itself first."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    if n < k:
        raise ValueError(f"a curve stroke needs at least {k} points for its {k}-nearest-neighbour mesh, got {n}")
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    d2[np.arange(n), np.arange(n)] = -1.0
    indices = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :k]
    jj, kk = np.triu_indices(k, 1)
    jj, kk = jj[jj >= 1], kk[jj >= 1]
    x = np.repeat(np.arange(n), jj.size)
    y, z = indices[:, jj].reshape(-1), indices[:, kk].reshape(-1)
    faces = np.stack([np.stack([x, y, z], 1), np.stack([x + n, y + n, z + n], 1), np.stack([x, y, x + n], 1), np.stack([x + n, y, y + n], 1)], 1)
    return faces.reshape(-1, 3).astype(np.int64)


def cluster_vertices(vertices, faces, voxel_size):
    """Vertex clustering with averaging (what open3d's `simplify_vertex_clustering(contraction=Average)` does): the vertices of one
    voxel of the grid with origin min bound - voxel_size / 2 become their mean; faces with a repeated vertex and duplicate faces
    (the same vertex cycle) go.  -> (vertices [V,3], faces [F,3]).  open3d is not available: this is a restatement -- clusters are
    numbered by voxel key (x, y, z lexicographic) and faces sorted, where open3d's hash containers give an unspecified order, and a
    vertex exactly on a voxel boundary may fall to the other side.  Neither changes the surface the ray test sees."""
    v = np.asarray(vertices, dtype=np.float64)
    origin = v.min(0) - 0.5 * voxel_size
    key = np.floor((v - origin) / voxel_size).astype(np.int64)
    _, cluster, count = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    cluster = cluster.reshape(-1)
    merged = np.zeros((count.shape[0], 3))
    np.add.at(merged, cluster, v)
    merged /= count[:, None]
    f = cluster[np.asarray(faces, dtype=np.int64)]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    first = np.argmin(f, axis=1)                               # rotate the cycle so that its smallest vertex comes first
    f = np.stack([f[np.arange(f.shape[0]), (first + r) % 3] for r in range(3)], 1)
    return merged, np.unique(f, axis=0)


def fit_prism_mesh(points, normal, growth, simplify_voxel=16):
    """`get_trimesh_fit` (seal_utils.py:599-631) in numpy -> (vertices, faces): the k-nearest-neighbour prism over `points` between
    points + normal * growth[0] and points + normal * growth[1], simplified by vertex clustering with a voxel of the largest extent /
    simplify_voxel."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    faces = knn_prism_faces(p)
    verts = np.concatenate([p + normal * growth[0], p + normal * growth[1]])
    voxel = (verts.max(0) - verts.min(0)).max() / simplify_voxel
    return cluster_vertices(verts, faces, voxel)


def mesh_surface_points_mask(triangles, points):
    """seal_utils.py:720-733: the points from which some +-1e-4 step along an axis leaves the mesh (default test direction)."""
    offset_value = 1e-4
    offsets = torch.from_numpy(np.array([[0, 0, offset_value], [0, 0, -offset_value], [0, offset_value, 0], [0, -offset_value, 0],
                                         [offset_value, 0, 0], [-offset_value, 0, 0]])).to(points.device, points.dtype)
    return torch.sum(torch.stack([~points_in_mesh(points + offsets[i], triangles) for i in range(offsets.shape[0])]), 0) > 0


def brush_triangle_records(triangles, test_dir):
    """The [F,16] fp32 triangle records of `sdn_seal_brush_map`: v0, E1, E2, N = E1 x E2, then moller_trumbore's inverse determinant
    1 / -(d . N + eps) for the ray along `test_dir` and for the opposite ray (fp32 arithmetic, eps = 1e-8: one direction serves all
    points, so neither depends on the point), two zeros of padding."""
    tri = np.asarray(triangles, dtype=np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    rec = np.zeros((tri.shape[0], 16), dtype=np.float32)
    rec[:, :12] = np.concatenate([tri[:, 0], e1, e2, np.cross(e1, e2)], axis=1).astype(np.float32)
    d = np.asarray(test_dir, dtype=np.float64).reshape(3).astype(np.float32)
    n = rec[:, 9:12]
    dn = n[:, 0] * d[0] + n[:, 1] * d[1] + n[:, 2] * d[2]
    with np.errstate(divide="ignore"):
        rec[:, 12] = np.float32(1.0) / -(dn + np.float32(1e-8))
        rec[:, 13] = np.float32(1.0) / -(-dn + np.float32(1e-8))
    return rec


_BRUSH_MODES = {"linear": 0, "dry": 1}
MAX_STAMP_TEXELS = 1 << 28     # the device record's texel index (SdnSealImage: H * W below this)


def load_stamp(path, config_path=None):
    """The brush's texture file as the reference's constructor holds it (seal_utils.py:392-401) -> (image [H,W,3] float32 = RGB / 255,
    image_mask [H,W] float64 = alpha / 255, or ones without an alpha channel).  Loaded with PIL (the reference uses cv2, which only
    decodes): an 8-bit RGB or RGBA file; for a lossless format (PNG) the arrays are what cv2 hands over, no parity is claimed for
    lossy ones.  `path` is tried as given, then relative to `config_path` (the edit's directory, or a file in it).  Anything that cannot
    be loaded here -- no such file, not an image, no PIL, 16-bit or palette-free grayscale data -- raises NotImplementedError naming
    the path and the cause."""
    tried = [path]
    if config_path is not None and not os.path.isabs(path):
        base = config_path if os.path.isdir(config_path) else os.path.dirname(config_path)
        tried.append(os.path.join(base, path))
    found = next((p for p in tried if os.path.isfile(p)), None)
    if found is None:
        raise NotImplementedError(f"the brush's `imageConfig` texture {path!r}: no such file (tried {tried})")
    try:
        from PIL import Image
    except ImportError as e:
        raise NotImplementedError(f"the brush's `imageConfig` texture {found!r}: PIL is needed to load it ({e})") from e
    try:
        with Image.open(found) as im:
            mode, (width, height) = im.mode, im.size
            raw = np.asarray(im) if mode in ("RGB", "RGBA") and width * height < MAX_STAMP_TEXELS else None
    except Exception as e:
        raise NotImplementedError(f"the brush's `imageConfig` texture {found!r} cannot be decoded: {e}") from e
    if width * height >= MAX_STAMP_TEXELS:
        raise ValueError(f"the brush's `imageConfig` texture {found!r} has {height} x {width} texels: at most 2^28 - 1")
    if raw is None or raw.dtype != np.uint8 or raw.ndim != 3 or raw.shape[2] not in (3, 4):
        raise NotImplementedError(f"the brush's `imageConfig` texture {found!r}: mode {mode!r} -- only 8-bit RGB / RGBA files are loaded "
                                  "(16-bit data, palettes and grayscale without a channel axis are not)")
    image = raw[:, :, :3].astype(np.float32) / 255
    alpha = raw[:, :, 3] / 255 if raw.shape[2] == 4 else np.ones(raw.shape[:2])
    return image, alpha


class SealBrushMapper(SealMapper):
    """seal_utils.py:289-461, the brush tool: the surface under a stroke is raised (or, with a negative pressure, lowered) along the
    stroke plane's normal.  seal_config: {type: 'brush', raw: [N,3] stroke points or a list of strokes [B][N_b,3] (B <= 4), normal: [3]
    the positive side of the plane, brushType: 'line' | 'curve' or one per stroke, simplifyVoxel: 16, brushDepth, brushPressure,
    attenuationDistance, attenuationMode: 'linear' | 'dry', hsv / rgb / rgbLightOffset optional}.

    Per stroke: the best-fit plane of its points, the normal turned towards `normal`, normal_expand = normal * brushPressure.  A 'line'
    stroke's mesh is the oriented box of the points moved by 2 normal_expand and by -brushDepth normal_expand (`oriented_box`: the
    documented PCA stand-in for trimesh's minimum-volume box); a 'curve' stroke's is `fit_prism_mesh` of its projected points between
    the same two offsets.  The stroke's border points are its projected points from which a 1e-4 step along some axis leaves its mesh.

    `map_to_origin` takes a sample inside one of the meshes back by normal_expand -- less towards the stroke's border: within
    attenuationDistance of the nearest border point the shift falls off linearly to zero.  'dry' changes colours only.  The map is
    per sample: which samples are mapped is `map_mask` alone, so, unlike the anchor mapper and `mapSource`, it also runs on frame
    groups.

    As in the reference, `normal_expand`, `center` and the ray test's direction (`map_test_dir`, not normalised) are the LAST stroke's:
    all strokes are assumed to lie in one plane.

    `imageConfig: {path, o, w, h}` stamps a texture onto the mapped samples' colours (`map_color`'s `image` branch, after hsv and rgb):
    the file (8-bit RGB / RGBA, loaded with PIL, see `load_stamp`) lies on the parallelogram with corner `o` and edges to `w` and `h`;
    a sample takes the texel its mapped position projects to (clamped at the edges) as `modify_rgb`'s target colour -- brightness
    re-centred on the mean of ALL masked samples of the call, plus `rgbLightOffset` -- blended in by the texel's alpha.  On the device:
    `sdn_seal_modify_image`.  A file this build cannot load raises NotImplementedError, a texture of 2^28 texels or more ValueError.

    Not built: the 'ease-in' / 'ease-out' modes (unimplemented in the reference too) raise NotImplementedError here, at construction;
    `to.obj` is not written."""

    MAX_STROKES = 4        # the device box test holds 4 bounds

    def __init__(self, seal_config, config_path=None):
        super().__init__(seal_config)
        missing = [k for k in ("raw", "brushType", "brushDepth", "brushPressure", "attenuationDistance", "attenuationMode") if k not in seal_config]
        if missing:
            raise NotImplementedError(f"seal mapper type 'brush' without the config keys {missing}: there is nothing to build a stroke from")
        mode = seal_config["attenuationMode"]
        if mode in ("ease-in", "ease-out"):
            raise NotImplementedError(f"attenuationMode {mode!r} (the reference leaves it unimplemented)")
        if mode not in _BRUSH_MODES:
            raise ValueError(f"attenuationMode {mode!r}")
        points = seal_config["raw"]
        if np.asarray(points[0]).ndim == 1:
            points = [points]
        if len(points) > self.MAX_STROKES:
            raise ValueError(f"a brush edit holds at most {self.MAX_STROKES} strokes, got {len(points)}")
        brush_type = seal_config["brushType"]
        if isinstance(brush_type, str):
            brush_type = [brush_type for _ in range(len(points))]
        if len(brush_type) != len(points):
            raise ValueError(f"{len(brush_type)} brush types for {len(points)} strokes")
        self.stroke_triangles, bounds, border_points = [], [], []
        for i in range(len(points)):
            current_points = np.asarray(points[i], dtype=np.float64).reshape(-1, 3)
            plane_point, normal = best_fit_plane(current_points)
            if "normal" in seal_config and normal @ np.array(seal_config["normal"], dtype=np.float64) < 0:
                normal = -normal
            normal_expand = normal * seal_config["brushPressure"]
            projected_points = project_points(torch.from_numpy(normal), torch.from_numpy(plane_point), torch.from_numpy(current_points))
            if brush_type[i] == "line":
                verts, _ = oriented_box(np.vstack([current_points + 2 * normal_expand, current_points - seal_config["brushDepth"] * normal_expand]))
                tri = verts[_BOX_FACES]
            elif brush_type[i] == "curve":
                verts, faces = fit_prism_mesh(projected_points.numpy(), normal_expand, [-seal_config["brushDepth"], 2], seal_config.get("simplifyVoxel", 16))
                if faces.shape[0] == 0:
                    raise ValueError(f"stroke {i}: the simplified mesh has no face left (simplifyVoxel {seal_config.get('simplifyVoxel', 16)})")
                tri = verts[faces]
            else:
                raise ValueError(f"brushType {brush_type[i]!r}")
            self.stroke_triangles.append(tri)
            bounds.append(_bounds(tri.reshape(-1, 3)))
            border_mask = mesh_surface_points_mask(torch.from_numpy(tri).to(self.dtype), projected_points.to(self.dtype))
            border_points.append(projected_points[border_mask])
        border_points = torch.cat(border_points)
        if border_points.shape[0] == 0:
            raise ValueError("no stroke point lies on the border of its mesh: there is no border to attenuate towards")
        self.map_triangles = torch.from_numpy(np.concatenate(self.stroke_triangles))
        self.map_test_dir = torch.from_numpy(normal_expand[None])
        self.map_data = {
            "force_fill_bound": np.array(bounds),
            "map_bound": np.array(bounds),
            "normal_expand": normal_expand,             # from the last stroke's plane, as is `center`
            "center": plane_point,
            "border_points": border_points,             # from all strokes
            "attenuation_distance": seal_config["attenuationDistance"],
            "attenuation_mode": mode,
        }
        self._read_color_options()
        if "imageConfig" in seal_config:               # :389-411
            image_conf = seal_config["imageConfig"]
            self.map_data["rgb_light_offset"] = seal_config.get("rgbLightOffset", 0)      # (the stamp's, also without an `rgb`)
            image, alpha = load_stamp(image_conf["path"], config_path)
            v_o, v_w, v_h = (np.asarray(image_conf[k], dtype=np.float64).reshape(3) for k in ("o", "w", "h"))
            self.map_data["image"] = image
            self.map_data["image_mask"] = alpha
            self.map_data["v_image_norm"] = best_fit_plane([v_o, v_w, v_h])[1]      # (either sign: project_points divides by n . n)
            self.map_data["v_image_o"] = v_o
            self.map_data["v_image_w"] = v_w
            self.map_data["v_image_h"] = v_h
        self.map_data_conversion(force=True)

    def _native_map_args(self, md, f32, cfl):
        device = self._native["tris"].device
        records = brush_triangle_records(self.map_triangles.detach().cpu().double().numpy(), md["normal_expand"])
        border = f32(md["border_points"].reshape(-1, 3))
        # the brush kernel's triangle records replace the 12-float ones of the box test
        return dict(tris=torch.from_numpy(records).to(device), normal_expand=cfl(f32(md["normal_expand"].reshape(3))), center=cfl(f32(md["center"].reshape(3))),
                    attenuation_distance=float(np.float32(md["attenuation_distance"])), mode=_BRUSH_MODES[self.map_data["attenuation_mode"]],
                    border=torch.from_numpy(border).to(device), n_border=int(border.shape[0]))

    native_kind = "SEAL_BRUSH"
    native_box_fields = (("test_dir", 3),)

    def _native_brush_record(self, a):
        import ctypes
        from sdn_backend import SdnSealBrush
        rec = SdnSealBrush()
        for k in range(3):
            rec.normal_expand[k], rec.center[k] = a["normal_expand"][k], a["center"][k]
        rec.attenuation_distance, rec.mode = a["attenuation_distance"], a["mode"]
        rec.border, rec.n_border = a["border"].data_ptr(), a["n_border"]
        rec.image = ctypes.addressof(a["image"]) if "image" in a else None      # the texture stamp (the caller keeps `a` alive)
        return rec

    def _native_map(self, lib, a, points, dirs, M, mask):
        """`sdn_seal_brush_map`: `dirs` are neither read nor written."""
        from sdn_backend import ptr, stream
        return "seal_brush_map", lib.sdn_seal_brush_map(
            ptr(points), None, M, a["bounds"], a["n_bounds"], ptr(a["tris"]), a["n_tris"], a["test_dir"], a["normal_expand"], a["center"],
            a["attenuation_distance"], a["mode"], ptr(a["border"]), a["n_border"], ptr(mask), stream())

    @torch.no_grad()
    def _map_to_origin_torch(self, points, dirs=None):
        """seal_utils.py:415-461, statement by statement (`linear` and `dry`)."""
        with torch.autocast(points.device.type if points.device.type != "cpu" else "cpu", enabled=False):
            self.map_data_conversion(points)
            md = self.map_data
            map_mask = self.map_mask(points)
            if not map_mask.any():
                return points, dirs, map_mask
            inner_points = points[map_mask]
            mode = md["attenuation_mode"]
            if mode == "linear":
                projected_points = project_points(md["normal_expand"], md["center"], inner_points)
                brush_border_distance = torch.cdist(projected_points, md["border_points"]).min(1)[0]
                points_mapped = inner_points - md["normal_expand"]
                distance_filter = md["attenuation_distance"] > brush_border_distance
                points_compensation = (torch.abs(md["attenuation_distance"] - brush_border_distance[distance_filter]) /
                                       md["attenuation_distance"])[None].T @ md["normal_expand"][None]
                points_mapped[distance_filter] += points_compensation
            elif mode == "dry":
                points_mapped = inner_points              # for a dry brush no space mapping is applied
            else:
                raise NotImplementedError(mode)
            points_copy = points.clone()
            points_copy[map_mask] = points_mapped
            return points_copy, dirs, map_mask


def get_seal_mapper(seal_config, config_path=None):
    """seal_utils.py:581-592 for the mapper types built here."""
    mapper = {"bbox": SealBBoxMapper, "anchor": SealAnchorMapper, "brush": SealBrushMapper}.get(seal_config.get("type"))
    if mapper is None:
        raise NotImplementedError(f"seal mapper type {seal_config.get('type')!r}")
    return mapper(seal_config, config_path)


@torch.no_grad()
def fill_bitfield(density_bitfield, bounds, grid_size=128, bound=1.0):
    """Marks every occupancy cell (cascade 0) whose centre lies in one of the axis-aligned `bounds` [B,2,3] as occupied, in every
    time slice of `density_bitfield` [T, grid_size^3 / 8] (uint8, Morton-ordered bits, bit i%8 of byte i/8) -- what the reference's
    trainer does with `force_fill_bound` before rendering an edit (`hack_bitfield`): the marcher must sample inside the box the
    content is moved INTO, where the unedited scene is empty.  In place; returns the number of cells marked."""
    import raymarching
    dev = density_bitfield.device
    b = torch.as_tensor(bounds, dtype=torch.float32, device=dev).reshape(-1, 2, 3)
    H = int(grid_size)
    c = (torch.arange(H, dtype=torch.float32, device=dev) + 0.5) * (2.0 * bound / H) - bound
    inside = torch.zeros(H, H, H, dtype=torch.bool, device=dev)
    for lo, hi in b:
        mx, my, mz = (c > lo[0]) & (c < hi[0]), (c > lo[1]) & (c < hi[1]), (c > lo[2]) & (c < hi[2])
        inside |= mx[:, None, None] & my[None, :, None] & mz[None, None, :]
    coords = torch.nonzero(inside).to(torch.int32).contiguous()
    if coords.shape[0] == 0:
        return 0
    idx = raymarching.morton3D(coords).long()
    bits = torch.zeros(H * H * H, dtype=torch.uint8, device=dev)
    bits[idx] = 1
    packed = (bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8, device=dev)).sum(1).to(torch.uint8)
    density_bitfield[:, : packed.shape[0]] |= packed[None]
    return int(coords.shape[0])
