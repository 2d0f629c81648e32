"""Coherence of the derived copies the hot path keeps of model state, after the state was written by this package's own kernels.

Three caches are keyed on torch's version counter: the drop-in marcher's cull grid per occupancy slice (raymarching `_CULL_CACHE`, also
carrying the slice's fine bits), the grid encoder's QUAD fp16 copy of the table (gridencoder `_QUAD_TABLES`) and the packed weights /
fp16 table behind NeRFNetwork's fused dispatch (`_fused_cache`, `_fused_cache32`); the native loops keep cull grids per model on the
same key.  The counter only moves when torch writes a tensor, so every kernel that writes model state through a raw pointer --
`raymarching.packbits` into a given bitfield, the native density update, the native training step's optimizer pass -- has to move it
itself.  Each test here warms a cache, writes through such a kernel, checks that the write really changed the data, and then asks for
the bit-exact answer of a cold evaluation (the CPU oracle, or a deep copy of the model without its caches).

Section 6 covers the SealD hooks of the pipelined native loop: every loop context needs its own seal scratch (modify_rgb's sum, the
mapSource flag word), since the contexts share the mapper and run on their own streams.

Sections 7-10 cover the other writers of the parameters behind torch's back: the replayed optimizer of `GraphedTrainStep` (single
graph, data parallel, SealD edit training, the trainer's train / update / evaluate sequence), the collective of
`GradSync.broadcast_parameters`, and the table pass of `NativeTrainStep(overlap_table_update=True)`, which is still running on a second
stream when the step returns: the table's readers must order themselves behind it."""
import copy

import numpy as np
import pytest
import torch

import oracle as O  # noqa: E402  (tests are one of the three places allowed to use the oracle)

pytestmark = pytest.mark.gpu

N_RAYS = 1024
H_GRID = 128
# what NeRFNetwork / DeviceLoop derive and keep on the model object itself (a deep copy without them starts cold)
_CACHE_KEYS = ("_fused_cache", "_fused_cache32", "_fused_params", "_fused_time", "_sdn_cull_cache", "_density_updater")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cold_copy(model):
    """copy.deepcopy(model) with none of the derived state the original carries (`_density_updater` stays with the original)."""
    kept = {k: model.__dict__.pop(k) for k in _CACHE_KEYS if k in model.__dict__}
    try:
        twin = copy.deepcopy(model)
    finally:
        model.__dict__.update(kept)
    return twin


def _occ3(bits):
    """Morton bitfield slice [H^3/8] -> bool [H,H,H] in (ix, iy, iz) order."""
    from dnerf_amd import scene
    flat = np.unpackbits(bits, bitorder="little").astype(bool)
    return flat[scene._grid_cache(H_GRID)[1]].reshape(H_GRID, H_GRID, H_GRID)


def _rewritten_grid(bits):
    """A density grid [1, H^3] (Morton order, 1 occupied / 0 empty at threshold 0.5) that differs from the occupancy `bits` both ways:
    the half x < 0 is cleared, and a box is added whose cells all lie in 4^3 blocks -- the cull grid's cells (csrc: 32^3 mark bits) --
    that hold no old bit.  -> (grid, gained [H,H,H], lost [H,H,H])."""
    from dnerf_amd import scene
    old = _occ3(bits)
    new = old.copy()
    new[: H_GRID // 2] = False
    coarse = old.reshape(32, 4, 32, 4, 32, 4).any(axis=(1, 3, 5))
    empty_block = ~np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)
    c = scene._grid_cache(H_GRID)[0]
    X, Y, Z = c[:, None, None], c[None, :, None], c[None, None, :]
    box = (np.abs(X - 0.45) < 0.2) & (np.abs(Y + 0.35) < 0.25) & (np.abs(Z - 0.3) < 0.2)
    new |= box & empty_block
    grid = np.zeros(H_GRID ** 3, np.float32)
    grid[scene._grid_cache(H_GRID)[1]] = new.reshape(-1)
    return grid.reshape(1, -1), new & ~old, old & ~new


def _cells_of(xyzs, bound=1.0):
    """Cell indices (ix, iy, iz) of sample positions [M,3] in the bound-1 grid."""
    return np.clip(((xyzs + bound) / (2 * bound) * H_GRID).astype(np.int64), 0, H_GRID - 1)


@pytest.fixture(scope="module")
def cam():
    from dnerf_amd import scene
    ro, rd = scene.get_rays(scene.look_at_pose(), scene.intrinsics(32, 32), 32, 32)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = O.near_far_from_aabb(ro, rd, aabb, 0.2)
    return dict(ro=ro, rd=rd, bf=scene.jumpingjacks_occupancy(0.5), nears=nears, fars=fars, N=ro.shape[0])


# ---- 1. the drop-in marcher after packbits into the same slice -------------------------------------------------------------------
@pytest.mark.parametrize("n_step", [1, 8])
def test_march_rays_after_packbits_into_the_same_slice(cam, n_step):
    """March an aligned 128^3 slice (its cull grid is built and kept), rewrite the slice in place with `raymarching.packbits`, march
    again: the samples are the oracle's on the NEW bits, bit for bit; then the same with an all-empty grid (no sample at all)."""
    import raymarching
    from raymarching import raymarching as RM
    N = cam["N"]
    alive = np.arange(N, dtype=np.int32)[::-1].copy()[: N - 7]
    n_alive = alive.shape[0]
    rays_t = cam["nears"].copy()

    def march(bf):
        return raymarching.march_rays(n_alive, n_step, _dev(alive), _dev(rays_t), _dev(cam["ro"]), _dev(cam["rd"]), 1.0, bf, 1, 128,
                                      _dev(cam["nears"]), _dev(cam["fars"]), 128, False, 0.0, 1024)

    def oracle(bits):
        return O.march_rays(n_alive, n_step, alive, rays_t, cam["ro"], cam["rd"], 1.0, bits, 1, 128, cam["nears"], cam["fars"], align=128)

    def same(out, ref):
        for o, r, name in zip(out, ref, ("xyzs", "dirs", "deltas")):
            assert o.shape == r.shape, name
            assert np.array_equal(o.cpu().numpy().view(np.uint32), r.view(np.uint32)), name

    bf = _dev(cam["bf"])
    assert bf.data_ptr() % 8 == 0
    first = march(bf)
    assert RM._CULL_CACHE.get((bf.data_ptr(), bf.numel(), str(bf.device))) is not None     # the slice's cull grid is kept
    same(first, oracle(cam["bf"]))

    grid, gained, lost = _rewritten_grid(cam["bf"])
    new_bits = O.packbits(grid, 0.5)
    out = raymarching.packbits(_dev(grid), 0.5, bf)
    assert out.data_ptr() == bf.data_ptr() and np.array_equal(bf.cpu().numpy(), new_bits)
    assert gained.sum() > 1000 and lost.sum() > 1000
    ref = oracle(new_bits)
    # not vacuous: the new occupancy gives other samples, some of them in cells the old cull grid had marked empty
    assert not np.array_equal(ref[0], first[0].cpu().numpy())
    live = ref[2][:, 0] > 0
    ijk = _cells_of(ref[0][live])
    assert int(gained[ijk[:, 0], ijk[:, 1], ijk[:, 2]].sum()) > 10
    same(march(bf), ref)

    raymarching.packbits(torch.zeros(1, H_GRID ** 3, device="cuda"), 0.5, bf)
    none = march(bf)
    assert int(bf.count_nonzero()) == 0 and float(none[2].abs().max()) == 0.0
    same(none, oracle(np.zeros_like(cam["bf"])))


# ---- shared set-up of the training tests ----------------------------------------------------------------------------------------
def _trained_setup(seed=0, lr=1e-3):
    """A 32x32 scene's model in training mode with the optimizer, scaler and budget a NativeTrainStep needs
    (tests/test_gpu_train_native.py `_setup`)."""
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network import NeRFNetwork
    sc = build_scene(H=32, W=32, device="cuda", seed=seed)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    opt = torch.optim.Adam(model.get_params(10 * lr, lr), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    target = torch.rand(1, N_RAYS, 3, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1, force_all_rays=False)
    model.mean_count = int(model.step_counter[0, 0].item()) + 256
    model.local_step = 0
    model.step_counter.zero_()
    return sc, model, opt, scaler, target


def _native_steps(sc, model, opt, scaler, target, n=5):
    """n native training steps (forward + backward + Adam in csrc/train.hip); asserts that every trained parameter moved."""
    from dnerf_amd.train_native import NativeTrainStep
    was_training = model.training
    model.train()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    step = NativeTrainStep(model, opt, scaler, N_RAYS, "cuda", perturb=False)
    for _ in range(n):
        step(sc.rays_o, sc.rays_d, target, sc.time)
    torch.cuda.synchronize()
    for name in ("encoder.embeddings", "deform_net.0.weight", "sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight"):
        assert not torch.equal(before[name], dict(model.named_parameters())[name].detach()), name
    model.train(was_training)
    return step


def _probe(sc, n=4096, seed=6):
    from dnerf_amd.bench_scene import _probe_points
    x = torch.from_numpy(_probe_points(sc.bitfield, n, seed)).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda", generator=g), dim=1).contiguous()
    return x, d


# ---- 2. the native loop after a direct packbits -----------------------------------------------------------------------------------
def test_device_loop_after_a_direct_packbits():
    """A DeviceLoop that keeps its cull grids renders a slice; the slice is rewritten with `raymarching.packbits` (iter_density does not
    move); the next render equals the render of a cold copy of the model, bit for bit."""
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop
    import raymarching
    sc = build_scene(H=32, W=32, device="cuda", seed=0)
    model = sc.model
    N = sc.rays_o.shape[0]
    loop = DeviceLoop(model, FusedField(model, sc.time), N, "cuda", keep_cull_grids=True)
    a = loop.render(sc.rays_o, sc.rays_d, sc.time)
    assert sc.t_idx in model.__dict__["_sdn_cull_cache"]["grids"]
    image_a, n_a = a["image"].clone(), a["n_samples"]
    grid, gained, lost = _rewritten_grid(sc.bitfield)
    iters = model.iter_density
    raymarching.packbits(_dev(grid), 0.5, model.density_bitfield[sc.t_idx])
    assert model.iter_density == iters
    assert np.array_equal(model.density_bitfield[sc.t_idx].cpu().numpy(), O.packbits(grid, 0.5))
    b = loop.render(sc.rays_o, sc.rays_d, sc.time)
    twin = _cold_copy(model)
    c = DeviceLoop(twin, FusedField(twin, sc.time), N, "cuda", keep_cull_grids=True).render(sc.rays_o, sc.rays_d, sc.time)
    torch.cuda.synchronize()
    assert not torch.equal(c["image"], image_a)          # the rewrite changes the frame
    assert torch.equal(b["image"], c["image"]) and b["n_samples"] == c["n_samples"]
    assert torch.equal(torch.nan_to_num(b["depth"]), torch.nan_to_num(c["depth"]))      # (rays that miss the box: 0 / 0)


# ---- 3. NeRFNetwork's fused dispatch after native training steps --------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["f16", "f32"])
def test_fused_dispatch_after_native_training_steps(fp32):
    """`model(x, d, t)` through the fused dispatch (fp16 -O: eval + no_grad + fp16 autocast; fp32: `fused_inference_f32`, no autocast)
    with warm caches, then native training steps: the next call equals the same call on a cold copy of the model bit for bit, and that
    is within the dispatch's bars of the op-by-op network."""
    import contextlib
    sc, model, opt, scaler, target = _trained_setup()
    x, d = _probe(sc)
    model.eval()
    model.fused_inference_f32 = fp32
    amp = (lambda: contextlib.nullcontext()) if fp32 else (lambda: torch.autocast("cuda", dtype=torch.float16))

    def call(m):
        with torch.no_grad(), amp():
            assert m._fused_inference_ok(x, d) == (32 if fp32 else 16)
            return m(x, d, sc.time)

    before = call(model)
    call(model)
    assert model.__dict__.get("_fused_cache32" if fp32 else "_fused_cache") is not None
    _native_steps(sc, model, opt, scaler, target)
    model.eval()
    after = call(model)
    twin = _cold_copy(model)
    cold = call(twin)
    assert not torch.equal(cold[0], before[0]) and not torch.equal(cold[1], before[1])          # the steps change the network's output
    n_out = 3 if fp32 else 2
    for k in range(n_out):
        assert torch.equal(after[k], cold[k]), k
    _assert_within_dispatch_bars(twin, x, d, sc.time, cold, fp32)


def _assert_within_dispatch_bars(twin, x, d, t, cold, fp32):
    """The fused dispatch's answer `cold` of the cold copy `twin` is within the dispatch's bars of the op-by-op network.

    The training steps in front of this check sum the table gradient with atomics, so the trained weights, and with them this distance,
    differ from run to run.  Measured for `test_readers_after_graphed_training_steps[dispatch_f32]`, largest relative sigma error of a
    run (4096 points) over 24 runs: 2.1e-5 .. 2.6e-4, one run beyond the 2e-4 bar with one element (3.0e-4 has been seen as well); rgb
    1.2e-7 throughout.  The spread is that of the fp32 kernel against the hipBLASLt GEMMs on the weights a run happens to train; the
    bar stands."""
    import contextlib
    from dnerf_amd.network import NeRFNetwork
    twin.fused_inference = False
    with torch.no_grad(), (contextlib.nullcontext() if fp32 else torch.autocast("cuda", dtype=torch.float16)):
        s_ops, c_ops, _ = NeRFNetwork.forward(twin, x, d, t)
    s_ops, c_ops = s_ops.float(), c_ops.float()
    if fp32:
        # the bars of test_gpu_field_f32.py::test_forward_dispatches_to_the_fp32_kernel_when_asked
        np.testing.assert_allclose(cold[0].cpu().numpy(), s_ops.cpu().numpy(), rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(cold[1].cpu().numpy(), c_ops.cpu().numpy(), rtol=2e-4, atol=1e-6)
    else:
        # the -O bars of the fused kernel on the network's outputs (test_gpu_caller_fixtures.py::test_field_network_reproduces_reference_forward)
        rel = ((cold[0] - s_ops) / s_ops.abs().clamp_min(1e-3)).abs()
        assert float(rel.max()) < 5e-2 and float(rel.mean()) < 5e-3, (float(rel.max()), float(rel.mean()))
        assert float((cold[1] - c_ops).abs().max()) < 1e-2


# ---- 4. the op-by-op grid encoder's QUAD copy after native training steps -----------------------------------------------------------
def test_grid_encode_quad_copy_after_native_training_steps():
    """The op-by-op network (`fused_inference = False`) under fp16 autocast reads the QUAD copy of the table from the second call on;
    after native training steps the encoder's forward is the oracle's on the NEW fp16 table, bit for bit."""
    from gridencoder import grid as G
    sc, model, opt, scaler, target = _trained_setup()
    enc = model.encoder
    model.eval()
    model.fused_inference = False
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.uniform(-1, 1, (4000, 3)).astype(np.float32)).cuda()
    G._QUAD_TABLES.clear()

    def run():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return enc(x, bound=1)

    first = run()
    run()
    ent = [e for e in G._QUAD_TABLES.values() if e["ref"]() is enc.embeddings]
    assert len(ent) == 1 and ent[0]["quad"] is not None                    # the copy is built and in use
    table_before = enc.embeddings.detach().clone()
    _native_steps(sc, model, opt, scaler, target)
    assert not torch.equal(table_before.half(), enc.embeddings.detach().half())
    got = run()
    emb16 = enc.embeddings.detach().half().cpu().numpy()
    off = enc.offsets.cpu().numpy().astype(np.int32)
    xin = ((x + 1) / 2).cpu().numpy()
    ref, _ = O.grid_encode_forward(xin, emb16, off, float(enc.per_level_scale), enc.base_resolution, False, 1, False, 0)
    assert not np.array_equal(first.cpu().numpy().view(np.uint16), ref.view(np.uint16))
    assert np.array_equal(got.cpu().numpy().view(np.uint16), ref.view(np.uint16))
    again = run()                                                          # and the copy rebuilt from the new table
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))


# ---- 5. the reference trainer's sequence --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native_update", [False, True], ids=["mirror_update", "native_update"])
def test_train_update_evaluate_sequence(native_update, monkeypatch):
    """Evaluate (every cache warm), train natively, `update_extra_state` (a full update: the occupancy changes), evaluate again: image,
    depth and sample count equal the same render of a deep copy of the model taken at that point, bit for bit."""
    import raymarching
    sc, model, opt, scaler, target = _trained_setup()
    if native_update:
        model.use_native_density_update()
    counted = []
    march = raymarching.march_rays

    def counting_march(*args):
        out = march(*args)
        counted.append((out[2][:, 0] > 0).sum())
        return out

    monkeypatch.setattr(raymarching, "march_rays", counting_march)

    def evaluate(m):
        counted.clear()
        m.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out = m.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1)
        return out["image"].clone(), torch.nan_to_num(out["depth"]).clone(), int(sum(int(c) for c in counted))

    warm = evaluate(model)
    evaluate(model)
    bits_before = model.density_bitfield[sc.t_idx].clone()
    _native_steps(sc, model, opt, scaler, target)
    model.train()
    model.iter_density = 0                       # a full update: every cell of every slice is queried again
    with torch.autocast("cuda", dtype=torch.float16):
        model.update_extra_state()
    bits_after = model.density_bitfield[sc.t_idx]
    gained = int((bits_after & ~bits_before).count_nonzero())
    lost = int((bits_before & ~bits_after).count_nonzero())
    assert gained > 0 and lost > 0, (gained, lost)
    twin = _cold_copy(model)
    got = evaluate(model)
    want = evaluate(twin)
    assert not torch.equal(want[0], warm[0])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2], (got[2], want[2])


# ---- 6. SealD rgb tint + mapSource in the pipelined native loop ---------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4])
def test_pipelined_seald_rgb_tint_and_map_source(K):
    """caller_seald_rgb.npz's mapper (rgb tint: the mean brightness of each iteration's masked samples; mapSource: a flag word only
    ever raised to a growing tag) through PipelinedDeviceLoop with K contexts on K streams: every frame equals DeviceLoop.render with
    the same mapper bit for bit, and the K contexts' seal records point at K distinct scratch buffers."""
    from caller_fixtures import fill_bitfield_host, fixture_model, fixture_scene
    from test_caller_fixtures_cpu import SEAL_CONFIG_RGB_MOVE
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop, PipelinedDeviceLoop
    from dnerf_amd.seal_mapper import SealBBoxMapper
    model, bits = fixture_model("cuda")
    sc = fixture_scene("cuda", H=32, W=32, model_bits=(model, bits))
    mapper = SealBBoxMapper(SEAL_CONFIG_RGB_MOVE)
    model.density_bitfield.copy_(torch.from_numpy(fill_bitfield_host(bits, mapper.map_data["force_fill_bound"].cpu().numpy())))
    field = FusedField(model, sc.time)
    N = sc.rays_o.shape[0]
    plain = DeviceLoop(model, field, N, "cuda", T_thresh=1e-4).render(sc.rays_o, sc.rays_d, sc.time)["image"].clone()
    ref = DeviceLoop(model, field, N, "cuda", T_thresh=1e-4, mapper=mapper).render(sc.rays_o, sc.rays_d, sc.time)["image"].clone()
    torch.cuda.synchronize()
    assert int(((ref - plain).abs().max(1).values > 1e-3).sum()) > 20          # the edit shows in the frame
    pl = PipelinedDeviceLoop(model, field, N, "cuda", contexts=K, T_thresh=1e-4, mapper=mapper)
    n = 2 * K + 1
    outputs = [(torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda")) for _ in range(n)]
    outs, _ = pl.render_frames([sc.rays_o] * n, [sc.rays_d] * n, sc.time, outputs=outputs)
    torch.cuda.synchronize()
    bad = [f for f, (img, _) in enumerate(outs) if not torch.equal(img, ref)]
    scratch = {lp._seal[0].scratch for lp in pl.loops}
    assert len(scratch) == K and not bad, (len(scratch), bad)


# ---- shared readers of the tests below ------------------------------------------------------------------------------------------------
def _dispatch(m, x, d, t, fp32):
    """NeRFNetwork's fused dispatch (fp16 -O, or the fp32 kernel).  NeRFNetworkFF keeps NeRFNetwork's parameters and derived caches but
    its own forward has no dispatch; it is called as NeRFNetwork's here, on the parameters the graphed step trains."""
    import contextlib
    from dnerf_amd.network import NeRFNetwork
    m.eval()
    m.fused_inference_f32 = fp32
    with torch.no_grad(), (contextlib.nullcontext() if fp32 else torch.autocast("cuda", dtype=torch.float16)):
        assert m._fused_inference_ok(x, d) == (32 if fp32 else 16)
        return NeRFNetwork.forward(m, x, d, t)


def _encode(m, x):
    """The op-by-op grid encoder under -O eval: the QUAD copy of the table from the second call on."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        return m.encoder(x, bound=1)


def _quad_entry(m):
    from gridencoder import grid as G
    ent = [e for e in G._QUAD_TABLES.values() if e["ref"]() is m.encoder.embeddings]
    return ent[0] if len(ent) == 1 else None


def _oracle_encode(m, x):
    """The oracle's grid encoder forward on the model's current fp16 table."""
    enc = m.encoder
    emb16 = enc.embeddings.detach().half().cpu().numpy()
    off = enc.offsets.cpu().numpy().astype(np.int32)
    ref, _ = O.grid_encode_forward(((x + 1) / 2).cpu().numpy(), emb16, off, float(enc.per_level_scale), enc.base_resolution, False, 1,
                                   False, 0)
    return ref


def _eval_render(m, sc):
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = m.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1)
    return out["image"].clone(), torch.nan_to_num(out["depth"]).clone()


def _enc_points(n=4000, seed=9):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)).cuda()


_TRAINED = ("encoder.embeddings", "sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight")


def _snapshot(m):
    return {k: p.detach().clone() for k, p in m.named_parameters()}


def _assert_moved(m, before, names=_TRAINED):
    now = dict(m.named_parameters())
    for name in names:
        assert not torch.equal(before[name], now[name].detach()), name
    assert not torch.equal(before["encoder.embeddings"].half(), now["encoder.embeddings"].detach().half())   # the fp16 table too


# ---- 7. GraphedTrainStep: the replayed optimizer writes the parameters behind torch's back ---------------------------------------------
def _graphed_setup(seed=0):
    """tests/test_gpu_train_graph.py `_setup` with the learning rates of `_trained_setup`: an NeRFNetworkFF (the network the graph
    captures: no host branch on t) with the fused, capturable Adam."""
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network_ff import NeRFNetworkFF
    from dnerf_amd.train_graph import merged_param_groups
    sc = build_scene(H=32, W=32, device="cuda", seed=seed)
    model = NeRFNetworkFF(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    opt = torch.optim.Adam(merged_param_groups(model.get_params(1e-2, 1e-3)), betas=(0.9, 0.99), eps=1e-15, fused=True, capturable=True)
    scaler = torch.amp.GradScaler("cuda")
    target = torch.rand(1, N_RAYS, 3, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1, force_all_rays=False)
    model.mean_count = int(model.step_counter[0, 0].item()) + 256
    model.local_step = 0
    model.step_counter.zero_()
    return sc, model, opt, scaler, target


def _captured_step(sc, model, opt, scaler, target, **kw):
    """A GraphedTrainStep, captured.  The capture puts the parameters back with torch writes (their counters move): the caches are
    warmed after it, so that only the replays stand between the warm caches and the next read."""
    from dnerf_amd.train_graph import GraphedTrainStep
    step = GraphedTrainStep(model, opt, scaler, N_RAYS, "cuda", perturb=False, **kw)
    step.load(sc.rays_o, sc.rays_d, target, sc.time)
    step.capture()
    torch.cuda.synchronize()
    return step


def _replay(step, model, n=4):
    before = _snapshot(model)
    model.train()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    _assert_moved(model, before)


@pytest.mark.parametrize("reader", ["dispatch_f16", "dispatch_f32", "quad_copy", "render"])
def test_readers_after_graphed_training_steps(reader):
    """Warm a reader of the parameters, replay captured training steps (single graph: forward + backward + fused Adam), read again:
    the answer equals the same read of a cold copy bit for bit -- the fused dispatch's (and that is within its bars of the op-by-op
    network), the grid encoder's QUAD copy's (the oracle's forward on the new fp16 table), an -O eval render's."""
    sc, model, opt, scaler, target = _graphed_setup()
    step = _captured_step(sc, model, opt, scaler, target)
    x, d = _probe(sc)
    if reader.startswith("dispatch"):
        fp32 = reader == "dispatch_f32"
        before = _dispatch(model, x, d, sc.time, fp32)
        _dispatch(model, x, d, sc.time, fp32)
        assert model.__dict__.get("_fused_cache32" if fp32 else "_fused_cache") is not None
        _replay(step, model)
        after = _dispatch(model, x, d, sc.time, fp32)
        twin = _cold_copy(model)
        cold = _dispatch(twin, x, d, sc.time, fp32)
        assert not torch.equal(cold[0], before[0]) and not torch.equal(cold[1], before[1])
        for k in range(3 if fp32 else 2):
            assert torch.equal(after[k], cold[k]), k
        _assert_within_dispatch_bars(twin, x, d, sc.time, cold, fp32)
    elif reader == "quad_copy":
        xe = _enc_points()
        first = _encode(model, xe)
        _encode(model, xe)
        ent = _quad_entry(model)
        assert ent is not None and ent["quad"] is not None
        _replay(step, model)
        got, again = _encode(model, xe), _encode(model, xe)          # the plain kernel's read, then the copy's
        ref = _oracle_encode(model, xe)
        assert not np.array_equal(first.cpu().numpy().view(np.uint16), ref.view(np.uint16))
        assert np.array_equal(got.cpu().numpy().view(np.uint16), ref.view(np.uint16))
        assert np.array_equal(again.cpu().numpy().view(np.uint16), ref.view(np.uint16))
    else:
        warm = _eval_render(model, sc)
        _eval_render(model, sc)
        ent = _quad_entry(model)
        assert ent is not None and ent["quad"] is not None
        _replay(step, model)
        got = _eval_render(model, sc)
        want = _eval_render(_cold_copy(model), sc)
        assert not torch.equal(want[0], warm[0])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_train_update_evaluate_sequence_with_graphed_steps():
    """The reference trainer's sequence with the graphed step: evaluate (every cache warm), replay training steps, `update_extra_state`
    (a full update, whose density queries read the table through the grid encoder), evaluate again: image and depth equal the same
    render of a cold copy of the model taken at that point, bit for bit."""
    sc, model, opt, scaler, target = _graphed_setup()
    step = _captured_step(sc, model, opt, scaler, target)
    warm = _eval_render(model, sc)
    _eval_render(model, sc)
    assert _quad_entry(model) is not None and _quad_entry(model)["quad"] is not None
    bits_before = model.density_bitfield[sc.t_idx].clone()
    _replay(step, model)
    model.train()
    model.iter_density = 0
    with torch.autocast("cuda", dtype=torch.float16):
        model.update_extra_state()
    bits_after = model.density_bitfield[sc.t_idx]
    assert int((bits_after ^ bits_before).count_nonzero()) > 0           # the occupancy changes
    twin = _cold_copy(model)
    got = _eval_render(model, sc)
    want = _eval_render(twin, sc)
    assert not torch.equal(want[0], warm[0])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, tmp_path, world=2):
    """`fn(rank, world, port, out_dir)` on `world` gloo ranks, all on this one GPU (test_gpu_ffmlp_parity.py `_dp_rank`)."""
    import json
    import torch.multiprocessing as mp
    mp.spawn(fn, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    return [json.load(open(tmp_path / f"rank_{r}.json")) for r in range(world)]


def _rank_init(rank, world, port):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)   # one-GPU rehearsal: both ranks on cuda:0, collectives through the host
    return dist


def _same_on_every_rank(dist, t):
    t = t.detach().contiguous().cpu()
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    return all(torch.equal(parts[0], q) for q in parts)


def _graphed_dp_rank(rank, world, port, out_dir):
    import json
    import os
    dist = _rank_init(rank, world, port)
    try:
        from dnerf_amd.dist import GradSync
        sc, model, opt, scaler, target = _graphed_setup()
        target = torch.rand(1, N_RAYS, 3, generator=torch.Generator().manual_seed(50 + rank)).cuda()     # own batch per rank
        sync = GradSync(model)
        sync.broadcast_parameters()
        step = _captured_step(sc, model, opt, scaler, target, warmup=1, grad_sync=sync)
        x, d = _probe(sc)
        before = _dispatch(model, x, d, sc.time, False)
        _dispatch(model, x, d, sc.time, False)
        res = {"warm": model.__dict__.get("_fused_cache") is not None, "two_graphs": step.graph_opt is not None}
        _replay(step, model)
        after = _dispatch(model, x, d, sc.time, False)
        cold = _dispatch(_cold_copy(model), x, d, sc.time, False)
        res["changed"] = not torch.equal(cold[0], before[0]) and not torch.equal(cold[1], before[1])
        res["equals_cold"] = [torch.equal(after[k], cold[k]) for k in range(2)]
        res["same_across_ranks"] = [_same_on_every_rank(dist, after[k]) for k in range(2)]
        with open(os.path.join(out_dir, f"rank_{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def test_fused_dispatch_after_data_parallel_graphed_steps(tmp_path):
    """Two ranks train through the two-graph step (forward + backward | gradient all-reduce | optimizer graph), each with a warm fused
    dispatch: afterwards each rank's dispatch equals its cold copy's bit for bit, and the ranks' answers are identical."""
    for r, res in enumerate(_spawn(_graphed_dp_rank, tmp_path)):
        assert res["warm"] and res["two_graphs"] and res["changed"], (r, res)
        assert all(res["equals_cold"]) and all(res["same_across_ranks"]), (r, res)


# ---- 8. GradSync.broadcast_parameters writes every replica's parameters through a collective ------------------------------------------
def _broadcast_rank(rank, world, port, out_dir):
    import json
    import os
    dist = _rank_init(rank, world, port)
    try:
        from dnerf_amd.bench_scene import build_scene
        from dnerf_amd.dist import GradSync
        sc = build_scene(H=32, W=32, device="cuda", seed=0)
        model = sc.model.eval()
        x, d = _probe(sc)
        xe = _enc_points()
        if rank == 1:                                   # this replica's weights differ from rank 0's
            with torch.no_grad():
                model.encoder.embeddings.mul_(1.5)
                for layers in (model.deform_net, model.sigma_net, model.color_net):
                    for l in layers:
                        l.weight.mul_(1.05)

        def answers():
            return [*_dispatch(model, x, d, sc.time, False)[:2], *_dispatch(model, x, d, sc.time, True), _encode(model, xe)]

        answers()
        before = answers()                               # every cache warm (the QUAD copy from the second call on)
        res = {"warm": [model.__dict__.get(k) is not None for k in ("_fused_cache", "_fused_cache32")] + [_quad_entry(model)["quad"] is not None]}
        res["differed"] = [not _same_on_every_rank(dist, a) for a in before]
        GradSync(model).broadcast_parameters()
        after, again = answers(), answers()              # (the encoder: the plain kernel's read, then the rebuilt copy's)
        res["same"] = [_same_on_every_rank(dist, a) for a in after + again]
        with open(os.path.join(out_dir, f"rank_{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def test_readers_after_broadcast_parameters(tmp_path):
    """Rank 1 changes its weights and warms its fused dispatch (f16, f32) and QUAD copy; after `broadcast_parameters()` its answers
    equal rank 0's bit for bit (outputs, twice: f16 sigma, rgb; f32 sigma, rgb, deform; the encoder's)."""
    for r, res in enumerate(_spawn(_broadcast_rank, tmp_path)):
        assert all(res["warm"]) and all(res["differed"]), (r, res)
        assert all(res["same"]), (r, res)


# ---- 9. SealD-NeRF edit training: the student's graphed (or native) steps -------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True], ids=["graphed", "native"])
def test_seald_student_render_after_edit_training(native):
    """EditTrainStep.run trains an NeRFNetworkFF student on the teacher's mapped render; the student's -O eval render, warm before the
    epoch, equals its cold copy's after it bit for bit (native=True: the native step, which moves the counters itself)."""
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network_ff import NeRFNetworkFF
    from dnerf_amd.seald_train import EditTrainStep, freeze_deformation
    from dnerf_amd import seal_mapper as SM
    sc = build_scene(H=32, W=32, device="cuda", seed=0)
    half, centre = 0.12, (0.0, 0.47, 0.0)
    raw = [[centre[0] + sx * half, centre[1] + sy * half, centre[2] + sz * half] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]
    T = np.eye(4)
    T[0, 3] = 0.35
    mapper = SM.get_seal_mapper({"type": "bbox", "raw": raw, "transform": T.tolist(), "scale": [1.0, 1.0, 1.0], "boundType": "to", "hsv": [0.3, 0.0, 0.0]})
    SM.fill_bitfield(sc.model.density_bitfield, mapper.map_data["force_fill_bound"].cpu().numpy(), sc.model.grid_size, sc.model.bound)
    n_rays = sc.rays_o.shape[0]
    student = NeRFNetworkFF(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    student.load_state_dict(sc.model.state_dict())
    params = freeze_deformation(student)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        student.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1, force_all_rays=False, max_steps=1024)
    student.mean_count = int(student.step_counter[0, 0].item()) + 512
    student.local_step = 0
    opt = torch.optim.Adam(params, lr=2e-3, betas=(0.9, 0.99), eps=1e-15, fused=True, capturable=True)
    edit = EditTrainStep(sc.model, student, mapper, opt, torch.amp.GradScaler("cuda"), n_rays, "cuda", sc.time, native=native,
                         perturb=False, warmup=1)
    batch = (sc.rays_o, sc.rays_d, sc.time)
    assert edit.run([batch] * 2) == 2                  # (the graphed step is captured here: its restore writes are torch's)
    torch.cuda.synchronize()
    warm = _eval_render(student, sc)
    _eval_render(student, sc)
    assert _quad_entry(student) is not None and _quad_entry(student)["quad"] is not None
    before = _snapshot(student)
    student.train()
    assert edit.run([batch] * 5) == 5
    torch.cuda.synchronize()
    _assert_moved(student, before)
    got = _eval_render(student, sc)
    want = _eval_render(_cold_copy(student), sc)
    assert not torch.equal(want[0], warm[0])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 10. NativeTrainStep(overlap_table_update=True): the table's Adam pass still runs on the second stream ----------------------------
_SIDE_DELAY_CYCLES = 1_000_000_000   # torch.cuda._sleep: ~0.4 s at the shader clock, longer than any reader's host work -- the table pass queues behind it


@pytest.mark.parametrize("reader", ["dispatch_f16", "dispatch_f32", "quad_copy"])
def test_readers_right_after_overlapped_native_steps(reader):
    """Warm a reader of the table, take native steps whose table pass runs on the step's second stream -- the last one queued behind a
    delay there, so the race is decided the same way every run -- and read straight away (no flush(), no synchronize): the answer
    equals the same read of a cold copy taken after a synchronize, bit for bit."""
    from dnerf_amd.train_native import NativeTrainStep
    sc, model, opt, scaler, target = _trained_setup()
    step = NativeTrainStep(model, opt, scaler, N_RAYS, "cuda", perturb=False, overlap_table_update=True)
    step(sc.rays_o, sc.rays_d, target, sc.time)        # builds the record and the second stream's events
    torch.cuda.synchronize()
    x, d = _probe(sc)
    xe = _enc_points()
    fp32 = reader == "dispatch_f32"
    if reader == "quad_copy":
        model.eval()
        read = lambda m: (_encode(m, xe), _encode(m, xe))             # noqa: E731  (the plain kernel's read, then the copy's)
    else:
        read = lambda m: _dispatch(m, x, d, sc.time, fp32)            # noqa: E731
    read(model)
    before = read(model)
    if reader == "quad_copy":
        assert _quad_entry(model)["quad"] is not None
    else:
        assert model.__dict__.get("_fused_cache32" if fp32 else "_fused_cache") is not None
    snap = _snapshot(model)
    model.train()
    step(sc.rays_o, sc.rays_d, target, sc.time)
    with torch.cuda.stream(step._table_side[0]):
        torch.cuda._sleep(_SIDE_DELAY_CYCLES)
    step(sc.rays_o, sc.rays_d, target, sc.time)
    got = read(model)
    torch.cuda.synchronize()
    _assert_moved(model, snap)
    if reader == "quad_copy":
        ref = _oracle_encode(model, xe)
        assert not np.array_equal(before[1].cpu().numpy().view(np.uint16), ref.view(np.uint16))
        assert np.array_equal(got[0].cpu().numpy().view(np.uint16), ref.view(np.uint16))
        assert np.array_equal(got[1].cpu().numpy().view(np.uint16), ref.view(np.uint16))
        return
    twin = _cold_copy(model)
    cold = read(twin)
    assert not torch.equal(cold[0], before[0]) and not torch.equal(cold[1], before[1])
    for k in range(3 if fp32 else 2):
        assert torch.equal(got[k], cold[k]), k
    _assert_within_dispatch_bars(twin, x, d, sc.time, cold, fp32)
