"""NativeTrainStep in fp32 (a disabled GradScaler: the reference without `-O`) -> sdn_train_step_f32 (csrc/train.hip) against the
reference's own fp32 training fixture, the mirror network's eager fp32 autograd step and torch.optim.Adam."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_RAYS = 1024
_FLAT_DEF, _FLAT_COL = 128 * 80 + 6 * 128 * 128 + 16 * 128, 64 * 32 + 64 * 64 + 16 * 64


def _off():
    return torch.amp.GradScaler("cuda", enabled=False)


def _setup(seed=0, lr=1e-3):
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network import NeRFNetwork
    sc = build_scene(H=32, W=32, device="cuda", seed=seed)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    opt = torch.optim.Adam(model.get_params(10 * lr, lr), betas=(0.9, 0.99), eps=1e-15)
    target = torch.rand(1, N_RAYS, 3, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1, force_all_rays=False)
    model.mean_count = int(model.step_counter[0, 0].item()) + 256
    model.local_step = 0
    model.step_counter.zero_()
    return sc, model, opt, target


def _eager_backward(model, rays_o, rays_d, target, time, perturb=False):
    """The reference's fp32 step up to the gradients: op-by-op render without autocast, MSE, plain backward (the disabled scaler)."""
    model.zero_grad(set_to_none=True)
    out = model.render(rays_o[None], rays_d[None], time, staged=False, perturb=perturb, bg_color=1, force_all_rays=False, max_steps=1024)
    loss = torch.nn.MSELoss(reduction="none")(out["image"], target).mean(-1).mean()
    loss.backward()
    return out, loss


def _flat_to_layers(flat, in_cols, in_ld, width, n_hidden, out_rows):
    parts, at = [flat[:width * in_ld].view(width, in_ld)[:, :in_cols]], width * in_ld
    for _ in range(n_hidden - 1):
        parts.append(flat[at:at + width * width].view(width, width))
        at += width * width
    parts.append(flat[at:at + 16 * width].view(16, width)[:out_rows])
    return parts


def _grads(step, model):
    """name -> the fp32 gradient the step left in its workspace (unscaled: there is no loss scale)."""
    rows = model.encoder.embeddings.shape[0]
    g = {"encoder.embeddings": step.view("g_table", torch.float32, (rows, 2)).clone()}
    for i, w in enumerate(_flat_to_layers(step.view("g_deform", torch.float32, (_FLAT_DEF,)), 76, 80, 128, 7, 3)):
        g[f"deform_net.{i}.weight"] = w.clone()
    for i, w in enumerate(_flat_to_layers(step.view("g_color", torch.float32, (_FLAT_COL,)), 32, 32, 64, 2, 3)):
        g[f"color_net.{i}.weight"] = (torch.cat([w[:, :16], w[:, 17:]], dim=1) if i == 0 else w).clone()
    g["sigma_net.0.weight"] = step.view("g_sigma0", torch.float32, (64, 32)).clone()
    g["sigma_net.1.weight"] = step.view("g_sigma1", torch.float32, (16, 64)).clone()
    return g


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("case", ["budget", "overflow"])
def test_reference_training_fixture_at_fp32_distance(case):
    """The reference's own fp32 training branch (`caller_train.npz`) at the bars the op-by-op fp32 path meets
    (test_gpu_caller_fixtures.py::test_training_branch_reproduces_reference): exact sample counts, image 1e-4, loss 1e-4, every MLP
    gradient rtol 1e-3 / atol 1e-4 max (`budget` repeats `perturb` with M = its sample count), the hash-grid gradient per level, on
    the sampled rows and in its count of touched rows."""
    from caller_fixtures import fixture_model, fixture_scene, load
    from dnerf_amd.train_native import NativeTrainStep
    fx = load("train")
    model_bits = fixture_model("cuda")
    model = model_bits[0]
    sc = fixture_scene("cuda", model_bits=model_bits)
    sel = torch.from_numpy(fx["sel"]).long().cuda()
    ro, rd = sc.rays_o[sel].contiguous(), sc.rays_d[sel].contiguous()
    target = torch.from_numpy(fx["target"]).cuda()
    try:
        model.train()
        model.local_step, model.mean_count = 0, {"budget": int(fx["perturb_counter"][0]), "overflow": 2000}[case]
        model.step_counter.zero_()
        opt = torch.optim.Adam(model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
        step = NativeTrainStep(model, opt, _off(), ro.shape[0], "cuda", perturb=True)
        assert step.fp32
        step.noises = torch.from_numpy(fx["noises"]).cuda()
        loss = step(ro, rd, target, sc.time, grads_only=True)
        torch.cuda.synchronize()
        assert model.step_counter[0].cpu().numpy().tolist() == fx[f"{case}_counter"].tolist()
        np.testing.assert_allclose(step.image.cpu().numpy(), fx[f"{case}_image"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(float(loss), float(fx[f"{case}_loss"]), rtol=1e-4)
        grads = _grads(step, model)
        if case == "budget":
            for k, g in grads.items():
                if k == "encoder.embeddings":
                    continue
                ref = fx[f"perturb_grad_{k}"]
                np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=1e-3, atol=1e-4 * float(np.abs(ref).max()), err_msg=k)
        name = "perturb" if case == "budget" else "overflow"
        ge = grads["encoder.embeddings"].cpu().numpy()
        off = model.encoder.offsets.cpu().numpy()
        lv = np.stack([[ge[off[l]:off[l + 1]].astype(np.float64).sum(), np.abs(ge[off[l]:off[l + 1]]).astype(np.float64).sum(),
                        (ge[off[l]:off[l + 1]].astype(np.float64) ** 2).sum()] for l in range(16)])
        ref_lv = fx[f"{name}_grad_emb_levels"]
        np.testing.assert_allclose(lv[:, 1:], ref_lv[:, 1:], rtol=1e-4)
        np.testing.assert_allclose(lv[:, 0], ref_lv[:, 0], rtol=0, atol=1e-4 * ref_lv[:, 1].max())
        rows = fx[f"{name}_grad_emb_rows"]
        scale = float(np.abs(fx[f"{name}_grad_emb_vals"]).max())
        np.testing.assert_allclose(ge[rows], fx[f"{name}_grad_emb_vals"], rtol=1e-4, atol=1e-4 * scale)
        assert int((np.abs(ge).sum(1) != 0).sum()) == int(fx[f"{name}_grad_emb_nnz_rows"])
    finally:
        model.eval()
        model.mean_count, model.local_step = 0, 0


@pytest.mark.parametrize("time", [0.5, 0.0])
def test_gradients_match_the_eager_fp32_step(monkeypatch, time):
    """4096 rays of the bench scene's 800 x 800 camera, perturbed starts replayed through torch.rand: the eager fp32 autograd step
    against the native one.  Counts exact, loss 1e-5, image 1e-4, every gradient 1e-4 in relative L2 (the table gradient differs by
    the order of its fp32 atomics); at time == 0 the deformation MLP has no gradient and is not stepped."""
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network import NeRFNetwork
    from dnerf_amd.train_native import NativeTrainStep
    import raymarching.raymarching as rm_mod
    n_rays = 4096
    sc = build_scene(H=800, W=800, device="cuda", seed=0)
    idx = torch.randint(0, sc.rays_o.shape[0], (n_rays,), generator=torch.Generator(device="cpu").manual_seed(0)).cuda()
    rays_o, rays_d = sc.rays_o[idx].contiguous(), sc.rays_d[idx].contiguous()
    target = torch.rand(1, n_rays, 3, generator=torch.Generator(device="cpu").manual_seed(2)).cuda()
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    opt = torch.optim.Adam(model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    with torch.no_grad():
        for _ in range(2):
            model.render(rays_o[None], rays_d[None], sc.time, staged=False, perturb=True, bg_color=1, force_all_rays=False, max_steps=1024)
    model.mean_count = int(model.step_counter[:2, 0].sum().item() / 2)
    noises = torch.rand(n_rays, generator=torch.Generator(device="cpu").manual_seed(1)).cuda()
    tval = torch.tensor([[time]], dtype=torch.float32, device="cuda")
    model.local_step = 0
    model.step_counter.zero_()
    real_rand = torch.rand

    def fake_rand(*size, **kw):
        n = size[0] if len(size) == 1 and isinstance(size[0], int) else None
        return noises.clone() if n == n_rays else real_rand(*size, **kw)
    monkeypatch.setattr(rm_mod.torch, "rand", fake_rand)
    out, loss = _eager_backward(model, rays_o, rays_d, target, tval, perturb=True)
    monkeypatch.undo()
    ref_counter = model.step_counter[0].clone()
    ref = {k: v.grad.detach().clone() if v.grad is not None else None for k, v in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    model.local_step = 0
    step = NativeTrainStep(model, opt, _off(), n_rays, "cuda", perturb=True)
    step.noises = noises
    got = step(rays_o, rays_d, target, tval, grads_only=True)
    torch.cuda.synchronize()
    assert torch.equal(model.step_counter[0], ref_counter)
    np.testing.assert_allclose(float(got), float(loss.detach()), rtol=1e-5)
    assert float((step.image - out["image"][0]).abs().max()) < 1e-4
    grads = _grads(step, model)
    for k, want in ref.items():
        if want is None:
            assert time == 0.0 and k.startswith("deform_net"), k
            assert not grads[k].any(), k
            continue
        assert _rel(grads[k], want) < 1e-4, (k, _rel(grads[k], want))
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    step(rays_o, rays_d, target, tval)
    torch.cuda.synchronize()
    for k, v in model.named_parameters():
        assert torch.equal(v.detach(), before[k]) == (time == 0.0 and k.startswith("deform_net")), k
    assert step.adam_steps.tolist() == [1.0, 0.0 if time == 0.0 else 1.0]


def test_full_steps_are_torch_adam_on_the_native_gradients():
    """Three full steps against torch.optim.Adam(foreach=False) fed with the gradients of a grads-only call on the same state: parameters,
    moments and step counts within 1e-6; the EMA shadow is torch_ema's; the table-gradient accumulator is cleared."""
    from dnerf_amd.train_native import NativeTrainStep
    sc, model, opt, target = _setup()
    step = NativeTrainStep(model, opt, _off(), N_RAYS, "cuda", perturb=False, ema_decay=0.95, deterministic=True)
    ref_model = copy.deepcopy(model)
    ref_opt = torch.optim.Adam(ref_model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15, foreach=False)
    shadow = [p.detach().clone() for p in step.params]
    names = {id(p): n for n, p in model.named_parameters()}
    for it in range(3):
        step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True)
        grads = _grads(step, model)
        for k, p in ref_model.named_parameters():
            p.grad = grads[k].reshape(p.shape).clone()
        ref_opt.step()
        step(sc.rays_o, sc.rays_d, target, sc.time)          # deterministic: the same gradients, bit for bit
        torch.cuda.synchronize()
        d = min(0.95, (2 + it) / (11 + it))
        want = dict(ref_model.named_parameters())
        for i, p in enumerate(step.params):
            k = names[id(p)]
            q = want[k]
            assert float((p.detach() - q.detach()).abs().max()) <= 1e-6, (k, it)
            for key in ("exp_avg", "exp_avg_sq"):
                assert float((opt.state[p][key] - ref_opt.state[q][key]).abs().max()) <= 1e-6, (k, key, it)
            shadow[i] = shadow[i] - (1 - d) * (shadow[i] - p.detach())
            assert float((step.ema_shadow[i] - shadow[i]).abs().max()) <= 1e-6, (k, it)
    rows = model.encoder.embeddings.shape[0]
    assert float(step.view("g_table", torch.float32, (rows, 2)).abs().max()) == 0
    assert step.adam_steps.tolist() == [3.0, 3.0]
    step.sync_optimizer_state()
    assert all(float(opt.state[p]["step"]) == 3 == float(ref_opt.state[q]["step"]) for p, q in zip(model.parameters(), ref_model.parameters()))


def test_twenty_steps_track_the_eager_fp32_trajectory():
    """20 native fp32 steps against 20 eager fp32 steps (autograd, disabled scaler, torch Adam) from the same state on the same
    batch: the loss trajectories agree within 1e-3 relative at every step (worst case measured on an MI355X: 1.9e-7 to 4.9e-7)."""
    from dnerf_amd.train_native import NativeTrainStep
    sc, model, opt, target = _setup()
    ref_model = copy.deepcopy(model)
    ref_opt = torch.optim.Adam(ref_model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    ref_scaler = _off()
    step = NativeTrainStep(model, opt, None, N_RAYS, "cuda", perturb=False)
    a, b = [], []
    for _ in range(20):
        a.append(float(step(sc.rays_o, sc.rays_d, target, sc.time)))
        _, loss = _eager_backward(ref_model, sc.rays_o, sc.rays_d, target, sc.time)
        ref_scaler.step(ref_opt)
        ref_scaler.update()
        b.append(float(loss))
    worst = float(np.max(np.abs(np.array(a) - np.array(b)) / np.array(b)))
    print("worst relative loss difference over 20 steps:", worst)
    assert a[-1] < a[0] and b[-1] < b[0]
    assert worst < 1e-3, worst


def _state(model, opt):
    return {k: v.detach().clone() for k, v in model.named_parameters()} | {
        f"{k}.{s}": opt.state[p][s].clone() for k, p in model.named_parameters() if p in opt.state for s in ("exp_avg", "exp_avg_sq")}


def test_deterministic_runs_resume_and_prefetch_are_bit_identical():
    """deterministic=True: two runs from the same state, a run checkpointed after three steps and resumed in fresh objects, and a run
    that marches each next batch ahead (`prefetch`) all give the same losses and parameters bit for bit."""
    from dnerf_amd.network import NeRFNetwork
    from dnerf_amd.train_native import NativeTrainStep
    times = [0.5, 0.25, 0.0, 0.75, 0.5, 0.25]

    def run(ahead=False, stop_at=None):
        sc, model, opt, target = _setup()
        step = NativeTrainStep(model, opt, _off(), N_RAYS, "cuda", perturb=True, seed=5, deterministic=True)
        losses, saved = [], None
        for k, t in enumerate(times):
            losses.append(step(sc.rays_o, sc.rays_d, target, t).clone())
            if ahead and k + 1 < len(times):
                step.prefetch(sc.rays_o, sc.rays_d, times[k + 1])
            if k + 1 == stop_at:
                torch.cuda.synchronize()
                step.sync_optimizer_state()
                saved = {"model": copy.deepcopy(model.state_dict()), "opt": copy.deepcopy(opt.state_dict()), "mean_count": model.mean_count,
                         "local_step": model.local_step, "step_count": step.step_count}
        torch.cuda.synchronize()
        return [float(x) for x in losses], _state(model, opt), saved, (sc, target)

    la, A, saved, (sc, target) = run(stop_at=3)
    lb, B, _, _ = run()
    lc, C, _, _ = run(ahead=True)
    assert la == lb == lc
    assert [k for k in A if not torch.equal(A[k], B[k])] == [] and [k for k in A if not torch.equal(A[k], C[k])] == []
    model2 = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model2.load_state_dict(saved["model"])
    model2.mean_count, model2.local_step = saved["mean_count"], saved["local_step"]
    opt2 = torch.optim.Adam(model2.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    step2 = NativeTrainStep(model2, opt2, _off(), N_RAYS, "cuda", perturb=True, seed=5, deterministic=True)
    opt2.load_state_dict(saved["opt"])
    step2.refresh(optimizer_state=True)
    step2.step_count = saved["step_count"]
    l2 = [float(step2(sc.rays_o, sc.rays_d, target, t)) for t in times[3:]]
    torch.cuda.synchronize()
    assert l2 == la[3:]
    R = _state(model2, opt2)
    assert [k for k in A if not torch.equal(A[k], R[k])] == []


def test_frozen_deformation_student():
    """train_deform=False (SealD-NeRF's student): the deformation weights stay bit-unchanged, the optimizer stays serialisable; the table
    gradient equals a train_deform=True grads-only step's bit for bit (deterministic mode) and the sigma / colour gradients within 1e-6."""
    from dnerf_amd.seald_train import freeze_deformation
    from dnerf_amd.train_native import NativeTrainStep
    sc, model, opt_all, target = _setup()
    full = NativeTrainStep(model, opt_all, _off(), N_RAYS, "cuda", perturb=False, deterministic=True)
    full(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True)
    want = _grads(full, model)
    opt = torch.optim.Adam(freeze_deformation(model), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
    step = NativeTrainStep(model, opt, _off(), N_RAYS, "cuda", perturb=False, train_deform=False, deterministic=True)
    step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True)
    got = _grads(step, model)
    assert torch.equal(got["encoder.embeddings"], want["encoder.embeddings"])
    for k in got:
        if k.startswith("sigma_net") or k.startswith("color_net"):
            assert _rel(got[k], want[k]) <= 1e-6, k
    deform_before = [p.detach().clone() for p in model.deform_net.parameters()]
    sigma_before = model.sigma_net[0].weight.detach().clone()
    for _ in range(3):
        step(sc.rays_o, sc.rays_d, target, sc.time)
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(deform_before, model.deform_net.parameters()))
    assert not torch.equal(sigma_before, model.sigma_net[0].weight.detach())
    step.sync_optimizer_state()
    opt.state_dict()
    assert step.adam_steps.tolist() == [3.0, 0.0]


def _cold_copy(model):
    """copy.deepcopy(model) without the caches derived from the parameters (test_gpu_cache_coherence.py's helper)."""
    keys = ("_fused_cache", "_fused_cache32", "_fused_params", "_fused_time", "_sdn_cull_cache", "_density_updater")
    kept = {k: model.__dict__.pop(k) for k in keys if k in model.__dict__}
    try:
        return copy.deepcopy(model)
    finally:
        model.__dict__.update(kept)


def test_readers_see_the_new_weights_and_an_empty_batch_is_finite():
    """After fp32 native steps the fused fp32 dispatch (`fused_inference_f32`, warm caches) and DensityGridUpdater(fp32=True) equal a cold
    copy of the model bit for bit; a batch without a single sample gives the background loss, zero gradients and finite parameters."""
    from dnerf_amd.fused import DensityGridUpdater
    from dnerf_amd.train_native import NativeTrainStep
    sc, model, opt, target = _setup()
    x = (torch.rand(4096, 3, generator=torch.Generator().manual_seed(7)) * 1.6 - 0.8).cuda()
    d = torch.nn.functional.normalize(torch.randn(4096, 3, generator=torch.Generator().manual_seed(8)), dim=-1).cuda()

    def call(m):
        m.eval()
        m.fused_inference_f32 = True
        with torch.no_grad():
            assert m._fused_inference_ok(x, d) == 32
            return m(x, d, sc.time)

    before = call(model)
    assert model.__dict__.get("_fused_cache32") is not None
    model.use_native_density_update(fp32=True)           # update_extra_state through DensityGridUpdater(fp32=True)
    model.train()
    model.update_extra_state()                          # warm: the updater has packed the current weights
    step = NativeTrainStep(model, opt, _off(), N_RAYS, "cuda", perturb=False)
    for _ in range(2):
        step(sc.rays_o, sc.rays_d, target, sc.time)
    after = call(model)
    twin = _cold_copy(model)
    cold = call(twin)
    assert not torch.equal(cold[0], before[0])
    for k in range(3):
        assert torch.equal(after[k], cold[k]), k
    twin.use_native_density_update(fp32=True)
    twin._density_updater.seed = model._density_updater.seed
    assert isinstance(model._density_updater, DensityGridUpdater) and model._density_updater.fp32
    for m in (model, twin):
        m.train()
        torch.manual_seed(3)
        m.update_extra_state()
    torch.cuda.synchronize()
    assert torch.equal(model.density_grid, twin.density_grid) and torch.equal(model.density_bitfield, twin.density_bitfield)
    # empty occupancy: every pixel is the background
    model.train()
    with torch.no_grad():
        model.density_bitfield.zero_()
    step.refresh()
    got = step(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(got), float(((1 - target) ** 2).mean()), rtol=1e-5)
    assert all(not g.any() for g in _grads(step, model).values())
    step(sc.rays_o, sc.rays_d, target, sc.time)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_refusals_and_the_fp16_step_stays_selected_by_an_enabled_scaler():
    from dnerf_amd.train_native import NativeTrainStep
    import sdn_backend as B
    sc, model, opt, target = _setup()
    with pytest.raises(NotImplementedError):
        NativeTrainStep(model, opt, _off(), N_RAYS, "cuda", grad_sync=object())
    with pytest.raises(NotImplementedError):
        NativeTrainStep(model, opt, None, N_RAYS, "cuda", overlap_table_update=True)
    from dnerf_amd.seald_train import EditTrainStep
    with pytest.raises(NotImplementedError):
        EditTrainStep(model, model, None, opt, _off(), N_RAYS, "cuda", 0.5)
    # an enabled scaler keeps the fp16 step: same loss and gradients as a step built before the fp32 path existed would give
    on = NativeTrainStep(model, opt, torch.amp.GradScaler("cuda"), N_RAYS, "cuda", perturb=False)
    assert not on.fp32 and on._fn is B.lib.sdn_train_step_f16
    loss = on(sc.rays_o, sc.rays_d, target, sc.time, grads_only=True)
    rows = model.encoder.embeddings.shape[0]
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(on.view("g_table", torch.float16, (rows, 2)).float().abs().max()) > 0
    assert torch.equal(on.view("w_sigma0", torch.float16, (64, 32)), model.sigma_net[0].weight.detach().half())
