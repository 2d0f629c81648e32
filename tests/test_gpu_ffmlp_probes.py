"""The fused MLP operator (csrc/ffmlp.hip, csrc/ffmlp_kernels.h) pinned element by element, through the `ffmlp` package and the C ABI,
on the cases of tests/ffmlp_probe_support.py (validated without a GPU by tests/test_ffmlp_probes_cpu.py).

Exact cases: inference outputs, training-forward outputs (and `torch.equal` of the two), the whole forward_buffer, the whole
backward_buffer (C ABI call with the test's own buffers), grad_inputs and every element of grad_weights are compared BIT FOR BIT with
float64 of the same integers rounded once; no element is left out; 64 guard rows behind every output buffer keep their -7.  The batches
come from the launch rule restated in the support module and the CU count of the device, so every case names the kernel variant it ran
(-s shows it) and the coverage test asserts the union over both epilogues (ReLU; `none` for the run-time-dispatch instantiation) and the
three modes.  Not asserted, because no batch reaches it at ANY CU count (ffmlp_probe_support.unreachable): the SW-wave latency branch
of `launch_width` (widths 64 and 128).  The ReLU case of the dispatch instantiation is unreachable too: `launch_fused` routes ReLU to its
own instantiation.

Non-finite values follow the reference's formulas (x * (x > 0), g * (f > 0)); a NaN matches any NaN, everything else is bit for bit.

Activations, one element at a time over every finite fp16 value (identity first layer): ReLU / none bit for bit; the others against the
float64 activation with the bar of ffmlp_probe_support.forward_bar / backward_bar; infinite and zero sets equal to the reference's
float formulas (squareplus: the kernel's cancellation-free form of it).  Measured on an MI355X (-s prints the figures): MEASURED below.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ffmlp_probe_support as P  # noqa: E402

MEASURED = """
forward, worst distance as a share of its bar (widths 16 and 32 alike): exponential 0.998 (x = 0.0227), sigmoid 0.998 (x = 0.0107),
  squareplus 0.997 (x = 2.04), softplus 0.996 (x = 0.340), sine for |x| < 100 0.962 (x = 81.9).  Sets: exponential 12 916 inf, 12 202
  zero, 891 subnormal; softplus 13 200 inf (x > 8.87: the reference's float formula overflows there too), 15 869 zero; squareplus none.
backward, worst over g in {1, -1, 2^-14, 1000}: exponential 1.000 (ties of the one product rounding), sigmoid 0.989, squareplus 0.990,
  softplus 0.987.
sine, |x| >= 100, worst absolute error per binade [2^6, 2^7) .. [2^15, 2^16): 2.5e-4, 2.6e-4, 2.6e-4, 2.7e-4, 3.3e-4, 4.4e-4, 7.3e-4,
  1.4e-3, 2.7e-3, 5.3e-3 (recorded, not a bar; finite and |y| <= 1 everywhere).
Found by this sweep and fixed: squareplus as the reference writes it, 0.5 (s + sqrt(s^2 + 4)) with s = 10 x, cancels to 0 or one float
quantum of |s| for s << -1 (x = -423.5: 0 or 2.4e-5 where the function is 2.36e-5; zero for every x < -820); the kernel now evaluates
2 / (sqrt(s^2 + 4) - s) for s < 0.  Found in the test's own derivation: the hardware exp's 1e-6 is relative to exp(-10 f), not to
1 - exp(-10 f) (softplus backward, f near 0).
"""
GUARD = 64
NAMES = [s["name"] for s in P.SPECS]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _guarded(n_elems, guard_elems):
    return torch.full((n_elems + guard_elems,), -7.0, dtype=torch.float16, device="cuda")


def _abi(s, c):
    """inference, training forward and backward through the C ABI on guarded buffers -> numpy results + guard verdicts."""
    import sdn_backend as sb
    lib = sb.lib
    B, W, L, in_dim, act = s["B"], s["W"], s["L"], s["in_dim"], P.ACT[s["act"]]
    x, w, g = (torch.from_numpy(c[k]).cuda().contiguous() for k in ("x", "w", "g"))
    nbytes = int(lib.sdn_ffmlp_scratch_bytes(B, in_dim, 16, W, L))
    assert nbytes > 0
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = sb.stream()
    out_i, out_t = _guarded(B * 16, GUARD * 16), _guarded(B * 16, GUARD * 16)
    fwd, bwd = _guarded(L * B * W, GUARD * W), _guarded(L * B * W, GUARD * W)
    gi, gw = _guarded(B * in_dim, GUARD * in_dim), _guarded(w.numel(), GUARD)
    sb.check(lib.sdn_ffmlp_inference(x.data_ptr(), w.data_ptr(), B, in_dim, 16, W, L, act, 6, out_i.data_ptr(), work.data_ptr(), st), "inference")
    sb.check(lib.sdn_ffmlp_forward(x.data_ptr(), w.data_ptr(), B, in_dim, 16, W, L, act, 6, fwd.data_ptr(), out_t.data_ptr(), work.data_ptr(), st), "forward")
    sb.check(lib.sdn_ffmlp_backward(g.data_ptr(), x.data_ptr(), w.data_ptr(), fwd.data_ptr(), B, in_dim, 16, W, L, act, 6, int(s["dx"]), bwd.data_ptr(),
                                    gi.data_ptr() if s["dx"] else None, gw.data_ptr(), work.data_ptr(), st), "backward")
    torch.cuda.synchronize()
    sizes = dict(out_i=B * 16, out_t=B * 16, fwd=L * B * W, bwd=L * B * W, gi=B * in_dim if s["dx"] else 0, gw=w.numel())
    bufs = dict(out_i=out_i, out_t=out_t, fwd=fwd, bwd=bwd, gi=gi, gw=gw)
    guards = {k: bool((bufs[k][sizes[k]:] == -7).all()) for k in bufs}
    r = {k: bufs[k][:sizes[k]].cpu().numpy() for k in bufs}
    return dict(out=r["out_t"].reshape(B, 16), out_inf=r["out_i"].reshape(B, 16), fwd=r["fwd"].reshape(L, B, W), bwd=r["bwd"].reshape(L, B, W),
                gi=r["gi"].reshape(B, in_dim) if s["dx"] else None, gw=r["gw"]), guards


def _package(s, c):
    """The same through ffmlp.ffmlp_forward and autograd."""
    import ffmlp
    act = P.ACT[s["act"]]
    xd = torch.from_numpy(c["x"]).cuda().requires_grad_(s["dx"])
    wd = torch.from_numpy(c["w"]).cuda()
    out_inf = ffmlp.ffmlp_forward(xd.detach(), wd, s["in_dim"], 16, s["W"], s["L"], act, 6, True, False)
    wg = wd.clone().requires_grad_(True)
    out = ffmlp.ffmlp_forward(xd, wg, s["in_dim"], 16, s["W"], s["L"], act, 6, False, s["dx"])
    same = torch.equal(out, out_inf) if not torch.isnan(out_inf).any() else None
    fwd = out.grad_fn.saved_tensors[3]
    out.backward(torch.from_numpy(c["g"]).cuda())
    return dict(out=out.detach().cpu().numpy(), out_inf=out_inf.cpu().numpy(), fwd=fwd.cpu().numpy(), gi=xd.grad.cpu().numpy() if s["dx"] else None,
                gw=wg.grad.cpu().numpy()), same


def _first_difference(got, want):
    d = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
    return f"{d.shape[0]} of {got.size} elements differ, first at {d[0].tolist()}: got {got[tuple(d[0])]} want {want[tuple(d[0])]}"


def _compare(s, c, ref, equal):
    abi, guards = _abi(s, c)
    pkg, same = _package(s, c)
    assert all(guards.values()), (s["name"], guards)
    assert same in (True, None), "training-forward outputs differ from inference outputs"
    for k in ("out", "out_inf", "fwd", "bwd", "gi", "gw"):
        want = ref["out" if k == "out_inf" else k]
        if want is None:
            continue
        assert equal(abi[k], want), (s["name"], "C ABI", k, _first_difference(abi[k], want))
        if k in pkg:
            assert equal(pkg[k], want), (s["name"], "package", k, _first_difference(pkg[k], want))


@pytest.mark.parametrize("name", NAMES)
def test_exact_case_bit_for_bit(name):
    s = P.resolve(P.SPEC_BY_NAME[name], _cus())
    c = P.make_case(s)
    ref = P.reference(s, c)
    assert ref["cert"] < 2.0 ** 24 and P.live_rows_reach_every_tile(s, c)
    print(f"[ffmlp-probe] {P.describe(s)}")
    _compare(s, c, ref, P.same_bits)


def test_cases_cover_every_reachable_launch_variant():
    cus = _cus()
    for spec in P.SPECS:
        print(f"[ffmlp-probe] {P.describe(P.resolve(spec, cus))}")
    print(f"[ffmlp-probe] {cus} CUs; compiled but unreachable here (and at any CU count): {P.unreachable(cus)}")
    missing = P.required() - P.coverage(cus)
    assert not missing, sorted(missing)


def test_seventeen_hidden_layers_are_refused_before_anything_is_written():
    """L = 17 would need 18 weight-gradient jobs: SDN_E_UNSUPPORTED, and neither backward_buffer, grad_inputs nor grad_weights is touched."""
    import sdn_backend as sb
    B, W, L, in_dim = 200, 64, 17, 32
    n_w = W * (in_dim + (L - 1) * W + 16)
    x = torch.ones(B, in_dim, dtype=torch.float16, device="cuda")
    w, g = torch.ones(n_w, dtype=torch.float16, device="cuda"), torch.ones(B, 16, dtype=torch.float16, device="cuda")
    fwd = torch.ones(L * B * W, dtype=torch.float16, device="cuda")
    work = torch.empty(int(sb.lib.sdn_ffmlp_scratch_bytes(B, in_dim, 16, W, L)), dtype=torch.uint8, device="cuda")
    bwd, gi, gw = _guarded(L * B * W, 0), _guarded(B * in_dim, 0), _guarded(n_w, 0)
    for act in (0, 6):
        rc = sb.lib.sdn_ffmlp_backward(g.data_ptr(), x.data_ptr(), w.data_ptr(), fwd.data_ptr(), B, in_dim, 16, W, L, act, 6, 1, bwd.data_ptr(),
                                       gi.data_ptr(), gw.data_ptr(), work.data_ptr(), sb.stream())
        torch.cuda.synchronize()
        assert rc == P.SDN_E_UNSUPPORTED
        assert bool((bwd == -7).all()) and bool((gi == -7).all()) and bool((gw == -7).all())


@pytest.mark.parametrize("name", P.NONFINITE)
def test_non_finite_values_follow_the_reference_formulas(name):
    s = P.resolve(P.SPEC_BY_NAME[name], _cus())
    c = P.make_nonfinite_case(s)
    ref = P.reference(s, c)
    assert ref["cert"] < 2.0 ** 24
    print(f"[ffmlp-probe] {P.describe(s)} | NaN share: fwd {np.isnan(ref['fwd']).mean():.3f} bwd {np.isnan(ref['bwd']).mean():.3f} gw {np.isnan(ref['gw']).mean():.3f}")
    _compare(s, c, ref, P.same_bits_or_nan)


# ---- activations, one element at a time -----------------------------------------------------------------------------------------------
def _sweep_forward(act, W):
    """forward_buffer[0] = act(x) for every finite fp16 x: identity first layer, zero layers behind it."""
    import ffmlp
    x = P.all_finite_halves().reshape(-1, W)
    w = np.concatenate([np.eye(W).reshape(-1), np.zeros(W * W + 16 * W)]).astype(np.float16)
    wg = torch.from_numpy(w).cuda().requires_grad_(True)
    out = ffmlp.ffmlp_forward(torch.from_numpy(x).cuda(), wg, W, 16, W, 2, P.ACT[act], 6, False, False)
    return x, out.grad_fn.saved_tensors[3][0].cpu().numpy()


def _sweep_backward(act, g):
    """backward_buffer[0] = g * act'(f) for every finite fp16 f: identity output layer (width 16), the test's own forward_buffer."""
    import sdn_backend as sb
    W, L = 16, 2
    f = P.all_finite_halves()
    B = f.shape[0]
    w = torch.from_numpy(np.concatenate([np.zeros(2 * W * W), np.eye(W).reshape(-1)]).astype(np.float16)).cuda()
    fwd = torch.from_numpy(np.stack([np.zeros_like(f), f])).cuda().contiguous()
    grad = torch.full((B, 16), float(g), dtype=torch.float16, device="cuda")
    x = torch.zeros(B, W, dtype=torch.float16, device="cuda")
    bwd, gw = torch.empty(L, B, W, dtype=torch.float16, device="cuda"), torch.empty_like(w)
    work = torch.empty(int(sb.lib.sdn_ffmlp_scratch_bytes(B, W, 16, W, L)), dtype=torch.uint8, device="cuda")
    rc = sb.lib.sdn_ffmlp_backward(grad.data_ptr(), x.data_ptr(), w.data_ptr(), fwd.data_ptr(), B, W, 16, W, L, P.ACT[act], 6, 0, bwd.data_ptr(), None,
                                   gw.data_ptr(), work.data_ptr(), sb.stream())
    torch.cuda.synchronize()
    return rc, f, bwd[0].cpu().numpy()


@pytest.mark.parametrize("W", [16, 32])
def test_relu_and_none_over_every_finite_half_bit_for_bit(W):
    for act in ("relu", "none"):
        x, y = _sweep_forward(act, W)
        z = (x.astype(np.float64) + 0.0).astype(np.float16)      # the layer output of x = -0 is +0: its sum starts from +0
        want = P.relu_forward(z) if act == "relu" else z
        assert P.same_bits(y, want), (act, _first_difference(y, want))
    if W == 16:
        for act in ("relu", "none"):
            for g in (1.0, -1.0, 2.0 ** -14, 1000.0):
                rc, f, d = _sweep_backward(act, g)
                gg = np.full_like(f, g)
                want = P.relu_backward(gg, f) if act == "relu" else gg
                assert rc == 0 and P.same_bits(d, want), (act, g, _first_difference(d, want))


def _worst(err, bar, x):
    share = err / bar
    i = np.unravel_index(np.nanargmax(share), share.shape)
    return float(share[i]), float(x[i])


@pytest.mark.parametrize("act", ["exponential", "sigmoid", "squareplus", "softplus", "sine"])
def test_activation_forward_over_every_finite_half(act):
    over = []
    for W in (16, 32):
        x, y = _sweep_forward(act, W)
        y64, y32 = P.act_forward64(act, x), P.act_forward32(act, x)
        yd = y.astype(np.float64)
        if act == "sine":
            assert np.isfinite(yd).all() and (np.abs(yd) <= 1).all()
            big = np.abs(x.astype(np.float64)) >= 100
            e = np.abs(yd - y64)
            per_binade = [float(e[big & (np.abs(x.astype(np.float64)) >= 2.0 ** k) & (np.abs(x.astype(np.float64)) < 2.0 ** (k + 1))].max()) for k in range(6, 16)]
            print(f"[ffmlp-probe] sine W={W}: worst |error| per binade 2^6 .. 2^15 for |x| >= 100: {['%.2e' % v for v in per_binade]}")
            sel = ~big
        else:
            assert np.array_equal(np.isinf(yd), np.isinf(y32.astype(np.float64))), (act, "infinite set", x[np.isinf(yd) != np.isinf(y32.astype(np.float64))][:8])
            assert np.array_equal(yd == 0, y32 == 0), (act, "zero set", x[(yd == 0) != (y32 == 0)][:8])
            assert not np.isnan(yd).any()
            sel = np.isfinite(yd)
        err = np.where(sel, np.abs(np.where(sel, yd, 0) - np.where(sel, y64, 0)), 0.0)
        share, at = _worst(err, P.forward_bar(act, x, np.where(sel, y64, 1.0)), x)
        print(f"[ffmlp-probe] {act} forward W={W}: worst distance {share:.3f} of its bar at x = {at!r}; inf {int(np.isinf(yd).sum())}, zero {int((yd == 0).sum())}, "
              f"subnormal {int(((np.abs(yd) < 2.0 ** -14) & (yd != 0)).sum())}")
        if share > 1.0:
            over.append((act, W, share, at))
    assert not over, over


@pytest.mark.parametrize("act", ["exponential", "sigmoid", "squareplus", "softplus"])
def test_activation_backward_over_every_finite_half(act):
    over = []
    for g in (1.0, -1.0, 2.0 ** -14, 1000.0):
        rc, f, d = _sweep_backward(act, g)
        assert rc == 0
        d64 = P.act_backward_factor64(act, f)
        want = g * d64
        dd = d.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            want16 = P.r16(g * P.r16(d64).astype(np.float64)).astype(np.float64)
        fin = np.isfinite(want16) & (np.abs(want) < 65504.0 - 32.0)
        # beyond the finite range both must overflow (or come within a rounding of it) the same way
        assert np.array_equal(np.isnan(dd), np.isnan(want16)), (act, g)
        assert (np.isinf(dd[~fin & ~np.isnan(want16)]) | (np.abs(dd[~fin & ~np.isnan(want16)]) >= 65504.0 - 64.0)).all(), (act, g)
        with np.errstate(invalid="ignore", over="ignore"):
            bar = np.where(fin, P.backward_bar(act, g, f), 1.0)
        err = np.where(fin, np.abs(np.where(fin, dd, 0) - np.where(fin, want, 0)), 0.0)
        share, at = _worst(err, bar, f)
        print(f"[ffmlp-probe] {act} backward g={g!r}: worst distance {share:.3f} of its bar at f = {at!r}")
        if share > 1.0:
            over.append((act, g, share, at))
    assert not over, over


def test_sine_backward_stays_refused():
    rc, _, _ = _sweep_backward("sine", 1.0)
    assert rc == P.SDN_E_UNSUPPORTED
