"""Shared by tests/test_basis_f32_cpu.py and tests/test_gpu_basis_f32.py: the ONE fp32 bar the temporal-basis model's fp32 fused field
(csrc/field_basis_f32.hip) is held to, and a numpy restatement of its weight packing.

The bar: rtol = 1e-4, atol = 1e-6 on sigma and on rgb against `BasisOracle(mode="fp32")` (float64 accumulation) -- the bar
tests/test_gpu_field_f32.py holds the fp32 deformation kernel to.  The margin comes from the fixture: the reference's own fp32
evaluation (GEMMs of unspecified order) lies within 2e-5 of that restatement on these weights (tests/test_basis_cpu.py); an
fp32-accumulating kernel is the same kind of evaluation, and 1e-4 leaves it five times that.
"""
import numpy as np

f32 = np.float32
RTOL, ATOL = 1e-4, 1e-6
STAGE_FLOATS = 15360          # S0 | S1 | C0 | C1 | C2


def bar_failures(got, want):
    """Elementwise: True where `got` misses the bar against `want` (non-finite values miss it)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(got - want) <= ATOL + RTOL * np.abs(want))


def field_bar(sigma, rgb, want_sigma, want_rgb):
    """-> (ok, stats) of a kernel's (or a wrong variant's) sigma [N], rgb [N,3] against the expected values."""
    bs, br = bar_failures(sigma, want_sigma), bar_failures(rgb, want_rgb)
    rel = lambda g, w: np.abs(np.asarray(g, np.float64) - w) / (ATOL + RTOL * np.abs(np.asarray(w, np.float64)))  # noqa: E731
    with np.errstate(invalid="ignore"):
        stats = {"sigma_failed": int(bs.sum()), "rgb_failed": int(br.any(axis=-1).sum()), "points_failed": int((bs | br.any(axis=-1)).sum()),
                 "sigma_worst_of_bar": float(np.nanmax(rel(sigma, want_sigma))), "rgb_worst_of_bar": float(np.nanmax(rel(rgb, want_rgb)))}
    return not bs.any() and not br.any(), stats


# ---- the weight packing, restated ----------------------------------------------------------------------------------------------------------
# v_mfma_f32_32x32x2_f32, weights = A operand: per layer a block [pair][lane][m-tile] of floats; lane l of k-pair p and output tile mt
# holds W[32 mt + (l & 31)][pair p's column for k = l >> 5].
def _acc_pair(p):
    t, v = p >> 4, p & 15
    r = 32 * t + 8 * (v >> 2) + (v & 3)
    return r, r + 4


def pair_columns():
    """Per layer (S0 S1 C0 C1 C2): (m-tiles, [pair] -> (column of lane half 0, column of lane half 1))."""
    s0 = [(2 * l, 2 * l + 1) for l in range(16)]
    hidden = [_acc_pair(p) for p in range(32)]
    c0 = [(2 * p, 2 * p + 1) for p in range(8)] + [(16 + 8 * (v >> 2) + (v & 3), 16 + 8 * (v >> 2) + (v & 3) + 4) for v in range(16)]
    return [(2, s0), (2, hidden), (2, c0), (2, hidden), (1, hidden)]


def pack_numpy(weights):
    """weights: the five [out, in] float32 arrays -> flat float32 [15360]."""
    parts = []
    for W, (n_mt, pairs) in zip(weights, pair_columns()):
        W = np.asarray(W, f32)
        blk = np.zeros((len(pairs), 64, n_mt), f32)
        for p, cols in enumerate(pairs):
            for l in range(64):
                for mt in range(n_mt):
                    r = 32 * mt + (l & 31)
                    if r < W.shape[0]:
                        blk[p, l, mt] = W[r, cols[l >> 5]]
        parts.append(blk.reshape(-1))
    return np.concatenate(parts)


def unpack_numpy(flat, shapes):
    """The inverse: every weight read back from the one element that holds it; rows a tile pads must be zero."""
    out, at = [], 0
    for shape, (n_mt, pairs) in zip(shapes, pair_columns()):
        blk = flat[at:at + len(pairs) * 64 * n_mt].reshape(len(pairs), 64, n_mt)
        at += blk.size
        W = np.full(shape, np.nan, f32)
        for p, cols in enumerate(pairs):
            for l in range(64):
                for mt in range(n_mt):
                    r = 32 * mt + (l & 31)
                    if r < shape[0]:
                        W[r, cols[l >> 5]] = blk[p, l, mt]
                    else:
                        assert blk[p, l, mt] == 0
        assert not np.isnan(W).any()
        out.append(W)
    assert at == flat.shape[0]
    return out
