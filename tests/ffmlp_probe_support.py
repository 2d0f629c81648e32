"""Probe cases and exact references for the fused MLP operator (csrc/ffmlp.hip, csrc/ffmlp_kernels.h), numpy only; validated without
a GPU by tests/test_ffmlp_probes_cpu.py and used on the MI355X by tests/test_gpu_ffmlp_probes.py.

Exact cases.  The matrix cores' accumulation order cannot be restated, so the cases are built such that every order gives the same
bits: inputs and output gradients are small signed integers, every layer but one is a signed routing matrix (one +-1 per row, the
columns a seeded permutation), and one layer -- its position cycles over all L + 1 -- is dense with entries in {-1, 0, 1}.  A case
is CERTIFIED EXACT when, for every sum the operator forms (every layer output forward, every pre-activation gradient, grad_inputs,
every dW[m][n] over the batch), the sum of the absolute values of its products divided by their common quantum is below 2^24: all
fp32 partial sums, in any order, are then exact integers times that quantum, and the result is float64 of the same numbers rounded
once (float64 -> float32 -> fp16).  `reference()` returns that result together with the certificate's worst ratio.

The launch rule (`launch_variant`, `dw_plan`) restates `launch_width`, `dw_splits`, `dw_blocks`, `dw_batched` and the split sizes of
`sdn_ffh::dw_jobs` as pure functions, so that the tests can name the kernel variant every case runs and size batches on both sides
of every boundary from the CU count of the machine.

ReLU follows the reference's formulas, products with the compare result (ffmlp/src/utils.h:430, :543): x * (x > 0), g * (f > 0).
"""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
ACT = {"relu": 0, "exponential": 1, "sine": 2, "sigmoid": 3, "squareplus": 4, "softplus": 5, "none": 6}
K_ACT = 10.0
WIDTHS = {16: dict(NT=2, OCC=4, RW=4, SW=4), 32: dict(NT=2, OCC=4, RW=4, SW=4), 64: dict(NT=1, OCC=4, RW=4, SW=8),
          128: dict(NT=1, OCC=4, RW=4, SW=8), 256: dict(NT=1, OCC=2, RW=4, SW=8)}
RESIDENT_MAX_FRAGS = 64
DW_ROWS = 64                       # batch rows per LDS tile of k_ffmlp_dw
DW_BUDGET = 64 << 20
DW_MAX_JOBS = 17
SDN_E_UNSUPPORTED = -2


def div_up(a, b):
    return -(-a // b)


# ---- the launch rule ------------------------------------------------------------------------------------------------------------------
def total_frags(in_dim, W, L, backward, with_last):
    MT, KS = div_up(W, 32), W // 16
    if not backward:
        return MT * (in_dim // 16) + (L - 1) * MT * KS + KS
    return MT + (L - 1) * MT * KS + (div_up(in_dim, 32) * KS if with_last else 0)


def launch_variant(W, in_dim, L, with_last, direction, B, cus):
    """`launch_width`'s choice -> dict(kind, waves, points (per workgroup), grid, ntiles, tile_loop, lone_wave).
    kind: resident | latency-2 | latency-4 | latency-sw | throughput (width 256 has only the last of the streamed ones).
    lone_wave: the last workgroup holds a wave without a live point next to a live one (the `wave_full == false` path)."""
    p = WIDTHS[W]
    backward = direction == "backward"
    frags = total_frags(in_dim, W, L, int(backward), with_last if backward else 1)
    wave_pts = 32 * p["NT"]

    def made(kind, waves, grid):
        pts = waves * wave_pts
        ntiles = div_up(B, pts)
        tail = B - (ntiles - 1) * pts
        return dict(kind=kind, waves=waves, points=pts, grid=grid, ntiles=ntiles, tile_loop=ntiles > grid, frags=frags,
                    lone_wave=waves > 1 and div_up(tail, wave_pts) < waves)

    if frags <= RESIDENT_MAX_FRAGS:
        per_cu = max(1, min(163840 // max(frags * 1024, 1024), p["OCC"] * 4 // p["RW"]))
        return made("resident", p["RW"], min(div_up(B, p["RW"] * wave_pts), cus * per_cu))
    ntiles = div_up(B, p["SW"] * wave_pts)
    if W in (64, 128) and p["OCC"] > 2 and ntiles <= cus:
        if div_up(B, 2 * wave_pts) <= 2 * cus:
            return made("latency-2", 2, div_up(B, 2 * wave_pts))
        if div_up(B, 4 * wave_pts) <= 2 * cus:
            return made("latency-4", 4, div_up(B, 4 * wave_pts))
        return made("latency-sw", p["SW"], ntiles)
    return made("throughput", p["SW"], ntiles)


def resident_capacity(W, in_dim, L, cus):
    """Points one launch of the resident forward kernel covers without its tile loop."""
    v = launch_variant(W, in_dim, L, 1, "forward", 1 << 30, cus)
    assert v["kind"] == "resident"
    return v["grid"] * v["points"]


def dw_blocks(M, N):
    return div_up(div_up(M, 32) * 32, 128) * div_up(div_up(N, 32) * 32, 128)


def dw_splits(B, blocks):
    return max(1, min(div_up(B, 256), 512 // blocks))


def dw_partial_bytes(B, M, N):
    return dw_splits(B, dw_blocks(M, N)) * div_up(M, 32) * 32 * div_up(N, 32) * 32 * 4


def dw_batched(B, in_dim, W, L):
    total = dw_partial_bytes(B, 16, W) + (L - 1) * dw_partial_bytes(B, W, W) + dw_partial_bytes(B, W, in_dim)
    return L + 1 <= DW_MAX_JOBS and total <= DW_BUDGET


def dw_plan(W, in_dim, L, B):
    """-> (batched, jobs): per weight matrix, in flat-weight order (layer 0 .. L), the split geometry `dw_jobs` uses."""
    jobs = []
    for M, N in [(W, in_dim)] + [(W, W)] * (L - 1) + [(16, W)]:
        blocks = dw_blocks(M, N)
        ns = dw_splits(B, blocks)
        rows = div_up(div_up(B, ns), DW_ROWS) * DW_ROWS
        used = div_up(B, rows)
        jobs.append(dict(M=M, N=N, blocks=blocks, splits=ns, at_cap=ns == 512 // blocks and div_up(B, 256) > ns, rows_per_split=rows,
                         used=used, last_rows=B - (used - 1) * rows))
    return dw_batched(B, in_dim, W, L), jobs


def first_unbatched_batch(W, in_dim, L):
    """Smallest B whose partial sums no longer fit the one-launch budget (None if every B fits)."""
    for ns in range(1, 514):
        if not dw_batched((ns - 1) * 256 + 1, in_dim, W, L):
            return (ns - 1) * 256 + 1
    return None


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# B is a number or the name of a rule resolved from the CU count: the smallest batch on each side of every boundary of the launch rule
BATCH_RULES = {
    "res_loop": lambda s, c: resident_capacity(s["W"], s["in_dim"], s["L"], c) + 77,
    "lat2_max": lambda s, c: 2 * c * 2 * 32 * WIDTHS[s["W"]]["NT"],
    "lat4_min": lambda s, c: 2 * c * 2 * 32 * WIDTHS[s["W"]]["NT"] + 1,
    "lat4_max": lambda s, c: c * WIDTHS[s["W"]]["SW"] * 32 * WIDTHS[s["W"]]["NT"],
    "thr_min": lambda s, c: c * WIDTHS[s["W"]]["SW"] * 32 * WIDTHS[s["W"]]["NT"] + 1,
    "unbatched": lambda s, c: first_unbatched_batch(s["W"], s["in_dim"], s["L"]),
}


def _specs():
    out = []

    def add(name, W, in_dim, L, B, dense="all", dx=True, acts=("relu", "none")):
        positions = range(L + 1) if dense == "all" else [dense]
        for act in acts:
            for d in positions:
                out.append(dict(name=f"{name}-{act}-d{d}", family=name, W=W, in_dim=in_dim, L=L, B=B, dense=d, act=act, dx=dx,
                                seed=len(out) + 1))

    add("res64", 64, 16, 2, 1000)                        # resident, no tile loop; N = 16; ragged last tile
    add("res64-nodx", 64, 64, 2, 200, dense=1, dx=False)  # in_dim = width; one dW split; calc_grad_inputs off
    add("res-loop16", 16, 16, 2, "res_loop", dense=1)    # resident with its tile loop; width 16; dW splits at the cap, ragged last
    add("res32-lone", 32, 32, 3, 513)                    # width 32; B = 1 mod 256: a wave without live points
    add("one-row", 64, 32, 2, 1, dense=0)                # B = 1
    add("tail-row", 64, 32, 3, 257, dense=2)             # two dW splits of 192 rows: the second holds 65, a full LDS tile and one row
    add("tail-split", 64, 32, 2, 769, dense=1)           # four dW splits of 256 rows: the last is a single row
    add("in128-w16", 16, 128, 2, 300, dense=0)           # in_dim > width, KS0 > KS
    add("in288-w128", 128, 288, 2, 300, dense=0)         # in_dim > width; N = 288: three column blocks, the last 32 wide
    add("lat2-128", 128, 32, 3, 300)                     # streamed latency variant, 2 waves, ragged
    add("deep64", 64, 32, 16, 300, dx=False)             # L = 16: 17 weight-gradient jobs
    add("deep64-dx", 64, 32, 16, 77, dense=16, acts=("relu",))
    for W, L in ((64, 9), (128, 3)):
        for rule in ("lat2_max", "lat4_min", "lat4_max", "thr_min"):
            add(f"{rule}-{W}", W, 32, L, rule, dense=L // 2)
    add("w256", 256, 16, 2, 300, dense=1)                # width 256: streamed, no latency variant
    add("w256-unbatched", 256, 512, 2, "unbatched", dense=0)   # in_dim = 512; weight gradients layer by layer
    return out


SPECS = _specs()
SPEC_BY_NAME = {s["name"]: s for s in SPECS}


def resolve(spec, cus):
    s = dict(spec)
    if isinstance(s["B"], str):
        s["B"] = BATCH_RULES[s["B"]](s, cus)
    s["cus"] = cus
    return s


def layer_shapes(W, in_dim, L):
    return [(W, in_dim)] + [(W, W)] * (L - 1) + [(16, W)]


def _routing(rng, M, K, p_neg):
    """One +-1 per row, the columns a seeded permutation (repeated when M > K); when K > M every column is routed to some row
    (K / M entries per row), so that no input feature -- and no column of the gradient flowing back -- is left out."""
    perm = rng.permutation(K)
    m = np.zeros((M, K), F64)
    n = max(M, K)
    m[np.arange(n) % M, perm[np.arange(n) % K]] = np.where(rng.random(n) < p_neg, -1.0, 1.0)
    return m


def nonzero_rows(rng, B):
    """Rows that carry an output gradient: one seeded row in every 64-row LDS tile of the weight-gradient kernel (tiles are 64-aligned:
    rows_per_split is a multiple of 64), the last row, and a seeded share of the rest that keeps about 4096 rows in a large batch."""
    live = rng.random(B) < min(1.0, 4096.0 / B)
    starts = np.arange(0, B, DW_ROWS)
    live[starts + (rng.integers(0, DW_ROWS, starts.size) % np.minimum(DW_ROWS, B - starts))] = True
    live[B - 1] = True
    return live


def make_case(s):
    """-> dict(w flat fp16, mats, x [B, in] fp16, g [B, 16] fp16, live rows).  Under ReLU the hidden routing layers after the first
    carry a -1 on an eighth of their rows only (a closed gate stays closed through every later routing layer)."""
    rng = np.random.default_rng(1000 + s["seed"])
    relu = s["act"] == "relu"
    mats = []
    for i, (M, K) in enumerate(layer_shapes(s["W"], s["in_dim"], s["L"])):
        if i == s["dense"]:
            mats.append(rng.integers(-1, 2, (M, K)).astype(F64))
        else:
            mats.append(_routing(rng, M, K, 0.125 if relu and 0 < i < s["L"] else 0.5))
    B = s["B"]
    x = rng.integers(-2, 3, (B, s["in_dim"])).astype(F16)
    live = nonzero_rows(rng, B)
    g = (rng.integers(-2, 3, (B, 16)) * live[:, None]).astype(F16)
    g[live, 0] = np.where(rng.random(int(live.sum())) < 0.5, -1, 1)      # (a live row is never all zero)
    return dict(w=np.concatenate([m.reshape(-1) for m in mats]).astype(F16), mats=mats, x=x, g=g, live=live)


# Non-finite values ride on exact cases whose FIRST layer is the dense one: a resident and a streamed variant, both epilogues.
NONFINITE = ("res64-relu-d0", "res64-none-d0", "lat2-128-relu-d0", "lat2-128-none-d0")


def make_nonfinite_case(s):
    """The exact case with, in chosen rows: inputs of 8192 under an all +1 and an all -1 weight row (exact sums of +-131072 and beyond:
    +-inf after the one rounding; -inf is NaN behind a ReLU), a NaN, a +inf and a -inf input (a routing row multiplies them by 0 too: the
    whole sample turns NaN downstream), and infinite and NaN output gradients on samples whose gates are open, closed and NaN."""
    assert s["dense"] == 0 and s["B"] >= 64
    c = make_case(s)
    c["mats"][0][0, :], c["mats"][0][1, :] = 1.0, -1.0
    c["w"] = np.concatenate([m.reshape(-1) for m in c["mats"]]).astype(F16)
    x, g = c["x"], c["g"]
    x[3, :], x[8, :] = 8192, -8192
    x[5, 2], x[6, 4], x[7, 1] = np.nan, np.inf, -np.inf
    g[10:14, :] = 1
    g[10, 3], g[11, 5], g[12, 0] = np.inf, np.nan, -np.inf
    g[3, :], g[5, :], g[8, :] = 2, -1, 1                    # finite gradients behind infinite, NaN and closed gates
    g[6, 7] = np.inf                                        # an infinite gradient behind NaN gates
    c["live"][[3, 5, 8, 10, 11, 12, 13, 6]] = True
    return c


def same_bits_or_nan(a, b):
    """Bit for bit, a NaN matching any NaN (the sign and payload of a NaN the hardware makes are not part of the contract)."""
    a, b = np.ascontiguousarray(a, F16), np.ascontiguousarray(b, F16)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb])


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------------
def r16(a):
    """float64 -> float32 -> fp16, the one rounding of a layer output whose sum sits in a float32 accumulator."""
    with np.errstate(over="ignore"):
        return np.asarray(a, F64).astype(F32).astype(F16)


def quantum(a):
    """Largest power of two every element of the fp16 array is a multiple of (1 for an all-zero array)."""
    v = np.abs(np.asarray(a, F64))
    v = v[np.isfinite(v) & (v != 0)]
    if v.size == 0:
        return 1.0
    i = (v * 2.0 ** 24).astype(np.int64)
    return float(np.min(i & -i)) * 2.0 ** -24


def lin64(a, b, cert=None):
    """[R, K] x [M, K] -> [R, M] in float64; records the certificate ratio max(sum_k |a||b|) / quantum."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    if cert is not None:
        fa, fb = np.where(np.isfinite(a), np.abs(a), 0.0), np.where(np.isfinite(b), np.abs(b), 0.0)
        cert.append(float((fa @ fb.T).max()) / (quantum(a) * quantum(b)))
    with np.errstate(invalid="ignore"):
        return a @ b.T


def lin32(a, b, order):
    """The same sum in float32, term by term: order 'forward', 'reversed', or 'mfma' (pairwise inside blocks of 16 k, blocks in turn)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    R, K = a.shape
    acc = np.zeros((R, b.shape[0]), F32)
    if order in ("forward", "reversed"):
        ks = range(K) if order == "forward" else range(K - 1, -1, -1)
        for k in ks:
            acc += a[:, k, None] * b[None, :, k]
        return acc
    pad = -K % 16
    a, b = np.pad(a, ((0, 0), (0, pad))), np.pad(b, ((0, 0), (0, pad)))
    for k0 in range(0, K + pad, 16):
        t = a[:, k0:k0 + 16, None] * b.T[None, k0:k0 + 16, :]
        while t.shape[1] > 1:
            t = t[:, 0::2] + t[:, 1::2]
        acc += t[:, 0]
    return acc


def relu_forward(z16):
    with np.errstate(invalid="ignore"):
        return z16 * (z16 > 0).astype(F16)


def relu_backward(g16, f16):
    with np.errstate(invalid="ignore"):
        return g16 * (f16 > 0).astype(F16)


WRONG = ("swap_runs", "k_order", "shift_layers", "drop_ragged_tile", "drop_split_tail", "transpose_dw_block")


def _swap_runs(buf):
    """Features 4..7 and 8..11 of every 16-feature row piece exchanged: what a wrong half-wave exchange stores."""
    out = buf.copy()
    v, o = buf.reshape(*buf.shape[:-1], -1, 16), out.reshape(*buf.shape[:-1], -1, 16)
    o[..., 4:8], o[..., 8:12] = v[..., 8:12], v[..., 4:8]
    return out


def reference(s, c, lin=None, wrong=None):
    """The operator on case `c` of spec `s` -> dict(out, fwd [L, B, W], bwd [L, B, W] (output side first), gi, gw (flat), cert).
    lin: the product-sum primitive (default: float64 with the certificate); wrong: one of WRONG, a deliberately wrong restatement."""
    cert = []
    if lin is None:
        lin = lambda a, b: lin64(a, b, cert)                                        # noqa: E731
    W, L, B, relu = s["W"], s["L"], s["B"], s["act"] == "relu"
    mats = [m.astype(F16) for m in c["mats"]]
    fmats = mats
    if wrong == "k_order":       # the two middle 4-element runs of every 16-wide k-step of the weights exchanged
        fmats = [_swap_runs(m) for m in mats]
    x, fwd = c["x"], []
    for m in fmats[:-1]:
        z = r16(lin(x, m))
        x = relu_forward(z) if relu else z
        fwd.append(x)
    out = r16(lin(x, fmats[-1]))
    fwd = np.stack(fwd)
    if wrong == "swap_runs":
        fwd = _swap_runs(fwd)
    if wrong == "shift_layers":
        fwd = np.roll(fwd, 1, axis=0)
    if wrong == "drop_ragged_tile":
        pts = launch_variant(W, s["in_dim"], L, 1, "forward", B, s["cus"])["points"]
        out = out.copy()
        out[(B - 1) // pts * pts:] = 0
    g, bwd, dws = c["g"], [], [None] * (L + 1)

    def dw(G, X, job):
        if wrong == "drop_split_tail":          # the rows of the last split's ragged last LDS tile never summed
            keep = (B - 1) // DW_ROWS * DW_ROWS
            G, X = G[:keep], X[:keep]
        if G.shape[0] == 0:
            return np.zeros((G.shape[1], X.shape[1]), F16)
        d = r16(lin(G.T, X.T))
        if wrong == "transpose_dw_block" and min(d.shape) >= 32:
            d = d.copy()
            d[:32, :32] = d[:32, :32].T.copy()
        return d

    dws[L] = dw(g, fwd[L - 1], L)
    for k in range(L):
        z = r16(lin(g, mats[L - k].T))
        g = relu_backward(z, fwd[L - 1 - k]) if relu else z
        bwd.append(g)
        dws[L - 1 - k] = dw(g, fwd[L - 2 - k] if L - 2 - k >= 0 else c["x"], L - 1 - k)
    gi = r16(lin(g, mats[0].T)) if s["dx"] else None
    return dict(out=out, fwd=fwd, bwd=np.stack(bwd), gi=gi, gw=np.concatenate([d.reshape(-1) for d in dws]), cert=max(cert) if cert else 0.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F16), np.ascontiguousarray(b, F16)
    return a.shape == b.shape and np.array_equal(a.view(np.uint16), b.view(np.uint16))


def results_equal(a, b):
    return all((a[k] is None and b[k] is None) or same_bits(a[k], b[k]) for k in ("out", "fwd", "bwd", "gi", "gw"))


def live_rows_reach_every_tile(s, c):
    """Every LDS tile of every split of every weight-gradient job holds a row with a non-zero output gradient."""
    B, live = s["B"], c["live"]
    _, jobs = dw_plan(s["W"], s["in_dim"], s["L"], B)
    for j in jobs:
        for sp in range(j["used"]):
            b0, b1 = sp * j["rows_per_split"], min(B, (sp + 1) * j["rows_per_split"])
            for t0 in range(b0, b1, DW_ROWS):
                if not live[t0:min(b1, t0 + DW_ROWS)].any():
                    return False
    return True


def describe(s):
    """One line: the kernel variant of each direction and the weight-gradient plan of the case."""
    f = launch_variant(s["W"], s["in_dim"], s["L"], 1, "forward", s["B"], s["cus"])
    b = launch_variant(s["W"], s["in_dim"], s["L"], int(s["dx"]), "backward", s["B"], s["cus"])
    batched, jobs = dw_plan(s["W"], s["in_dim"], s["L"], s["B"])

    def one(v):
        return f"{v['kind']}{'+loop' if v['tile_loop'] else ''}{'+lone' if v['lone_wave'] else ''}({v['grid']}x{v['waves']}w)"

    return (f"{s['name']}: {s['in_dim']}->{s['W']}x{s['L']} B={s['B']} act={s['act']} dx={int(s['dx'])} | fwd {one(f)} bwd {one(b)} | dW "
            f"{'batched' if batched else 'layer-by-layer'} splits {sorted({(j['used'], j['last_rows']) for j in jobs})}")


def coverage(cus):
    """-> (hit, unreachable): the named features each (epilogue, mode) / each epilogue reaches over all cases at this CU count."""
    hit = set()
    for spec in SPECS:
        s = resolve(spec, cus)
        f = launch_variant(s["W"], s["in_dim"], s["L"], 1, "forward", s["B"], cus)
        b = launch_variant(s["W"], s["in_dim"], s["L"], int(s["dx"]), "backward", s["B"], cus)
        for mode, v in (("inference", f), ("forward", f), ("backward", b)):
            tags = [v["kind"] + ("+loop" if v["tile_loop"] else "") if v["kind"] == "resident" else f"{v['kind']}-w{s['W']}"]
            tags += [f"width{s['W']}", f"in{s['in_dim']}", f"L{s['L']}", f"dx{int(s['dx'])}"]
            tags += ["lone_wave"] if v["lone_wave"] else []
            tags += ["B1"] if s["B"] == 1 else []
            tags += ["in=width"] if s["in_dim"] == s["W"] else []
            tags += [f"in{s['in_dim']}>w{s['W']}"] if s["in_dim"] > s["W"] else []
            hit.update((s["act"], mode, t) for t in tags)
        batched, jobs = dw_plan(s["W"], s["in_dim"], s["L"], s["B"])
        tags = ["dw-batched" if batched else "dw-layer-by-layer", f"dw-jobs{len(jobs)}"]
        for j in jobs:
            tags += ["dw-1split"] if j["used"] == 1 else []
            tags += ["dw-2splits-1row-tile"] if j["used"] == 2 and j["last_rows"] % DW_ROWS == 1 else []
            tags += ["dw-1row-split"] if j["used"] > 1 and j["last_rows"] == 1 else []
            tags += ["dw-cap-ragged"] if j["at_cap"] and j["last_rows"] % DW_ROWS else []
            tags += [f"dw-M{j['M']}", f"dw-N{j['N']}"]
        hit.update((s["act"], "dw", t) for t in tags)
    return hit


def required():
    need = set()
    for act in ("relu", "none"):
        for mode in ("inference", "forward", "backward"):
            for t in ("resident", "resident+loop", "latency-2-w64", "latency-4-w64", "throughput-w64", "latency-2-w128", "latency-4-w128",
                      "throughput-w128", "throughput-w256", "width16", "width32", "lone_wave", "B1", "in16", "in=width", "in288>w128",
                      "in128>w16", "in512", "L2", "L16"):
                need.add((act, mode, t))
        need.update((act, "backward", t) for t in ("dx0", "dx1"))
        need.update((act, "dw", t) for t in ("dw-1split", "dw-2splits-1row-tile", "dw-1row-split", "dw-cap-ragged", "dw-batched", "dw-layer-by-layer", "dw-M16",
                                             "dw-N16", "dw-N288", "dw-jobs17"))
    return need


def unreachable(cus):
    """Compiled variants no batch reaches at this CU count.  The SW-wave latency branch needs div_up(B, SW * 32) <= cus together with
    div_up(B, 4 * 32) > 2 cus; the first gives B <= 256 cus (SW = 8, NT = 1), which contradicts the second at every CU count."""
    out = []
    for W in (64, 128):
        if not any(launch_variant(W, 32, 9, 1, "forward", B, cus)["kind"] == "latency-sw" for B in range(1, 256 * cus + 2, 31)):
            out.append(f"latency-sw-w{W}")
    return out


# ---- activations, one element at a time -----------------------------------------------------------------------------------------------
def all_finite_halves():
    """Every finite fp16 value, both signs, subnormals and both zeros: 63 488 values as [3968, 16]."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    v = bits.view(F16)
    v = v[np.isfinite(v)]
    assert v.size == 63488
    return v.reshape(-1, 16).copy()


def ulp16(v):
    """Spacing of fp16 at |v| (the subnormal spacing 2^-24 below 2^-14)."""
    a = np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def act_forward64(act, x16):
    """The activation of the fp16 argument in float64 (the exact function the reference's float formulas approximate)."""
    x = x16.astype(F64)
    with np.errstate(over="ignore"):
        if act == "exponential":
            return np.exp(x)
        if act == "sine":
            return np.sin(x)
        if act == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if act == "squareplus":
            s = x * K_ACT
            return np.where(s < 0, 2.0 / (np.sqrt(s * s + 4.0) - s), 0.5 * (s + np.sqrt(s * s + 4.0))) / K_ACT
        if act == "softplus":
            s = x * K_ACT
            return (np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))) / K_ACT
    raise ValueError(act)


def act_forward32(act, x16):
    """The reference's own float formulas (utils.h:433-462) in float32, rounded to fp16: where its results are infinite or zero."""
    x = x16.astype(F32)
    one, k = F32(1), F32(K_ACT)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        if act == "exponential":
            y = np.exp(x)
        elif act == "sine":
            y = np.sin(x)
        elif act == "sigmoid":
            y = one / (one + np.exp(-x))
        elif act == "squareplus":
            s = x * k               # (the kernel's form: for s < 0 the reference's sum cancels to 0 or one quantum of |s|)
            r = np.sqrt(s * s + F32(4))
            y = np.where(s < 0, F32(2) / (r - s), F32(0.5) * (s + r)) / k
        elif act == "softplus":
            y = np.log(np.exp(x * k) + one) / k
        else:
            raise ValueError(act)
        return y.astype(F16)


def forward_bar(act, x16, ref64):
    """Half an fp16 ulp of the exact result, the hardware form's documented error (csrc/ffmlp_kernels.h: 1e-6 relative; sine 1e-5
    absolute for |x| < 100), and the fp16 subnormal spacing as the absolute floor."""
    hw = 1e-5 if act == "sine" else 1e-6 * np.abs(ref64)
    return 0.5 * ulp16(ref64) + hw + 2.0 ** -24


def act_backward_factor64(act, f16):
    f = f16.astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == "exponential":
            return f
        if act == "sigmoid":
            return f * (1.0 - f)
        if act == "squareplus":
            y = f * K_ACT
            return y * y / (y * y + 1.0)
        if act == "softplus":
            return 1.0 - np.exp(-f * K_ACT)
    raise ValueError(act)


def backward_bar(act, g, f16):
    """act_backward16 rounds twice: the derivative factor d to fp16, then the product g * d16 to fp16 (half an ulp each, the first
    times |g|).  exponential has no first rounding (d = f); sigmoid rounds 1 - f as well (one more half ulp of 1 - f, times f).
    The float evaluation of d carries float32's own rounding (2^-24 relative per operation, 4 at most) and the hardware forms' 1e-6
    relative error -- of the hardware form's RESULT: for softplus that is e = exp(-10 f) in d = 1 - e, so 1e-6 |e|, not 1e-6 |d|."""
    g = abs(float(g))
    d64 = act_backward_factor64(act, f16)
    f = f16.astype(F64)
    with np.errstate(over="ignore"):
        hw = {"exponential": 0.0, "sigmoid": 0.0, "squareplus": 1e-6 * np.abs(d64), "softplus": (1e-6 + 2.0 ** -24) * np.exp(-f * K_ACT)}[act]
    first = 0.0 if act == "exponential" else 0.5 * ulp16(d64) + 4 * 2.0 ** -24 * np.abs(d64) + hw + 2.0 ** -25
    if act == "sigmoid":
        first = first + np.abs(f) * 0.5 * ulp16(1.0 - f)
    return g * first + 0.5 * ulp16(g * d64) + 2.0 ** -24
