"""`dnerf_amd.renderer.loop_schedule` -- the Python statement of the schedule replay behind the one-pass renderer's rgb tint (phase B of
`sdn_whole_rays_schedule`, csrc/seal.hip) -- against a host-stepped loop written out here the way SealDNeRF/renderer.py:226-281 steps it:
n_step = max(min(N // n_alive, 8), 1), march n_step slots per alive ray, composite (which kills), compact."""
import numpy as np
import pytest

from dnerf_amd.renderer import loop_schedule


def stepped_loop(counts, stops, max_steps):
    """The loop itself on sample INDICES: a ray's k-th sample is (ray, k); `march` hands every alive ray its next n_step samples (empty
    slots once it has run out, as march_rays leaves zeros), `composite` walks a ray's slots as kernel_composite_rays does -- an empty
    slot ends the ray, the sample at which the transmittance test fires is still composited and ends it too -- and marks dead rays -1.
    -> (iteration of every sample, packed ray after ray; (n_alive, n_step) per iteration; was a ray alive when max_steps ended it)."""
    N = len(counts)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = np.full(int(first[-1]), -1, dtype=np.int32)
    rays_alive = np.arange(N, dtype=np.int32)
    rays_k = np.zeros(N, dtype=np.int64)          # rays_t: here, the index of a ray's next sample
    step, it, trace = 0, 0, []
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        # march_rays
        slots = np.full((n_alive, n_step), -1, dtype=np.int64)
        for n, r in enumerate(rays_alive):
            have = max(min(int(counts[r] - rays_k[r]), n_step), 0)
            slots[n, :have] = rays_k[r] + np.arange(have)
            ids[first[r] + rays_k[r]: first[r] + rays_k[r] + have] = it           # marched, evaluated and mapped in this iteration
        # composite_rays
        for n, r in enumerate(rays_alive.copy()):
            s = 0
            while s < n_step:
                if slots[n, s] < 0:
                    break
                if slots[n, s] == stops[r]:
                    break
                s += 1
            rays_k[r] += s
            if s < n_step:
                rays_alive[n] = -1
        rays_alive = rays_alive[rays_alive >= 0]
        trace.append((n_alive, n_step))
        step += n_step
        it += 1
    return ids, trace, rays_alive.shape[0] > 0


def random_case(rng, N, max_count, p_empty, p_stop):
    counts = rng.integers(1, max_count + 1, N)
    counts[rng.random(N) < p_empty] = 0
    stops = counts.copy()                                        # no kill: the ray runs out of samples
    killed = (rng.random(N) < p_stop) & (counts > 0)
    stops[killed] = rng.integers(0, counts[killed])              # anywhere, the first sample included
    first_sample = killed & (rng.random(N) < 0.2)
    stops[first_sample] = 0
    return counts, stops


@pytest.mark.parametrize("N,max_count,p_empty,p_stop,max_steps", [
    (1, 40, 0.0, 0.5, 1024),
    (63, 90, 0.6, 0.5, 1024),          # most rays empty: n_step climbs at once
    (64, 30, 0.0, 0.9, 1024),
    (100, 200, 0.3, 0.3, 64),          # long rays against a short loop: max_steps ends it
    (257, 120, 0.8, 0.4, 1024),
    (1000, 60, 0.5, 0.7, 16),
    (1000, 300, 0.1, 0.1, 1024),       # n_step stays 1 for a long time
])
def test_loop_schedule_is_the_stepped_loop(N, max_count, p_empty, p_stop, max_steps):
    rng = np.random.default_rng(1000 * N + max_steps)
    saw_cut = False
    for _ in range(3):
        counts, stops = random_case(rng, N, max_count, p_empty, p_stop)
        want_ids, want_trace, cut = stepped_loop(counts, stops, max_steps)
        ids, trace = loop_schedule(counts, stops, max_steps)
        assert trace == want_trace
        assert np.array_equal(ids, want_ids)
        assert sum(s for _, s in trace) <= max_steps + 7 and all(1 <= s <= 8 for _, s in trace)
        saw_cut |= cut
    if max_steps < 1024:
        assert saw_cut, "this case is here for the loop that max_steps ends with rays alive"


def test_the_cases_cover_what_they_claim():
    """Rays without samples, rays killed at their first sample, kills strictly inside a window (samples behind them carry the window's
    iteration) and an N that is no multiple of 64 all occur in one case; checked on the helper's own output."""
    rng = np.random.default_rng(7)
    counts, stops = random_case(rng, 257, 120, 0.8, 0.4)
    assert (counts == 0).any() and ((stops == 0) & (counts > 0)).any() and len(counts) % 64 != 0
    ids, trace = loop_schedule(counts, stops, 1024)
    assert len({s for _, s in trace}) >= 3
    first = np.concatenate([[0], np.cumsum(counts)])
    behind = [r for r in range(len(counts)) if stops[r] + 1 < counts[r] and ids[first[r] + stops[r] + 1] == ids[first[r] + stops[r]]]
    assert behind, "no kill strictly inside a window"
    empty = np.nonzero(counts == 0)[0]
    assert trace[0] == (257, 1) and trace[1][0] <= 257 - len(empty)


def test_degenerate_inputs():
    ids, trace = loop_schedule([0, 0, 0], [0, 0, 0])
    assert ids.shape == (0,) and trace == [(3, 1)]
    ids, trace = loop_schedule([5], [5], max_steps=1024)          # one ray: n_step 1 throughout, a last iteration finds nothing left
    assert ids.tolist() == [0, 1, 2, 3, 4] and trace == [(1, 1)] * 6
    ids, trace = loop_schedule([5], [5], max_steps=3)
    assert ids.tolist() == [0, 1, 2, -1, -1] and trace == [(1, 1)] * 3
    ids, trace = loop_schedule([4, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0])
    # iteration 0: 8 alive, 1 sample; iteration 1: 1 alive, window of 8 holds samples 1..3, the kill at sample 1 is inside it
    assert ids.tolist() == [0, 1, 1, 1] and trace == [(8, 1), (1, 8)]
