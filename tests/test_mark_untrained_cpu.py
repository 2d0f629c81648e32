"""NeRFRenderer.mark_untrained_grid on a CPU model (the torch restatement) against tests/golden/caller_mark_untrained.npz, which the
reference's own method produced (tests/golden/gen_mark_untrained_fixture.py), under the borderline rule of mark_untrained_support.

The renderer is built at its real 128^3 and its density grid cut to three time slices: the contract per slice is identical, and 64
slices of a two-cascade grid are 1 GiB the CPU suite has no use for."""
import numpy as np
import pytest
import torch

import mark_untrained_support as MU


def _renderer(bound, slices=3, cuda_ray=True):
    from dnerf_amd.renderer import NeRFRenderer
    r = NeRFRenderer(bound=bound, cuda_ray=cuda_ray)
    if cuda_ray:
        # a distinct, non-negative value per cell and slice: "left alone" is then a bit-for-bit statement
        g = torch.Generator().manual_seed(7)
        r.density_grid = torch.rand(slices, r.cascade, r.grid_size ** 3, generator=g)
    return r


@pytest.fixture(scope="module", params=list(MU.CASES))
def marked(request):
    case = MU.load_case(request.param)
    r = _renderer(int(case["bound"]))
    before = r.density_grid.clone()
    bits, mean, it = r.density_bitfield.clone(), r.mean_density, r.iter_density
    assert r.mark_untrained_grid(torch.from_numpy(case["poses"]), case["intrinsic"]) is None
    assert torch.equal(r.density_bitfield, bits) and r.mean_density == mean and r.iter_density == it
    return case, r, before


def test_restatement_reproduces_the_reference(marked):
    case, r, _ = marked
    assert (r.cascade, r.grid_size) == (case["cascade"], case["grid_size"])
    got = (r.density_grid[0] == -1).numpy()
    MU.assert_same_marks(got, case["unseen"], case["border"], "restatement vs reference")
    assert r.untrained_cells.dtype == torch.int32 and np.array_equal(r.untrained_cells.numpy(), got.sum(axis=1))
    assert (np.abs(r.untrained_cells.numpy() - case["marked"]) <= case["border"].sum(axis=1)).all()
    share = got.mean(axis=1)
    assert ((share == 1).all() if case["poses"].shape[0] == 1 else ((share > 0.3) & (share < 0.95)).all()), share


def test_every_slice_gets_the_same_marks_and_seen_cells_keep_their_values(marked):
    _, r, before = marked
    unseen = r.density_grid[0] == -1
    for t in range(r.density_grid.shape[0]):
        assert torch.equal(r.density_grid[t] == -1, unseen)
        assert torch.equal(r.density_grid[t][~unseen], before[t][~unseen])


def test_numpy_poses_and_batching():
    case = MU.load_case("bound2")
    a, b = _renderer(2, slices=1), _renderer(2, slices=1)
    a.mark_untrained_grid(torch.from_numpy(case["poses"]), case["intrinsic"])
    b.mark_untrained_grid(case["poses"], np.array(case["intrinsic"]), S=32)      # numpy in; S only changes the batching
    assert torch.equal(a.density_grid, b.density_grid) and torch.equal(a.untrained_cells, b.untrained_cells)
    c = _renderer(2, slices=1)
    c.mark_untrained_grid(case["poses"].astype(np.float64), case["intrinsic"])          # fp64 poses (a transforms.json) are taken as fp32
    assert torch.equal(a.density_grid, c.density_grid)


def test_without_cuda_ray_is_a_no_op():
    r = _renderer(1, cuda_ray=False)
    assert r.mark_untrained_grid(MU.case_poses("bound1"), MU.INTRINSIC) is None
    assert not hasattr(r, "density_grid") and not hasattr(r, "untrained_cells")


def test_seald_renderers_inherit_the_method():
    from dnerf_amd.renderer import NeRFRenderer
    from dnerf_amd.seald import SealDNeRFStudent, SealDNeRFTeacher
    assert SealDNeRFTeacher.mark_untrained_grid is NeRFRenderer.mark_untrained_grid
    assert SealDNeRFStudent.mark_untrained_grid is NeRFRenderer.mark_untrained_grid
