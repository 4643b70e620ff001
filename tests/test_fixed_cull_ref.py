"""CPU: the numpy reference of the occupancy cull (tests/fixed_cull_ref.py) against brute-force loops and the project's host-side Morton /
packbits helpers, and the argument checks of `fixedcull.Occupancy` / `render_field4(..., occupancy=)` on CPU tensors (they run before
anything touches a GPU)."""
import numpy as np
import pytest
import torch

import fixed_cull_ref as ref

H = 128


def _positions(n, bound, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-bound, bound, (n, 3)).astype(np.float32)
    # the edges: box faces and corners (clipped samples), the origin, the inner cascade's faces, exact cell boundaries
    edge = np.array([[bound, bound, bound], [-bound, -bound, -bound], [0, 0, 0], [1, 0.5, -0.25], [-1, 1, 1], [0.5, 0.5, 0.5],
                     [bound, -0.3, 0.1], [2.0 ** -7, -2.0 ** -7, 0], [1 - 2.0 ** -20, 0, 0]], np.float32)
    return np.concatenate([x, np.clip(edge, -bound, bound)])


@pytest.mark.parametrize("bound,cascade", [(1, 1), (2, 2)])
def test_cell_index_against_a_scalar_loop_and_the_host_morton(bound, cascade):
    from focnerf_amd import synthetic
    import math
    xyz = _positions(200, bound, 3)
    idx, level, n = ref.cell_index(xyz, bound, cascade, H)
    for k in range(xyz.shape[0]):
        x = [float(v) for v in xyz[k]]
        mx = max(abs(v) for v in x)
        lv = min(cascade - 1, max(0, math.frexp(mx)[1]))
        mb = min(2.0 ** lv, float(bound))
        nk = [int(min(max(np.float32(0.5 * float(np.float32(np.float32(v / mb) + np.float32(1))) * H), 0), H - 1)) for v in x]
        assert lv == level[k] and nk == list(n[k])
        assert idx[k] == lv * H ** 3 + int(synthetic.morton3D_host(torch.tensor([nk]))[0])
    assert idx.min() >= 0 and idx.max() < cascade * H ** 3
    if cascade == 2:
        assert (level == 0).any() and (level == 1).any()
        assert level[np.abs(xyz).max(-1) == 1.0].min() == 1          # |x| = 1 = 0.5 * 2^1: the outer cascade, as mip_from_pos has it


@pytest.mark.parametrize("bound,cascade", [(1, 1), (2, 2)])
def test_occupied_reads_the_bits_packbits_writes(bound, cascade):
    from focnerf_amd import synthetic
    xyz = _positions(300, bound, 5)
    idx, _, _ = ref.cell_index(xyz, bound, cascade, H)
    cells = cascade * H ** 3
    assert ref.occupied(idx, np.full(cells // 8, 255, np.uint8)).all()             # all ones: everything marked
    assert not ref.occupied(idx, np.zeros(cells // 8, np.uint8)).any()             # all zero: nothing marked
    grid = torch.zeros(cascade, H ** 3)
    chosen = idx[::7]
    grid.view(-1)[torch.from_numpy(chosen)] = 1.0
    bits = synthetic.packbits_host(grid, 0.5).numpy()
    assert np.array_equal(ref.occupied(idx, bits), np.isin(idx, chosen))
    assert int(np.unpackbits(bits).sum()) == len(set(chosen.tolist()))


def test_cull_against_a_brute_force_loop():
    N, T = 5, 7
    occ = np.random.default_rng(1).random((N, T)) < 0.5
    mask, offsets, order = ref.cull(occ)
    R = T                                                             # one ray block
    assert mask.shape == (R,) and offsets.shape == (R + 1,)
    want_order, want_mask, want_off = [], [], [0]
    for i in range(T):
        m = 0
        for n in range(64):
            if n < N and occ[n, i]:
                m |= 1 << n
                want_order.append((n, i))
        want_mask.append(m)
        want_off.append(want_off[-1] + bin(m).count("1"))
    assert [int(v) for v in mask] == want_mask and [int(v) for v in offsets] == want_off
    assert [tuple(v) for v in order.tolist()] == want_order
    for slot, (n, i) in enumerate(want_order):
        row = (n // 64) * T + i
        assert slot == int(offsets[row]) + bin(int(mask[row]) & ((1 << (n % 64)) - 1)).count("1")


def test_cull_over_several_blocks_all_ones_and_all_zero():
    N, T = 130, 3
    mask, offsets, order = ref.cull(np.ones((N, T), bool))
    assert offsets[-1] == N * T and len(order) == N * T
    assert [int(v) for v in mask] == [2 ** 64 - 1] * 6 + [3] * 3      # blocks 0 and 1 full, block 2 holds rays 128 and 129 only
    rows = [ref.blocked_row(n, i, T) for n, i in order]
    assert rows == sorted(rows)                                       # the compact order is the block-interleaved order
    mask, offsets, order = ref.cull(np.zeros((N, T), bool))
    assert not mask.any() and not offsets.any() and len(order) == 0


# ---------------------------------------------------------------- argument checks (no GPU)
def _net(bound=1, cuda_ray=False):
    from focnerf_amd.network import NeRFNetwork
    return NeRFNetwork(bound=bound, cuda_ray=cuda_ray).eval()


def test_occupancy_of_refuses_a_missing_or_empty_grid():
    from focnerf_amd.fixedcull import Occupancy
    with pytest.raises(ValueError, match="no occupancy grid"):
        Occupancy.of(_net(1, cuda_ray=False))
    m = _net(2, cuda_ray=True)
    with pytest.raises(ValueError, match="all zero"):
        Occupancy.of(m)
    m.density_bitfield[5] = 4
    occ = Occupancy.of(m)
    assert (occ.cascade, occ.grid_size, occ.bound) == (2, 128, 2.0)
    assert occ.bitfield.data_ptr() == m.density_bitfield.data_ptr()   # no copy


def test_occupancy_refuses_a_bitfield_of_another_grid():
    from focnerf_amd.fixedcull import Occupancy
    with pytest.raises(ValueError, match="does not describe"):
        Occupancy(torch.zeros(100, dtype=torch.uint8), 1, 128, 1)
    with pytest.raises(ValueError, match="uint8"):
        Occupancy(torch.zeros(128 ** 3 // 8), 1, 128, 1)
    with pytest.raises(ValueError, match="power-of-two"):
        Occupancy(torch.zeros(100 ** 3 // 8, dtype=torch.uint8), 1, 100, 1)


def test_render_field4_refuses_what_the_culled_path_does_not_serve(monkeypatch):
    from focnerf_amd.fixedcull import Occupancy
    from focnerf_amd.fixedstep import render_field4
    m = _net(1)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    ones = lambda c: torch.full((c * 128 ** 3 // 8,), 255, dtype=torch.uint8)
    with pytest.raises(ValueError, match="bound"):
        render_field4(m, o, d, num_steps=8, occupancy=Occupancy(ones(2), 2, 128, 2))
    with pytest.raises(ValueError, match="Occupancy"):
        render_field4(m, o, d, num_steps=8, occupancy=ones(1))
    monkeypatch.setenv("FOC_FUSED_INFER", "0")                        # no fused inference: refused, never rendered dense behind the caller's back
    with pytest.raises(ValueError, match="fused inference"):
        render_field4(m, o, d, num_steps=8, occupancy=Occupancy(ones(1), 1, 128, 1))
