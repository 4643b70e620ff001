"""CPU: tests/components_ref.py — the numpy definition of the connected-component labelling — pinned against scipy.ndimage.label with a
full 3 x 3 x 3 structure, its mutants, the keep order, the subset property of a filtered volume's mesh, the Morton packing of
Occupancy.pruned, and the host-side refusals of foc_cc_label / foc_cc_select and focnerf_amd.components (no launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as cr                                              # noqa: E402
import mesh_ref                                                          # noqa: E402

SHAPES = [(3, 2, 5), (5, 7, 67), (65, 3, 2), (35, 19, 131)]
FRACTIONS = [0.05, 0.12, 0.5]


def _scipy_label(mask):
    from scipy import ndimage
    lab, K = ndimage.label(mask, structure=np.ones((3, 3, 3)))
    return lab.astype(np.int64) - 1, K


def _check_against_scipy(vol, thr):
    labels, sizes, first, roots = cr.label(vol, thr)
    with np.errstate(invalid="ignore"):
        mask = np.asarray(vol, dtype=np.float32) >= np.float32(thr)
    want, K = _scipy_label(mask)
    assert len(sizes) == len(first) == K
    assert np.array_equal(labels, want)                                  # scipy's numbering minus one
    assert np.array_equal(sizes, np.bincount(want[want >= 0], minlength=K))
    flat = want.reshape(-1)
    assert np.array_equal(first, [np.flatnonzero(flat == k)[0] for k in range(K)])
    assert np.array_equal(roots.reshape(-1)[flat >= 0], first[flat[flat >= 0]])
    return K


@pytest.mark.parametrize("shape", SHAPES[:3])
@pytest.mark.parametrize("fraction", FRACTIONS)
def test_random_volumes_against_scipy(shape, fraction):
    _check_against_scipy(cr.random_volume(shape, fraction, seed=sum(shape)), 1.0 - fraction)


def test_the_largest_random_volume_against_scipy():
    K = _check_against_scipy(cr.random_volume(SHAPES[3], 0.12, seed=1), 0.88)
    assert K > 100


def test_corner_patterns_special_values_and_paths_against_scipy():
    for case in range(256):
        assert _check_against_scipy(cr.corner_pattern(case), 0.5) == (1 if case else 0)       # the corners of a cube are mutually adjacent
    assert _check_against_scipy(cr.special_volume(), 0.5) == 2
    vol, length = cr.serpentine((9, 5, 12))
    labels, sizes, first, _ = cr.label(vol, 0.5)
    assert _check_against_scipy(vol, 0.5) == 1 and sizes.tolist() == [length]
    for d in cr.FORWARD_26:
        vol, p, q = cr.diagonal_pair((12, 12, 12), 4, d)
        labels, sizes, first, _ = cr.label(vol, 0.5)
        assert sizes.tolist() == [2] and first.tolist() == [min(p, q)] and _check_against_scipy(vol, 0.5) == 1


def test_serpentine_is_one_single_voxel_wide_path():
    vol, length = cr.serpentine()
    assert vol.shape == (33, 9, 70) and length > 33 // 2 * 5 * 70
    inside = vol > 0
    # single-voxel-wide: no 2 x 2 x 1 block (in any orientation) is full
    for a, b in ((0, 1), (0, 2), (1, 2)):
        full = np.ones([n - (k in (a, b)) for k, n in enumerate(vol.shape)], dtype=bool)
        for da in (0, 1):
            for db in (0, 1):
                s = [slice(None)] * 3
                s[a] = slice(da, vol.shape[a] - 1 + da)
                s[b] = slice(db, vol.shape[b] - 1 + db)
                full &= inside[tuple(s)]
        assert not full.any()
    assert _scipy_label(inside)[1] == 1


def _cases():
    """The volumes the GPU tests label, small enough to label with every mutant here: (volume, threshold)."""
    out = [(cr.corner_pattern(case), 0.5) for case in range(256)] + [(cr.special_volume(), 0.5)]
    out += [(cr.diagonal_pair((12, 12, 12), 4, d)[0], 0.5) for d in cr.FORWARD_26]
    return out


@pytest.mark.parametrize("mutant", [dict(directions=cr.FORWARD_6), dict(directions=cr.FORWARD_18), dict(strict=True), dict(nan_inside=True)],
                         ids=["6-connectivity", "18-connectivity", "greater-than", "nan-inside"])
def test_mutants_are_caught(mutant):
    caught = 0
    for vol, thr in _cases():
        good, bad = cr.label(vol, thr), cr.label(vol, thr, **mutant)
        caught += not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
    assert caught >= 1


def test_keep_order_and_rules():
    sizes, first = np.array([3, 7, 7, 1, 3]), np.array([0, 10, 20, 30, 40])
    assert cr.keep_order(sizes, first).tolist() == [1, 2, 0, 4, 3]      # ties: the earlier first point goes first
    assert cr.keep_mask(sizes, first, keep_largest=1).tolist() == [False, True, False, False, False]
    assert cr.keep_mask(sizes, first, keep_largest=3).tolist() == [True, True, True, False, False]
    assert cr.keep_mask(sizes, first, min_voxels=3).tolist() == [True, True, True, False, True]
    assert cr.keep_mask(sizes, first, keep_largest=4, min_voxels=7).tolist() == [False, True, True, False, False]
    assert cr.keep_mask(sizes, first, keep_largest=9).all()
    with pytest.raises(ValueError):
        cr.keep_mask(sizes, first)
    vol = np.zeros((2, 2, 9), dtype=np.float32)
    vol[0, 0, 0:2], vol[1, 1, 4:6], vol[0, 0, 8] = 1.0, 1.0, 1.0         # sizes 2, 2, 1
    out = cr.filter(vol, 0.5, keep_largest=1, fill=-3.0)
    assert out[0, 0, 0] == 1 and out[1, 1, 4] == -3 and out[0, 0, 8] == -3 and out[0, 1, 0] == 0


def test_filtered_mesh_is_a_subset_of_the_unfiltered_one():
    vol = mesh_ref.noise_volume(14, seed=3)
    thr = float(np.quantile(vol, 0.8))
    _, sizes, _, _ = cr.label(vol, thr)
    kept = cr.filter(vol, thr, min_voxels=4)
    assert len(sizes) == 2 and len(cr.label(kept, thr)[1]) == int((sizes >= 4).sum()) == 1        # K = 2: the body and a floater of 3 points
    v, f = mesh_ref.marching_cubes(vol, thr)
    w, g = mesh_ref.marching_cubes(kept, thr)
    assert (len(f), len(g)) == (4196, 4172)
    have = {tuple(v[t].reshape(-1).tolist()) for t in f}                 # a triangle: its nine coordinates, exactly
    assert all(tuple(w[t].reshape(-1).tolist()) in have for t in g)


def test_morton_packing_round_trip_and_pruned():
    rng = np.random.default_rng(5)
    C, H = 2, 8
    bits = rng.integers(0, 256, C * H ** 3 // 8, dtype=np.uint8)
    grid = cr.unpack_bitfield(bits, C, H)
    assert grid.shape == (C, H, H, H) and np.array_equal(cr.pack_bitfield(grid), bits)
    import fixed_cull_ref
    for c, x, y, z in [(0, 0, 0, 0), (0, 1, 0, 0), (1, 3, 5, 7), (1, 7, 7, 7)]:
        index = np.array(c * H ** 3 + int(fixed_cull_ref.morton3d(np.array([x, y, z]))))
        assert grid[c, x, y, z] == fixed_cull_ref.occupied(index, bits)
    sparse = cr.pack_bitfield(rng.random((C, H, H, H)) < 0.08)
    out = cr.pruned(sparse, C, H, keep_largest=1)
    a, b = cr.unpack_bitfield(sparse, C, H), cr.unpack_bitfield(out, C, H)
    assert (b <= a).all() and (b != a).any()
    for c in range(C):
        sizes = cr.label(a[c].astype(np.float32), 0.5)[1]
        assert len(sizes) > 1 and b[c].sum() == sizes.max() and len(cr.label(b[c].astype(np.float32), 0.5)[1]) == 1


def test_argument_validation_needs_no_gpu():
    """Null pointers, a small workspace, a non-finite threshold and a NaN fill are refused on the host before any launch; the Python
    layer refuses fill >= threshold and a call without a keep rule before it looks at the volume."""
    from focnerf_amd import _lib, components
    lib = _lib.lib
    one = ctypes.c_void_p(8)                                             # never dereferenced: validation fails first
    need = lib.foc_cc_workspace_bytes(5, 7, 67)
    assert need == 5 * 7 * 67 * 8
    assert lib.foc_cc_workspace_bytes(1, 7, 67) == 0 and b"every dimension" in lib.foc_last_error()
    assert lib.foc_cc_workspace_bytes(1024, 1024, 1024) == 0 and b"2^29" in lib.foc_last_error()
    for k in range(5):
        args = [one] * 5
        args[k] = None
        rc = lib.foc_cc_label(args[0], 5, 7, 67, 0.5, args[1], args[2], args[3], need, args[4], None)
        assert rc == 1 and b"cc_label: null pointer" in lib.foc_last_error()
    assert lib.foc_cc_label(one, 5, 1, 67, 0.5, one, one, one, need, one, None) == 1 and b"every dimension" in lib.foc_last_error()
    assert lib.foc_cc_label(one, 5, 7, 67, 0.5, one, one, one, need - 1, one, None) == 1 and b"workspace of" in lib.foc_last_error()
    for thr in (float("nan"), float("inf"), float("-inf")):
        assert lib.foc_cc_label(one, 5, 7, 67, thr, one, one, one, need, one, None) == 1 and b"thr must be finite" in lib.foc_last_error()
    for k in range(4):
        args = [one] * 4
        args[k] = None
        assert lib.foc_cc_select(args[0], args[1], args[2], 0.0, args[3], 16, None) == 1 and b"cc_select: null pointer" in lib.foc_last_error()
    assert lib.foc_cc_select(one, one, one, float("nan"), one, 16, None) == 1 and b"fill" in lib.foc_last_error()
    assert lib.foc_cc_select(one, one, one, 0.0, one, (1 << 29) + 1, None) == 1 and b"2^29" in lib.foc_last_error()
    with pytest.raises(ValueError, match="keep_largest and / or min_voxels"):
        components.filter_components(None, 0.5)
    for fill in (0.5, 1.0, float("nan")):
        with pytest.raises(ValueError, match="fill must be < threshold"):
            components.filter_components(None, 0.5, keep_largest=1, fill=fill)
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        components.filter_components(np.zeros((2, 2, 2)), 0.5, keep_largest=1)
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        components.label_components(None, 0.5)
