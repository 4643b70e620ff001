"""CPU: `focnerf_amd.Placement` (focnerf_amd/placement.py) against float64 algebra, its refusals, the refusal of `render_field4` that needs
no device, and the input condition of tests/test_gpu_placement.py checked on the reference alone (tests/placement_ref.py)."""
import numpy as np
import pytest

import placement_ref as pr


def _all_placements():
    return [(SB, name, P) for SB, _, _ in pr.BOXES for name, P in pr.placements(SB).items()]


# ---------------------------------------------------------------- algebra
def test_world_to_object_is_the_float64_inverse_rounded_once():
    for SB, name, P in _all_placements():
        w32, w64 = P.world_to_object(), pr.world_to_object64(P)
        assert w32.dtype == np.float32 and w32.shape == (12,)
        # one rounding to fp32 (relative 2^-24) of a float64 value the two float64 routes agree on to ~1e-15
        assert (np.abs(w32.astype(np.float64) - w64) <= 2.0 ** -24 * np.abs(w64) + 1e-14).all(), (SB, name)
        assert float(P.dir_scale) == float(np.float32(P.scale)) and float(P.sigma_gain) == float(np.float32(1.0 / P.scale))
        assert P.dir_scale.dtype == np.float32 and P.sigma_gain.dtype == np.float32


def test_world_to_object_composed_with_object_to_world_is_the_identity():
    rng = np.random.default_rng(1)
    x = rng.uniform(-3, 3, size=(64, 3))
    for SB, name, P in _all_placements():
        M, t = P.object_to_world()
        A, b = P.world_to_object64()
        assert np.abs((x @ M.T + t) @ A.T + b - x).max() < 1e-12, (SB, name)
        assert np.abs(A @ M - np.eye(3)).max() < 1e-14 and np.abs(A @ t + b).max() < 1e-14
        # the stated formula, term by term
        want = P.scale * (x - P.pivot) @ P.rotation.T + P.pivot + P.translation
        assert np.abs(x @ M.T + t - want).max() < 1e-12


def test_pivot_is_the_point_rotation_and_scale_hold_fixed():
    from focnerf_amd import Placement
    pivot, tr = np.array([0.3, -0.2, 0.5]), np.array([1.0, 2.0, -1.0])
    P = Placement.rotated((1, 1, 0), 73, translation=tr, scale=1.7, pivot=pivot)
    M, t = P.object_to_world()
    assert np.abs(M @ pivot + t - (pivot + tr)).max() < 1e-14
    A, b = P.world_to_object64()
    assert np.abs(A @ (pivot + tr) + b - pivot).max() < 1e-14
    # without a pivot the origin is the fixed point
    P0 = Placement.rotated((1, 1, 0), 73, translation=tr, scale=1.7)
    assert np.abs(P0.object_to_world()[1] - tr).max() == 0


def test_rotated_is_the_axis_angle_rotation():
    from focnerf_amd import Placement
    for axis, deg in [((1, 2, 3), 37), ((3, -1, 2), 110), ((0, 0, 1), 90), ((0, 1, 0), -45), ((2, 0, 0), 180)]:
        R = Placement.rotated(axis, deg).rotation
        k = np.asarray(axis, float) / np.linalg.norm(axis)
        assert np.abs(R @ k - k).max() < 1e-15                       # the axis stays
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        assert abs(np.trace(R) - (1 + 2 * np.cos(np.radians(deg)))) < 1e-15
        v = np.cross(k, [0.3, 0.5, -0.7])                            # perpendicular to the axis: turns by the angle, right-handed
        assert abs(np.dot(np.cross(v, R @ v), k) - np.dot(v, v) * np.sin(np.radians(deg))) < 1e-15
    # quarter turns about a coordinate axis are exact signed permutations
    assert np.array_equal(Placement.rotated((0, 0, 1), 90).rotation, np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]))
    assert np.array_equal(Placement.rotated((0, 0, 5), 270).rotation, np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]]))
    assert np.array_equal(Placement.rotated((1, 0, 0), 360).rotation, np.eye(3))
    w = Placement.rotated((0, 0, 1), 90).world_to_object()
    assert np.array_equal(w, np.array([0, 1, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0], np.float32))


def test_identity_gives_exactly_I_0_1_1():
    from focnerf_amd import Placement
    for P in (Placement(), Placement(rotation=np.eye(3), pivot=(0.3, 0.1, -0.7)), Placement.rotated((1, 2, 3), 0)):
        w = P.world_to_object()
        assert np.array_equal(w, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)) and not np.signbit(w).any()
        assert P.dir_scale == np.float32(1) and P.sigma_gain == np.float32(1)


# ---------------------------------------------------------------- refusals
def test_every_refusal_names_the_offending_value():
    from focnerf_amd import Placement
    with pytest.raises(ValueError, match=r"max \|R\^T R - I\| = .*> 1e-5"):
        Placement(rotation=np.eye(3) * (1 + 1e-5))                    # R^T R - I = 2e-5
    Placement(rotation=np.eye(3) * (1 + 2e-6))                        # 4e-6: within the bound
    with pytest.raises(ValueError, match=r"not orthonormal"):
        Placement(rotation=[[1, 0.01, 0], [0, 1, 0], [0, 0, 1]])      # a shear
    with pytest.raises(ValueError, match=r"determinant -1.* \(a reflection\)"):
        Placement(rotation=np.diag([1.0, 1.0, -1.0]))
    for bad in (0, 0.0, -1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match=r"scale must be finite and > 0, got"):
            Placement(scale=bad)
        with pytest.raises(ValueError, match=r"scale must be finite and > 0, got"):
            Placement.rotated((0, 0, 1), 30, scale=bad)
    for bad in (float("nan"), float("inf")):
        R = np.eye(3)
        R[1, 2] = bad
        with pytest.raises(ValueError, match=r"rotation has a non-finite entry"):
            Placement(rotation=R)
        with pytest.raises(ValueError, match=r"translation has a non-finite entry"):
            Placement(translation=(0, bad, 0))
        with pytest.raises(ValueError, match=r"pivot has a non-finite entry"):
            Placement(pivot=(bad, 0, 0))
        with pytest.raises(ValueError, match=r"non-finite"):
            Placement.rotated((0, bad, 1), 30)
        with pytest.raises(ValueError, match=r"degrees must be finite"):
            Placement.rotated((0, 0, 1), bad)
    with pytest.raises(ValueError, match=r"axis must not be zero"):
        Placement.rotated((0, 0, 0), 30)
    with pytest.raises(ValueError, match=r"3x3"):
        Placement(rotation=np.eye(4))
    with pytest.raises(ValueError, match=r"3 entries"):
        Placement(translation=(1, 2))


def test_render_field4_refuses_a_placement_without_occupancy_before_touching_a_device():
    import torch
    from focnerf_amd import Placement
    from focnerf_amd.fixedstep import render_field4
    o, d = torch.zeros(4, 3), torch.ones(4, 3)                        # host tensors and no model: nothing but the refusal can run
    with pytest.raises(ValueError, match=r"placement needs occupancy=.*Occupancy\.of\(model\).*Occupancy\.estimate\(model\)"):
        render_field4(None, o, d, num_steps=8, placement=Placement())
    with pytest.raises(ValueError, match=r"scene_aabb belongs to a placement"):
        render_field4(None, o, d, num_steps=8, scene_aabb=torch.tensor([-2.0] * 3 + [2.0] * 3))


# ---------------------------------------------------------------- the reference itself
def test_reference_map_keeps_the_stated_order_and_is_the_identity_at_identity():
    from focnerf_amd import Placement
    rng = np.random.default_rng(3)
    x = rng.uniform(-2, 2, size=(500, 3)).astype(np.float32)
    assert np.array_equal(pr.to_object(Placement().world_to_object(), x), x)
    assert np.array_equal(pr.to_object_dir(Placement().world_to_object(), 1.0, x), x)
    for SB, name, P in _all_placements():
        w = P.world_to_object()
        q = pr.to_object(w, x)
        A, b = w[:9].astype(np.float64).reshape(3, 3), w[9:].astype(np.float64)
        exact = x.astype(np.float64) @ A.T + b
        # three roundings of partial sums of magnitude <= sum |A_kj x_j| + |b_k|, three of products: 6 * 2^-24 of that magnitude
        mag = np.abs(x.astype(np.float64)) @ np.abs(A).T + np.abs(b)
        assert (np.abs(q - exact) <= 6 * 2.0 ** -24 * mag).all(), (SB, name)
        # ((a + b) + c) + t, not a + (b + (c + t)): the first row by hand on one point
        p = x[7]
        by_hand = np.float32(np.float32(np.float32(w[0] * p[0]) + np.float32(w[1] * p[1])) + np.float32(w[2] * p[2])) + w[9]
        assert q[7, 0] == by_hand
    box = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    pts = np.array([[1, 1, 1], [-1, 0, 1], [1.0000001, 0, 0], [0, -1.0000001, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    assert pr.inside(pts, box).tolist() == [True, True, False, False, False, True]          # closed on both faces, False for a NaN


@pytest.mark.parametrize("SB,OB,C", pr.BOXES)
def test_input_condition_of_the_gpu_test_between_a_fifth_and_seven_tenths_inside(SB, OB, C):
    """With an all-ones grid the GPU test's occupied count is its inside count: neither "nothing" nor "everything" for every non-identity
    placement at T = 65 (float64 near / far and positions; the shares are 0.25 .. 0.65)."""
    for name, P in pr.placements(SB).items():
        if name == "identity":
            continue
        for N in (63, 65, 130):
            share = pr.inside_share64(P, N, 65, SB, OB)
            assert 0.2 <= share <= 0.7, (name, N, share)
