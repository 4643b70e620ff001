"""NOT a test module: the numpy restatement of a placed object's cull (csrc/fixedcull.hip foc_fixed_cull_placed, include/focnerf.h), in
the style of tests/fixed_cull_ref.py and on top of it, shared by tests/test_placement_ref.py (CPU) and tests/test_gpu_placement.py.

    object-frame point   q_k = ((A_k0 x + A_k1 y) + A_k2 z) + b_k in float32, in this order, every product and sum rounded on its own;
                         q is not clamped
    inside               obj_aabb_lo <= q <= obj_aabb_hi on all three axes (False for a NaN)
    occupied             inside && bit(cell(q)) with fixed_cull_ref.cell_index / occupied on q
    direction            dir_scale * ((A_k0 dx + A_k1 dy) + A_k2 dz), float32, per ray, not renormalised

The 12 coefficients come from `focnerf_amd.Placement.world_to_object()`; `world_to_object64` states them a second way (the inverse of the
4x4 object -> world matrix) for the algebra tests. `rays`, `boxes` and `placements` are the inputs both test files use.
"""
import numpy as np

import fixed_cull_ref as ref

f32 = np.float32


def to_object(w2o, xyz):
    """w2o float32 [12] (A row-major, then b), xyz float32 [...,3] -> q float32 [...,3]."""
    w = np.asarray(w2o, dtype=f32)
    p = np.asarray(xyz, dtype=f32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [(((w[3 * k] * x).astype(f32) + (w[3 * k + 1] * y).astype(f32)).astype(f32) + (w[3 * k + 2] * z).astype(f32)).astype(f32) + w[9 + k]
             for k in range(3)]
    return np.stack(q, -1).astype(f32)


def to_object_dir(w2o, dir_scale, d):
    """The emitted direction: float32 [...,3]."""
    w = np.asarray(w2o, dtype=f32)
    d = np.asarray(d, dtype=f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    r = [f32(dir_scale) * (((w[3 * k] * x).astype(f32) + (w[3 * k + 1] * y).astype(f32)).astype(f32) + (w[3 * k + 2] * z).astype(f32)).astype(f32)
         for k in range(3)]
    return np.stack(r, -1).astype(f32)


def inside(q, obj_aabb):
    box = np.asarray(obj_aabb, dtype=f32)
    with np.errstate(invalid="ignore"):
        return ((q >= box[:3]) & (q <= box[3:])).all(-1)


def norm(q, bound):
    """fs_norm: (q + bound) / (2 bound) in float32."""
    return ((np.asarray(q, f32) + f32(bound)).astype(f32) / f32(2 * bound)).astype(f32)


def occupied(xyz_world, w2o, obj_aabb, bitfield, bound, cascade, H):
    """World samples float32 [...,3] -> (occupied bool [...], inside bool [...], q float32 [...,3])."""
    q = to_object(w2o, xyz_world)
    ins = inside(q, obj_aabb)
    idx, _, _ = ref.cell_index(np.where(ins[..., None], q, f32(0)), bound, cascade, H)
    return ins & ref.occupied(idx, bitfield), ins, q


def world_to_object64(P):
    """float64 [12] from the inverse of the object -> world matrix of x_world = s R (x_obj - pivot) + pivot + translation."""
    M = np.eye(4)
    M[:3, :3] = P.scale * P.rotation
    M[:3, 3] = P.pivot + P.translation - M[:3, :3] @ P.pivot
    inv = np.linalg.inv(M)
    return np.concatenate([inv[:3, :3].reshape(-1), inv[:3, 3]])


# ---------------------------------------------------------------- the inputs of the tests
BOXES = [(2, 1, 1), (4, 2, 2)]                      # (scene bound, object bound, object cascade)
SHAPES_N, SHAPES_T = (1, 63, 65, 130), (2, 3, 65)


def placements(SB):
    """name -> Placement, in units of the scene bound."""
    from focnerf_amd import Placement
    return {
        "identity": Placement(),
        "shift": Placement(translation=(0.4 * SB, -0.3 * SB, 0.2 * SB)),
        "quarter": Placement.rotated((0, 0, 1), 90),
        "small": Placement.rotated((1, 2, 3), 37, translation=(0.3 * SB, 0.1 * SB, -0.2 * SB), scale=0.5),
        "large": Placement.rotated((3, -1, 2), 110, translation=(-0.2 * SB, 0.2 * SB, 0.1 * SB), scale=1.25),
    }


def rays(N, SB, centre, seed=0):
    """N rays as float32 (o [N,3], d [N,3]): origins on the sphere of radius 1.5 SB around `centre` (the object's world centre), aimed at
    the centre plus a seeded jitter of at most 0.1 SB, directions of unit length."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, dtype=np.float64)
    u = rng.normal(size=(N, 3))
    o = c + 1.5 * SB * u / np.linalg.norm(u, axis=-1, keepdims=True)
    j = rng.normal(size=(N, 3))
    j = j / np.linalg.norm(j, axis=-1, keepdims=True) * (0.1 * SB * rng.random((N, 1)))
    d = c + j - o
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(f32), d.astype(f32)


def near_far64(o, d, SB, min_near=0.2):
    """Slab test of the rays against [-SB, SB]^3 in float64 -> (near [N], far [N], hit bool [N])."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-SB - o) / d, (SB - o) / d
    lo, hi = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    return np.maximum(lo, min_near), hi, lo <= hi


def samples64(o, d, near, far, T, SB):
    """The T fixed-step positions of every ray in float64, clamped to the scene box: [N,T,3]."""
    z = near[:, None] + (far - near)[:, None] * np.linspace(0.0, 1.0, T)[None, :]
    x = o.astype(np.float64)[:, None, :] + d.astype(np.float64)[:, None, :] * z[..., None]
    return np.clip(x, -SB, SB)


def inside_share64(P, N, T, SB, OB, seed=0):
    """Share of the N * T samples of `rays(N, SB, P.translation)` whose object-frame point lies in [-OB, OB]^3, all in float64."""
    o, d = rays(N, SB, P.translation, seed)
    near, far, hit = near_far64(o, d, SB)
    assert hit.all()
    x = samples64(o, d, near, far, T, SB)
    w = world_to_object64(P)
    q = x @ w[:9].reshape(3, 3).T + w[9:]
    return float((np.abs(q) <= OB).all(-1).mean())
