"""Where an object stands in a scene: rotation, uniform scale and translation of a per-object network in the combined render.

    x_world = s * R @ (x_obj - pivot) + pivot + translation

The occupancy-culled field path (`fixedstep.render_field4(..., occupancy=occ, placement=P)`, csrc/fixedcull.hip) keeps the view's own
sample positions — the per-sample select needs every object at the same T positions of the same rays — and maps each position into the
object's frame in front of the cell test: q = A x + b with A = R^T / s. Samples outside the object's own box are empty, the encoder and
the networks see q and the turned direction, and the density is rescaled by 1 / s (the object's density per unit of WORLD length).

    P = Placement.rotated((0, 0, 1), 30, translation=(0.5, 0, 0), scale=0.5)
    render_field4(model, rays_o, rays_d, num_steps=T, occupancy=occ, placement=P, scene_aabb=scene_box)
"""
import math

import numpy as np


def _vec3(name, v):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,):
        raise ValueError(f"Placement: {name} must have 3 entries, got {v!r}")
    if not np.isfinite(a).all():
        raise ValueError(f"Placement: {name} has a non-finite entry: {a.tolist()}")
    return a


class Placement:
    """Object -> world: x_world = scale * rotation @ (x_obj - pivot) + pivot + translation. `rotation` is a proper rotation (3x3
    array-like, default the identity), `scale` a finite number > 0, `pivot` the point of the object's frame the rotation and the scale
    hold fixed. Everything is kept in float64; the kernels' coefficients are rounded to fp32 once (`world_to_object`)."""

    def __init__(self, rotation=None, translation=(0, 0, 0), scale=1.0, pivot=(0, 0, 0)):
        R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64)
        if R.shape != (3, 3):
            raise ValueError(f"Placement: rotation must be 3x3, got shape {R.shape}")
        if not np.isfinite(R).all():
            raise ValueError(f"Placement: rotation has a non-finite entry: {R.tolist()}")
        err = float(np.abs(R.T @ R - np.eye(3)).max())
        if err > 1e-5:
            raise ValueError(f"Placement: rotation is not orthonormal: max |R^T R - I| = {err:g} > 1e-5")
        det = float(np.linalg.det(R))
        if det < 0:
            raise ValueError(f"Placement: rotation has determinant {det:g} < 0 (a reflection)")
        try:
            s = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"Placement: scale must be a number, got {scale!r}") from None
        if not math.isfinite(s) or s <= 0:
            raise ValueError(f"Placement: scale must be finite and > 0, got {s!r}")
        self.rotation, self.scale = R, s
        self.translation, self.pivot = _vec3("translation", translation), _vec3("pivot", pivot)

    @classmethod
    def rotated(cls, axis, degrees, **kw):
        """A rotation by `degrees` about `axis` (any non-zero length; Rodrigues' formula in float64). Whole multiples of 90 degrees use
        the exact sines and cosines 0 and +-1, so a quarter turn about a coordinate axis is a signed permutation matrix."""
        k = _vec3("axis", axis)
        n = float(np.linalg.norm(k))
        if n == 0:
            raise ValueError(f"Placement.rotated: axis must not be zero, got {k.tolist()}")
        deg = float(degrees)
        if not math.isfinite(deg):
            raise ValueError(f"Placement.rotated: degrees must be finite, got {deg!r}")
        k = k / n
        quarter = deg / 90.0
        if quarter == round(quarter):
            c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(round(quarter)) % 4]
        else:
            c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        R = c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k)
        return cls(rotation=R, **kw)

    def object_to_world(self):
        """(M [3,3], t [3]) float64 with x_world = M x_obj + t."""
        M = self.scale * self.rotation
        return M, self.pivot + self.translation - M @ self.pivot

    def world_to_object64(self):
        """(A [3,3], b [3]) float64 with x_obj = A x_world + b: A = R^T / s, b = pivot - A (pivot + translation)."""
        A = self.rotation.T / self.scale
        return A, self.pivot - A @ (self.pivot + self.translation)

    def world_to_object(self):
        """The 12 coefficients the kernels take: A row-major, then b, computed in float64 and rounded once to float32 (numpy [12])."""
        A, b = self.world_to_object64()
        return np.concatenate([A.reshape(-1), b]).astype(np.float32) + np.float32(0)      # + 0: no negative zeros in the coefficients

    @property
    def dir_scale(self):
        """Factor of the emitted direction (A d has length 1 / s): s, rounded once to float32."""
        return np.float32(self.scale)

    @property
    def sigma_gain(self):
        """Factor of the object's density in the world's units of length: 1 / s, rounded once to float32."""
        return np.float32(1.0 / self.scale)

    def __repr__(self):
        return (f"Placement(rotation={self.rotation.tolist()}, translation={self.translation.tolist()}, scale={self.scale}, "
                f"pivot={self.pivot.tolist()})")
