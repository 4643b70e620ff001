"""`import mcubes` for the reference's `extract_geometry` (nerf/utils.py:536) when focnerf_amd/dropin is on the path: PyMCubes'
`marching_cubes(u, isovalue)` served by focnerf_amd.mesh on the device.

Takes a numpy array u[nx,ny,nz] and returns numpy (vertices float64 [V,3] in index units, triangles int64 [F,3]). The surface is the
piecewise-linear level set PyMCubes extracts; the order of vertices and triangles and the choice on ambiguous faces are this package's
(focnerf_amd/mesh.py), not PyMCubes' — that parity is not pinned. Triangles face the lower values. A trimesh stand-in is not provided."""
import numpy as np

__all__ = ["marching_cubes"]


def marching_cubes(u, isovalue):
    import torch
    from focnerf_amd import mesh
    if not torch.cuda.is_available():
        raise RuntimeError("mcubes (focnerf_amd drop-in): marching_cubes runs on the GPU; there is no CPU implementation")
    vol = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda()
    vertices, triangles = mesh.marching_cubes(vol, float(isovalue))
    return vertices.cpu().numpy().astype(np.float64), triangles.cpu().numpy().astype(np.int64)
