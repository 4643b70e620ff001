"""Connected components of a thresholded volume on the device (csrc/components.hip): meshes and occupancy grids without floaters.

A trained density field almost always carries small detached blobs above the threshold. The reference hands its marching-cubes result to
trimesh, where a user calls `split()` and keeps the largest part; here the lattice never leaves the device:

    c = label_components(vol, 10.0)                                    # c.labels int32 [nx,ny,nz], c.sizes, c.first, c.count
    vol = filter_components(vol, 10.0, keep_largest=1)                 # every other component's points read `fill` (0.0)
    v, f = extract_geometry(model, 256, 10.0, keep_largest=1)          # mesh.py applies it between the volume and the marching cubes
    occ = Occupancy.of(model).pruned(keep_largest=1)                   # fixedcull.py: the same per cascade of an occupancy bitfield

A point is inside iff u >= threshold (a NaN is outside: `marching_cubes`' rule) and two inside points are connected when they differ by
at most 1 in every coordinate (26-connectivity). The eight corners of a marching cube are mutually adjacent, so every inside corner of a
cube lies in one component: filling a component below the threshold removes exactly its triangles, and every other vertex and triangle
keeps its bits. Components are numbered by their first lattice point in linear order — `scipy.ndimage.label`'s numbering minus one with
a full 3 x 3 x 3 structure. The same bits on every run and in both deterministic modes.
"""
from dataclasses import dataclass

import torch

from ._lib import lib, ptr, stream_of, check
from .backend import _scratch


@dataclass
class Components:
    """labels int32 [nx,ny,nz]: -1 outside, else the dense id 0..K-1 of the point's component (numbered by first lattice point); sizes
    int64 [K] point counts; first int64 [K] each component's smallest linear index (its root); count = K. `roots` int32 [nx,ny,nz] is
    the kernel's own labelling: the root's linear index, -1 outside."""
    labels: torch.Tensor
    sizes: torch.Tensor
    first: torch.Tensor
    count: int
    roots: torch.Tensor


def _check_volume(who, volume):
    if not torch.is_tensor(volume) or not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() != 3:
        raise ValueError(f"{who}: a float32 CUDA tensor [nx,ny,nz] expected")


def _label(who, volume, threshold):
    """-> (roots int32 [nx,ny,nz], root_sizes int32 [n], K, inside, largest) after the ONE host read (counts4: K and the error flag)."""
    nx, ny, nz = volume.shape
    dev = volume.device
    nbytes = lib.foc_cc_workspace_bytes(nx, ny, nz)
    if nbytes == 0:
        raise ValueError(f"{who}: " + lib.foc_last_error().decode("utf-8", "replace"))
    workspace = _scratch.get("components", nbytes, dev)
    roots = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
    root_sizes = torch.empty(nx * ny * nz, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib.foc_cc_label(ptr(volume), nx, ny, nz, float(threshold), ptr(roots), ptr(root_sizes), ptr(workspace), nbytes, ptr(counts),
                           stream_of(volume)), "cc_label")
    K, inside, largest, err = (int(v) & 0xFFFFFFFF for v in counts.tolist())
    if err:
        raise RuntimeError(f"{who}: a union-find loop reached its iteration cap (foc_cc_label's error flag); the labels are not valid")
    return roots, root_sizes, K, inside, largest


def label_components(volume, threshold):
    """The connected components (26-connectivity) of the points u >= threshold of a float32 device tensor u[nx,ny,nz] -> `Components`.
    The kernels give every point its component's smallest linear index; the dense renumbering is torch. One host read (K, with the
    kernels' error flag: RuntimeError when a loop hit its cap)."""
    _check_volume("label_components", volume)
    volume = volume.contiguous()
    roots, root_sizes, K, _, _ = _label("label_components", volume, threshold)
    is_root = root_sizes > 0
    first = torch.nonzero(is_root).view(-1)                              # ascending: the order of first lattice points
    rank = torch.cumsum(is_root, 0) - 1                                  # dense id of a root at the root's index
    flat = roots.view(-1).long()
    labels = torch.where(flat >= 0, rank[flat.clamp_min(0)], flat).to(torch.int32).view(volume.shape)
    assert first.numel() == K
    return Components(labels, root_sizes[first].long(), first, K, roots)


def keep_mask(sizes, keep_largest=None, min_voxels=None):
    """bool [K] over components numbered by first point: the first `keep_largest` in the order (size descending, first point ascending)
    and / or those with sizes >= min_voxels; with both given a component must pass both."""
    if keep_largest is None and min_voxels is None:
        raise ValueError("filter_components: give keep_largest and / or min_voxels")
    keep = torch.ones(sizes.numel(), dtype=torch.bool, device=sizes.device)
    if keep_largest is not None:
        k = int(keep_largest)
        if k < 1 or k != keep_largest:
            raise ValueError(f"filter_components: keep_largest must be an integer >= 1 (got {keep_largest!r})")
        order = torch.sort(sizes, descending=True, stable=True).indices  # stable: equal sizes stay in the order of their first points
        top = torch.zeros_like(keep)
        top[order[:k]] = True
        keep &= top
    if min_voxels is not None:
        m = int(min_voxels)
        if m < 1 or m != min_voxels:
            raise ValueError(f"filter_components: min_voxels must be an integer >= 1 (got {min_voxels!r})")
        keep &= sizes >= m
    return keep


def filter_components(volume, threshold, keep_largest=None, min_voxels=None, fill=0.0, out=None):
    """`volume` with every component that is not kept set to `fill` (< threshold: such a point is then outside).
    keep_largest=k keeps the first k components in the order (size descending, first point ascending); min_voxels=m keeps sizes >= m;
    with both a component must pass both; with neither: ValueError. The input itself is returned when nothing is removed; otherwise a
    new tensor, or `out` (which may be `volume`: in place)."""
    if keep_largest is None and min_voxels is None:
        raise ValueError("filter_components: give keep_largest and / or min_voxels")
    fill, threshold = float(fill), float(threshold)
    if not fill < threshold:
        raise ValueError(f"filter_components: fill must be < threshold (got fill {fill}, threshold {threshold})")
    _check_volume("filter_components", volume)
    if out is not None and (not torch.is_tensor(out) or out.shape != volume.shape or out.dtype != volume.dtype or out.device != volume.device
                            or not out.is_contiguous() or not volume.is_contiguous()):
        raise ValueError("filter_components: out must be a contiguous tensor like the (contiguous) volume")
    src = volume.contiguous()
    roots, root_sizes, K, _, _ = _label("filter_components", src, threshold)
    first = torch.nonzero(root_sizes > 0).view(-1)
    keep_k = keep_mask(root_sizes[first].long(), keep_largest, min_voxels)
    if bool(keep_k.all()):                                               # nothing to remove (K == 0 included)
        if out is not None and out.data_ptr() != volume.data_ptr():
            out.copy_(volume)
            return out
        return volume
    keep = torch.zeros(src.numel(), dtype=torch.uint8, device=src.device)
    keep[first[keep_k]] = 1
    res = torch.empty_like(src) if out is None else out
    check(lib.foc_cc_select(ptr(src), ptr(roots), ptr(keep), fill, ptr(res), src.numel(), stream_of(src)), "cc_select")
    return res
