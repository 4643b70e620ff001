// components.hip — connected components of a thresholded float32 volume on the device (no reference binding: the reference hands its
// marching-cubes result to trimesh, where `split()` finds the floaters on the host).
//
//   foc_cc_label    labels[i] = the smallest linear index of i's component (26-connectivity; inside iff u >= thr, a NaN is outside),
//                   sizes[root] = the component's point count, counts4 = components, inside points, largest size, error flag
//   foc_cc_select   out[i] = fill where i's component is not kept, u[i] elsewhere
//
// Union-find with min-root links: parent[i] <= i ALWAYS, every value a word ever holds is an ancestor of i in i's own component, and a
// link goes from a root to a smaller index only. Hence (a) every chain strictly decreases: no walk can cycle, and the number of lattice
// points bounds every loop; (b) a read that is served stale returns an OLDER ancestor, which is still a correct place to go on from, and
// the atomicMin that links returns the word's true value: the loops below never wait for another thread's write, they only ever walk
// down; (c) the one root a component is left with is its smallest index, whatever order the unions ran in: the same bits on every run.
//
// Passes (one launch each; a launch boundary is the only ordering between them that anything relies on):
//   k_cc_tile     one workgroup per CC_TX x CC_TY x CC_TZ tile: union-find in LDS over the tile's inside points. Runs of inside points
//                 along z start joined (a ballot per row); of the 13 forward neighbours inside the tile only those unions run that the
//                 runs do not already imply. parent[i] = global index of the tile-local root, tsize[root] = tile-local point count
//   k_cc_border   inside points on a tile face: union through global memory with the inside neighbours in the adjacent tiles (all 13
//                 forward directions that leave the tile). parent[] is read with agent-scope atomic loads and changed with atomicMin only.
//   k_cc_roots    per tile-local root r: f = find(r); parent[r] = f; sizes[f] += tsize[r] — one integer atomic per tile-local component
//   k_cc_flatten  labels[i] = find(i) (at most two steps now); the counts
// Integer atomics only: nothing is refused under FOC_DETERMINISTIC.
#include <cmath>
#include "common.h"

#define CC_NONE 0xFFFFFFFFu                 // FOC_CC_NONE of include/focnerf.h
#define CC_TX 8u
#define CC_TY 8u
#define CC_TZ 32u
#define CC_TILE (CC_TX * CC_TY * CC_TZ)     // 2048 points: 8 per thread of a 256-thread workgroup, 16 KiB of LDS
#define CC_MAX_POINTS (1ull << 29)

struct CcDim { uint32_t nx, ny, nz, sx, n, ty, tz; };          // sx = ny * nz; ty, tz: tiles along y and z

// ---------------------------------------------------------------- union-find in LDS (tile-local indices, CC_NONE outside)
__device__ __forceinline__ uint32_t cc_ld_lds(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ uint32_t cc_find_lds(uint32_t *L, uint32_t a, uint32_t *err) {
    const uint32_t a0 = a;
    for (uint32_t it = 0; it <= CC_TILE; it++) {               // a chain strictly decreases below CC_TILE
        const uint32_t p = cc_ld_lds(L + a);
        if (p == a) {
            if (a != a0) atomicMin(L + a0, a);                 // the start skips to the root it found
            return a;
        }
        a = p;
    }
    *err = 1u;
    return a;
}
__device__ __forceinline__ void cc_union_lds(uint32_t *L, uint32_t a, uint32_t b, uint32_t *err) {
    for (uint32_t it = 0; it <= 2 * CC_TILE; it++) {           // a + b strictly decreases per turn
        a = cc_find_lds(L, a, err);
        b = cc_find_lds(L, b, err);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }     // a > b: the larger root goes under the smaller index
        const uint32_t old = atomicMin(L + a, b);
        if (old == a) return;                                  // a was a root: linked
        a = old;                                               // it was not any more: go on from where it pointed
    }
    *err = 1u;
}

// ---------------------------------------------------------------- union-find in global memory
__device__ __forceinline__ uint32_t cc_ld(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of a, halving the path it walks (a word only ever drops to another ancestor: atomicMin)
__device__ __forceinline__ uint32_t cc_find(uint32_t *P, uint32_t a, uint32_t cap, uint32_t *err) {
    for (uint32_t it = 0; it <= cap; it++) {
        const uint32_t p = cc_ld(P + a);
        if (p == a) return a;
        const uint32_t g = cc_ld(P + p);
        if (g == p) return p;
        atomicMin(P + a, g);
        a = g;
    }
    atomicOr(err, 1u);
    return a;
}
__device__ __forceinline__ void cc_union(uint32_t *P, uint32_t a, uint32_t b, uint32_t cap, uint32_t *err) {
    for (uint32_t it = 0; it <= cap; it++) {
        a = cc_find(P, a, cap, err);
        b = cc_find(P, b, cap, err);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(P + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(err, 1u);
}
// the root of a through plain loads: for a pass that no longer writes parent[]
__device__ __forceinline__ uint32_t cc_find_ro(const uint32_t *__restrict__ P, uint32_t a, uint32_t cap, uint32_t *err) {
    for (uint32_t it = 0; it <= cap; it++) {
        const uint32_t p = P[a];
        if (p == a) return a;
        a = p;
    }
    atomicOr(err, 1u);
    return a;
}

// the 13 forward directions: k = 0..8 (1, k / 3 - 1, k % 3 - 1), k = 9..11 (0, 1, k - 10), k = 12 (0, 0, 1)
__device__ __forceinline__ void cc_dir(int k, int &dx, int &dy, int &dz) {
    dx = k < 9 ? 1 : 0;
    dy = k < 9 ? k / 3 - 1 : (k < 12 ? 1 : 0);
    dz = k < 9 ? k % 3 - 1 : (k < 12 ? k - 10 : 1);
}

// ---------------------------------------------------------------- pass 1: tile-local components
__global__ void __launch_bounds__(256) k_cc_tile(const float *__restrict__ vol, CcDim D, float thr, uint32_t *__restrict__ parent, uint32_t *__restrict__ tsize,
                                                 uint32_t *__restrict__ sizes, uint32_t *__restrict__ counts) {
    __shared__ uint32_t L[CC_TILE];
    __shared__ uint32_t S[CC_TILE];
    __shared__ uint32_t ROW[CC_TX * CC_TY];                     // the inside bits of the z row (lx, ly)
    __shared__ uint32_t any_inside, lds_err;
    const uint32_t tid = threadIdx.x;
    const uint32_t tzi = blockIdx.x % D.tz, tyi = (blockIdx.x / D.tz) % D.ty, txi = blockIdx.x / (D.tz * D.ty);
    const uint32_t x0 = txi * CC_TX, y0 = tyi * CC_TY, z0 = tzi * CC_TZ;
    // thread tid owns the column (ly, lz) = (tid / 32, tid % 32) and in it the points lx = 0..7: local index lx * 256 + tid
    const uint32_t ly = tid >> 5, lz = tid & 31;
    const uint32_t y = y0 + ly, z = z0 + lz;
    const bool col = y < D.ny && z < D.nz;
    if (tid == 0) { any_inside = 0u; lds_err = 0u; }
    __syncthreads();
    bool mine = false;
#pragma unroll
    for (uint32_t lx = 0; lx < CC_TX; lx++) {
        const uint32_t x = x0 + lx, l = lx * 256 + tid;
        const bool in = col && x < D.nx && vol[x * D.sx + y * D.nz + z] >= thr;       // a NaN compares false: outside
        // a wave holds two z rows (lanes 0..31: ly even, 32..63: ly odd). A point starts at the FIRST point of its run of inside points
        // along z: the runs are joined before any union, and the union phase has only the four neighbouring rows to look at.
        const uint32_t row = (uint32_t)(__ballot(in) >> (tid & 32u));
        const uint32_t zeros = ~row & ((1u << lz) - 1u);       // the outside points below lz
        const uint32_t start = zeros ? 32u - (uint32_t)__clz(zeros) : 0u;
        L[l] = in ? l - lz + start : CC_NONE;
        S[l] = 0u;
        if (lz == 0) ROW[lx * CC_TY + ly] = row;
        mine = mine || in;
    }
    if (mine) any_inside = 1u;
    __syncthreads();
    if (any_inside == 0u) {                                    // an empty tile (most of a volume): nothing to join
#pragma unroll
        for (uint32_t lx = 0; lx < CC_TX; lx++) {
            const uint32_t x = x0 + lx;
            if (col && x < D.nx) { const uint32_t g = x * D.sx + y * D.nz + z; parent[g] = CC_NONE; tsize[g] = 0u; sizes[g] = 0u; }
        }
        return;
    }
    uint32_t err = 0u;
    for (uint32_t lx = 0; lx < CC_TX; lx++) {
        const uint32_t l = lx * 256 + tid;
        const uint32_t own = ROW[lx * CC_TY + ly];
        if (!((own >> lz) & 1u)) continue;
        const bool first = lz == 0 || !((own >> (lz - 1)) & 1u);           // the first point of its run
        // the four forward rows (dx, dy) = (0, 1), (1, -1), (1, 0), (1, 1); in such a row the points at z - 1, z, z + 1 are the neighbours.
        // If the middle one is inside, the other two are in its run: one union. A point that continues a run finds z - 1 and z joined
        // already by the point before it (whose neighbours they are too), and z + 1 with them unless the middle one is outside.
        for (int k = 0; k < 4; k++) {
            const uint32_t qx = lx + (k > 0 ? 1u : 0u), qy = ly + (uint32_t)(k == 0 ? 1 : k - 2);       // a step below 0 wraps past the limit
            if (qx >= CC_TX || qy >= CC_TY) continue;
            const uint32_t m = ROW[qx * CC_TY + qy], q = qx * 256 + qy * 32 + lz;
            const bool mid = (m >> lz) & 1u, lo = lz > 0 && ((m >> (lz - 1)) & 1u), hi = lz + 1 < CC_TZ && ((m >> (lz + 1)) & 1u);
            if (first) {
                if (mid) cc_union_lds(L, l, q, &err);
                else {
                    if (lo) cc_union_lds(L, l, q - 1, &err);
                    if (hi) cc_union_lds(L, l, q + 1, &err);
                }
            } else if (!mid && hi) cc_union_lds(L, l, q + 1, &err);
        }
    }
    __syncthreads();
    uint32_t root[CC_TX];
#pragma unroll
    for (uint32_t lx = 0; lx < CC_TX; lx++) {
        const uint32_t l = lx * 256 + tid;
        root[lx] = L[l] == CC_NONE ? CC_NONE : cc_find_lds(L, l, &err);
        if (root[lx] != CC_NONE) atomicAdd(S + root[lx], 1u);
    }
    if (err) lds_err = 1u;
    __syncthreads();
#pragma unroll
    for (uint32_t lx = 0; lx < CC_TX; lx++) {
        const uint32_t x = x0 + lx, l = lx * 256 + tid;
        if (!(col && x < D.nx)) continue;
        const uint32_t g = x * D.sx + y * D.nz + z, r = root[lx];
        // local order is global order inside a tile: the smallest local index is the smallest global one
        parent[g] = r == CC_NONE ? CC_NONE : (x0 + (r >> 8)) * D.sx + (y0 + ((r >> 5) & 7u)) * D.nz + z0 + (r & 31u);
        tsize[g] = S[l];
        sizes[g] = 0u;
    }
    if (tid == 0 && lds_err) atomicOr(counts + 3, 1u);
}

// ---------------------------------------------------------------- pass 2: joins across tile faces
__global__ void __launch_bounds__(256) k_cc_border(CcDim D, uint32_t *__restrict__ parent, uint32_t *__restrict__ counts) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < D.n; i += gridDim.x * 256) {
        const uint32_t pi = cc_ld(parent + i);
        if (pi == CC_NONE) continue;
        const uint32_t x = i / D.sx, r = i - x * D.sx, y = r / D.nz, z = r - y * D.nz;
        const bool x_hi = (x & (CC_TX - 1)) == CC_TX - 1, y_lo = (y & (CC_TY - 1)) == 0, y_hi = (y & (CC_TY - 1)) == CC_TY - 1,
                   z_lo = (z & (CC_TZ - 1)) == 0, z_hi = (z & (CC_TZ - 1)) == CC_TZ - 1;
        if (!(x_hi || y_lo || y_hi || z_lo || z_hi)) continue;
        // the neighbours' parent words first: 13 loads that do not wait for one another
        uint32_t pq[13];
#pragma unroll
        for (int k = 0; k < 13; k++) {
            int dx, dy, dz;
            cc_dir(k, dx, dy, dz);
            const bool leaves = (dx == 1 && x_hi) || (dy == 1 && y_hi) || (dy == -1 && y_lo) || (dz == 1 && z_hi) || (dz == -1 && z_lo);
            const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;          // below 0 wraps past the dimension
            pq[k] = (leaves && qx < D.nx && qy < D.ny && qz < D.nz) ? cc_ld(parent + qx * D.sx + qy * D.nz + qz) : CC_NONE;
        }
        // a parent word is an ancestor of its point: joining the two words' trees joins the two points, and a neighbour whose word equals
        // the one joined last lies in that neighbour's component (the face of a solid tile: one union in place of nine)
        uint32_t last = CC_NONE;
#pragma unroll
        for (int k = 0; k < 13; k++) {
            if (pq[k] == CC_NONE || pq[k] == last) continue;
            cc_union(parent, pi, pq[k], D.n, counts + 3);
            last = pq[k];
        }
    }
}

// ---------------------------------------------------------------- pass 3: tile-local roots -> final roots, sizes
__global__ void __launch_bounds__(256) k_cc_roots(CcDim D, uint32_t *__restrict__ parent, const uint32_t *__restrict__ tsize, uint32_t *__restrict__ sizes,
                                                  uint32_t *__restrict__ counts) {
    __shared__ uint32_t block_roots;
    if (threadIdx.x == 0) block_roots = 0u;
    __syncthreads();
    uint32_t n_roots = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < D.n; i += gridDim.x * 256) {
        const uint32_t t = tsize[i];
        if (t == 0u) continue;
        const uint32_t f = cc_find(parent, i, D.n, counts + 3);
        if (f == i) n_roots++;
        else atomicMin(parent + i, f);
        atomicAdd(sizes + f, t);
    }
    n_roots = (uint32_t)wave_sum_i((int)n_roots);
    if ((threadIdx.x & 63) == 0 && n_roots) atomicAdd(&block_roots, n_roots);
    __syncthreads();
    if (threadIdx.x == 0 && block_roots) atomicAdd(counts + 0, block_roots);
}

// ---------------------------------------------------------------- pass 4: labels and the counts
__global__ void __launch_bounds__(256) k_cc_flatten(CcDim D, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ sizes, uint32_t *__restrict__ labels,
                                                    uint32_t *__restrict__ counts) {
    __shared__ uint32_t block_inside, block_max;
    if (threadIdx.x == 0) { block_inside = 0u; block_max = 0u; }
    __syncthreads();
    uint32_t inside = 0, largest = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < D.n; i += gridDim.x * 256) {
        const uint32_t p = parent[i];
        labels[i] = p == CC_NONE ? CC_NONE : cc_find_ro(parent, p, D.n, counts + 3);
        inside += p != CC_NONE;
        largest = max(largest, sizes[i]);
    }
    inside = (uint32_t)wave_sum_i((int)inside);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, (uint32_t)__shfl_xor((int)largest, o, 64));
    if ((threadIdx.x & 63) == 0) {
        if (inside) atomicAdd(&block_inside, inside);
        if (largest) atomicMax(&block_max, largest);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (block_inside) atomicAdd(counts + 1, block_inside);
        if (block_max) atomicMax(counts + 2, block_max);
    }
}

// ---------------------------------------------------------------- select
__global__ void __launch_bounds__(256) k_cc_select(const float *vol, const uint32_t *__restrict__ labels, const uint8_t *__restrict__ keep, float fill, float *out,
                                                   uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t l = labels[i];
        out[i] = (l < n && !keep[l]) ? fill : vol[i];          // CC_NONE (and any word that is no index) keeps the value; out may be vol
    }
}

// ---------------------------------------------------------------- host side
// the dimensions foc_mc_count serves (mesh.hip mc_dims_ok)
static bool cc_dims_ok(const char *who, uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) { foc_set_error("%s: every dimension must be >= 2 (got %u x %u x %u)", who, nx, ny, nz); return false; }
    if ((uint64_t)nx * ny > CC_MAX_POINTS || (uint64_t)nx * ny * nz > CC_MAX_POINTS) {
        foc_set_error("%s: nx * ny * nz must not exceed 2^29 points (got %u x %u x %u)", who, nx, ny, nz);
        return false;
    }
    return true;
}

extern "C" {

uint64_t foc_cc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (!cc_dims_ok("cc_workspace_bytes", nx, ny, nz)) return 0;
    return (uint64_t)nx * ny * nz * 2 * sizeof(uint32_t);      // parent[n], tsize[n]
}

int foc_cc_label(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float thr, uint32_t *labels, uint32_t *sizes, void *workspace,
                 uint64_t workspace_bytes, uint32_t *counts4, void *stream) {
    FocDeviceGuard foc_guard_(stream, volume);
    FOC_REQUIRE(volume && labels && sizes && workspace && counts4, FOC_E_INVALID, "cc_label: null pointer (volume, labels, sizes, workspace, counts4)");
    if (!cc_dims_ok("cc_label", nx, ny, nz)) return FOC_E_INVALID;
    FOC_REQUIRE(std::isfinite(thr), FOC_E_INVALID, "cc_label: thr must be finite");
    FOC_REQUIRE(workspace_bytes >= foc_cc_workspace_bytes(nx, ny, nz), FOC_E_INVALID, "cc_label: workspace of %llu bytes, foc_cc_workspace_bytes(%u, %u, %u) asks for %llu",
                (unsigned long long)workspace_bytes, nx, ny, nz, (unsigned long long)foc_cc_workspace_bytes(nx, ny, nz));
    FOC_REQUIRE((((uintptr_t)workspace) & 3) == 0, FOC_E_INVALID, "cc_label: workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    CcDim D{nx, ny, nz, ny * nz, nx * ny * nz, foc_div_up(ny, CC_TY), foc_div_up(nz, CC_TZ)};
    const uint32_t tiles = foc_div_up(nx, CC_TX) * D.ty * D.tz;            // <= nx * ny * nz
    uint32_t *parent = reinterpret_cast<uint32_t *>(workspace), *tsize = parent + D.n;
    if (foc_zero_async(counts4, 16, st) != hipSuccess) { foc_set_error("cc_label: launch failed (zero fill)"); return FOC_E_LAUNCH; }
    hipLaunchKernelGGL(k_cc_tile, dim3(tiles), dim3(256), 0, st, volume, D, thr, parent, tsize, sizes, counts4);
    FOC_CHECK_LAUNCH("cc_label");
    const dim3 grid(foc_grid_1d(D.n, 256)), block(256);
    hipLaunchKernelGGL(k_cc_border, grid, block, 0, st, D, parent, counts4);
    FOC_CHECK_LAUNCH("cc_label");
    hipLaunchKernelGGL(k_cc_roots, grid, block, 0, st, D, parent, tsize, sizes, counts4);
    FOC_CHECK_LAUNCH("cc_label");
    hipLaunchKernelGGL(k_cc_flatten, grid, block, 0, st, D, parent, sizes, labels, counts4);
    FOC_CHECK_LAUNCH("cc_label");
    return FOC_OK;
}

int foc_cc_select(const float *volume, const uint32_t *labels, const uint8_t *keep, float fill, float *out, uint32_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, volume);
    FOC_REQUIRE(volume && labels && keep && out, FOC_E_INVALID, "cc_select: null pointer (volume, labels, keep, out)");
    FOC_REQUIRE(n <= CC_MAX_POINTS, FOC_E_INVALID, "cc_select: n must not exceed 2^29 points (got %u)", n);
    FOC_REQUIRE(fill == fill, FOC_E_INVALID, "cc_select: fill must not be a NaN");
    if (n == 0) return FOC_OK;
    hipLaunchKernelGGL(k_cc_select, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, volume, labels, keep, fill, out, n);
    FOC_CHECK_LAUNCH("cc_select");
    return FOC_OK;
}

} // extern "C"
