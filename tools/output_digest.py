#!/usr/bin/env python3
"""tools/output_digest.py [out.json] [--sections a,b] [--root DIR]: sha256 of every output of the fused-MLP, per-sample, ragged-composite, fixed-step,
combine, marching and grid-encoder kernels on seeded inputs, and of the occupancy node driven from Python, as one JSON object {case: {output: digest}} — the bits
of one build — printed, or written to out.json with a one-line summary printed instead. Run it once per build on the same GPU
(FOCNERF_LIB_PATH selects the library) and compare the two objects: equal = the same bits on every case.
--sections: of mlp, per_sample, ragged, fixed, combine, march, grid, node (default: all). --root DIR: the checkout whose focnerf_amd package (and library)
is imported instead of this one's — the `node` section runs the package's Python, so one copy of this tool serves both commits of a
comparison.

The cases are the smallest that reach every branch of those kernels: ray counts and step counts below, at and above one 64-lane step,
with and without noise, scalar and per-ray background, density_scale 1 and 2, colour widths 4 and 16, a ray list with an empty ray, a
ray that does not fit the list and spare rows behind the last ray, stops in the first step and in a later one.

`node` (FOC_DETERMINISTIC on): a training step of `NeRFRenderer.run_cuda` on the five network kinds — plain, network_linear with its
background model, network_tcnn_legacy (column 31 = 1), network_foc and network_tcnn (object feature, column 47 = 0 / 1) — through the
one-call node and the call-by-call chain (FOC_OCC_NATIVE_NODE 1 / 0), at 1, 63, 64, 65 and 300 rays, max_steps 16 and 64, with default,
scalar and per-ray backgrounds, the object networks with and without a ray mask, a list that overflows and an unbudgeted one; image, depth,
weights_sum, the criterion (the masked norm of ray_sumsq), the marched counts and every parameter gradient. Then one evaluation view per
kind through the native render loop. Run a build twice before comparing two builds: an output that differs between the two runs of one
build (an fp32 atomic of torch's own backward) says nothing about the builds.

`march` (raymarching.hip's entry points called through `_lib`, outputs only — scratch, worklists and block counts are left out; every walker
writes its own slots and the atomics involved are integer adds, so every digested output is deterministic): a random bitfield of fill 0.5 at
H = 32, bound 1 and 2 with their cascades. The training march, plain and `_field`: 1, 5 and 130 rays, max_steps 7 (dt_min > dt_max: the kernels
without the median), 64 (steps of dt_min, at bound 2 and dt_gamma 0.013 also of t dt_gamma) and 1024 (all three regimes), dt_gamma 0, 1/128
and 0.013, FOC_MARCH_SERIAL 0 and 1, counter base 0 and 37, a list that just fits and one too small for the last ray, the field form with
pad_align 0 and 128 and with the box or the ranges given. The inference march (max_steps 64 and 1024): lists of 1, 70 and 300 entries with dead ones among them,
foc_march_rays at n_step 1, 3, 8, 16 with the row form off and on, foc_march_rays_two_phase at n_step 1, 2, 4, 8, 16 in its four forms with
flags 0, 1, 3 and (where the form writes sample-major arrays) 7. foc_composite_rays at n_step 1, 2, 3, 4, 8, 16, foc_composite_compact at 2, 4
and 8 in both layouts with and without a deaths histogram, T_thresh 1e-4 and 0.5. foc_compact_alive at 1, 1023, 1025 and 2100 entries.

`mlp` (ffmlp.hip, field_fwd.hip, normals.hip through the C ABI; FOC_DETERMINISTIC on, so that the weight gradients of the two-kernel backward are
sums in a fixed order): at 1, 31, 33, 65, 129 and 257 rows — a ragged 32-row tile and the next one, past k_nerf_infer's 64-row tile, past
k_mlp_bwd_fused's 128-row group, past one workgroup of 64-row tiles. foc_ffmlp_forward (outputs, forward buffer), _inference and _forward_planar at
hidden 16, 32, 64, 128, 1 to 3 layers, input 16, 32, 64, relu, none and sigmoid (row-major only); foc_ffmlp_backward on the same shapes with
FOC_MLP_BWD_FUSED 1 and 0, from the stored activations and (single-pass kernel) re-evaluating them, with and without a backward buffer, and
foc_ffmlp_backward_planar: grad_inputs, grad_weights, the backward buffer. The colour head, the training forward of both networks and the field
inference each with their _pad / _pad31 twins, with and without an object feature: foc_color_head_forward / _backward at 2 and 3 layers, c_width 4
and 16 (outputs, grad_h, grad_w, grad_obj); foc_field_forward_train on the five layer pairs, relu and none; foc_nerf_field_inference planar and
row-major, dir_block 0 and 64, dir_div 1 and 4. foc_field_normals at 1, 2, 3 sigma layers with every optional output, with and without a rotation.

`grid` (gridencoder.hip, gridencoder_nd.hip through the C ABI): forward [L,B,C] and [B, L*C], dy_dx and grad_inputs — the outputs no atomic
touches — for D 2..5, C 1, 2, 4, 8 (fp16 tables: even C), both dtypes, hash and tiled grids, align_corners off and on, linear and
smoothstep interpolation, L 1, 3, 9 and B 1, 257, 600, the points with exact 0 and 1 and a few outside [0, 1]. The atomically summed
outputs only where arrival order cannot matter, which the tool asserts in float64 before it hashes: grad_embeddings of one level with
H = 9 (scale 8), align_corners on, positions on multiples of 1/16 and small-integer gradients — every addend a multiple of 2^-5 and
the sum of |addends| per table element below 2^6, so fp16 and fp32 adds are exact in any order; grad_total_variation on one tiled level
with every point in a cell and a row of its own (one add onto zero per row).

Left out: the gradient of the background model's table (foc_background_backward: fp32 atomics, not bit-stable run to run in the default
mode) and with it the whole background backward; the forward is covered. Every input is drawn on the host from a seeded generator.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ARGS = sys.argv[1:]


def _option(name):
    """The value behind `name` in the argument list (removed from it), or None."""
    if name not in ARGS:
        return None
    i = ARGS.index(name)
    if i + 1 >= len(ARGS):
        sys.exit(f"usage: output_digest.py [out.json] [--sections a,b] [--root DIR]: {name} needs a value")
    value = ARGS[i + 1]
    del ARGS[i: i + 2]
    return value


ROOT = _option("--root") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ALL_SECTIONS = ("mlp", "per_sample", "ragged", "fixed", "combine", "march", "grid", "node")
SECTIONS = (_option("--sections") or ",".join(ALL_SECTIONS)).split(",")
if set(SECTIONS) - set(ALL_SECTIONS):
    sys.exit(f"usage: output_digest.py [out.json] [--sections a,b] [--root DIR]: sections are {', '.join(ALL_SECTIONS)}, got {', '.join(SECTIONS)}")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from focnerf_amd._lib import lib, ptr, stream_of, check, set_option, get_option       # noqa: E402
import background_ref as br                                     # noqa: E402
import ragged_ref as rr                                         # noqa: E402

OUT = {}
NAN32 = float("nan")


def digest(t):
    t = t.detach().contiguous()
    if t.numel() <= 1 << 20:
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    # a table-sized tensor (the hash grid's gradient: almost all zero bits): the shape, and where the other bits are and what they are
    bits = t.view(-1).view({2: torch.int16, 4: torch.int32}[t.element_size()])
    at = bits.nonzero().view(-1)
    return hashlib.sha256(repr(tuple(t.shape)).encode() + at.cpu().numpy().tobytes() + bits[at].cpu().numpy().tobytes()).hexdigest()


def put(case, **tensors):
    torch.cuda.synchronize()
    OUT[case] = {k: digest(t) for k, t in tensors.items() if t is not None}


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda() if a is not None else None


def full(shape, dtype=torch.float32):
    """An output buffer with a recognisable fill: a row the kernel does not write shows up as such in both builds alike."""
    return torch.full(shape if isinstance(shape, tuple) else (shape,), -3.0, dtype=dtype, device="cuda")


def call(fn, *args):
    check(fn(*args, stream_of(None)), fn.__name__)


# ---------------------------------------------------------------- per-sample ops (head.hip, background.hip, Morton, density grid)
def per_sample():
    rng = np.random.default_rng(11)
    M = 130
    d = rng.normal(0, 1, (M, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    h = rng.normal(0, 3, (M, 16)); h[:8, 0] = [15.0, -15.0, 15.0078125, -15.0078125, 16.5, -20.0, 0.0, 14.5]
    dirs, h16 = cuda(d.astype(np.float32)), cuda(h.astype(np.float16))
    sh = full((M, 16))
    call(lib.foc_sh_encode, ptr(dirs), M, ptr(sh))
    put("sh_encode", sh=sh)
    obj = cuda(rng.normal(0, 1, 16).astype(np.float16))
    for width in (32, 48):
        sigma, cin = full(M), full((M, width), torch.float16)
        call(lib.foc_sample_head_forward, ptr(h16), ptr(dirs), M, ptr(sigma), ptr(cin), ptr(obj if width == 48 else None), width)
        g_sigma, g_cin, g_h = cuda(rng.normal(0, 1, M).astype(np.float32)), cuda(rng.normal(0, 1, (M, width)).astype(np.float16)), full((M, 16), torch.float16)
        call(lib.foc_sample_head_backward, ptr(h16), ptr(g_sigma), ptr(g_cin), M, ptr(g_h), width)
        put(f"sample_head[{width}]", sigma=sigma, cin=cin, grad_h=g_h)
    c16 = cuda(rng.normal(0, 3, (M, 16)).astype(np.float16))
    rgb, g_c = full((M, 3)), full((M, 16), torch.float16)
    call(lib.foc_rgb_head_forward, ptr(c16), M, ptr(rgb))
    g_rgb = cuda(rng.normal(0, 1, (M, 3)).astype(np.float32))
    call(lib.foc_rgb_head_backward, ptr(c16), ptr(g_rgb), M, ptr(g_c))
    put("rgb_head", rgb=rgb, grad_c=g_c)

    # the background forward at N = 130 (coordinates form), grid "b" of the float64 reference's cases
    W0, W1 = br.weights("lin")
    emb, off, blob = cuda(br.table("b", 0.5)), cuda(np.asarray(br.GRIDS["b"], np.int32)), cuda(br.pack_blob(W0, W1))
    coords = cuda(rng.uniform(-1, 1, (M, 2)).astype(np.float32))
    bg = full((M, 3), torch.float16)
    call(lib.foc_background_forward, None, ptr(dirs), ptr(coords), 0.0, M, ptr(emb), ptr(off), br.LOG2_SCALE, br.BASE_RESOLUTION, ptr(blob), ptr(bg))
    put("background_forward", rgb=bg)

    H = 32
    xyz = cuda(rng.integers(0, H, (M, 3)).astype(np.int32))
    idx, back = full(M, torch.int32), full((M, 3), torch.int32)
    call(lib.foc_morton3D, ptr(xyz), M, ptr(idx))
    call(lib.foc_morton3D_invert, ptr(idx), M, ptr(back))
    cells = full((H ** 3, 3))
    call(lib.foc_grid_cells_xyz, 1, H, 1.0, None, ptr(cells))
    grid = cuda(rng.uniform(-1, 2, (1, H ** 3)).astype(np.float32))
    Mc = 4096
    sig, ind = cuda(rng.uniform(0, 30, Mc).astype(np.float32)), cuda(rng.integers(0, H ** 3, Mc).astype(np.int32))
    bits, mean = torch.zeros(H ** 3 // 8, dtype=torch.uint8, device="cuda"), full(1)
    nbytes = lib.foc_grid_update_apply_workspace_bytes(1, H)
    ws = torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
    call(lib.foc_grid_update_apply, ptr(grid), 1, H, ptr(sig), ptr(ind), Mc, 1.0, 0.95, 10.0, ptr(bits), ptr(mean), ptr(ws), nbytes)
    put("morton_and_grid[32]", indices=idx, coords=back, cells=cells, density_grid=grid, bitfield=bits, mean=mean)


# ---------------------------------------------------------------- ragged composite (raymarching.hip R7 / R8, occtrain.hip)
def ragged():
    for T_thresh in (1e-4, 0.5):
        # (count, stop): empty, one sample, a full step, one past it (stop in the second step), two steps and a bit (stops in the first
        # step, in the third, never)
        pairs = [(0, None), (1, 0), (64, None), (65, 64), (130, 10), (130, 129), (130, None), (64, 63)]
        for ds in (1.0, 2.0):
            c = rr.constructed_case(pairs, 5, T_thresh, ds=ds)
            N, M, total = c["N"] + 1, c["M"], c["total"]
            assert M > total + 3                                           # spare rows behind the last ray
            rays = np.concatenate([c["rays"], [[N - 1, M - 3, 10]]]).astype(np.int32)       # the added ray does not fit the list
            rng = np.random.default_rng(17)
            ext = lambda a, v: np.concatenate([a, v]).astype(np.float32)
            nears, fars = ext(c["nears"], [0.3]), ext(c["fars"], [1.7])
            bg_ray = ext(c["bg"], rng.random((1, 3)))
            g = {k: cuda(ext(v, rng.normal(0, 1, (1,) + v.shape[1:]))) for k, v in c["grads"].items()}
            d_rays, d_deltas, d_h, counter = cuda(rays), cuda(c["deltas"]), cuda(np.repeat(c["h0"][:, None], 16, 1)), cuda(np.array([total, N], np.int32))
            c16 = np.zeros((M, 16), np.float16); c16[:, :3] = c["c"]
            d_c = {16: cuda(c16), 4: cuda(c16[:, :4])}
            d_near, d_far, d_bg = cuda(nears), cuda(fars), cuda(bg_ray)
            tag = f"[T_thresh={T_thresh:g},ds={ds:g}]"

            sig, rgb = rr.composite_inputs(c)
            d_sig, d_rgb = cuda(sig), cuda(rgb)
            ws, dep, img = full(N), full(N), full((N, 3))
            call(lib.foc_composite_rays_train_forward, ptr(d_sig), ptr(d_rgb), ptr(d_deltas), ptr(d_rays), M, N, T_thresh, ptr(ws), ptr(dep), ptr(img))
            res = dict(weights_sum=ws, depth=dep, image=img)
            for with_ws in (True, False):
                g_sig, g_rgb = torch.zeros(M, device="cuda"), torch.zeros(M, 3, device="cuda")
                call(lib.foc_composite_rays_train_backward, ptr(g["grad_ws"] if with_ws else None), ptr(g["grad_image"]), ptr(d_sig), ptr(d_rgb), ptr(d_deltas),
                     ptr(d_rays), ptr(ws), ptr(img), M, N, T_thresh, ptr(g_sig), ptr(g_rgb))
                res.update({f"grad_sigmas[ws={with_ws}]": g_sig, f"grad_rgbs[ws={with_ws}]": g_rgb})
            put("composite_rays_train" + tag, **res)

            for cw in (4, 16):
                for bgr in (d_bg, None):
                    for crit in (False, True):
                        ws, raw, img, dep, sq = full(N), full((N, 3)), full((N, 3)), full(N), full(N) if crit else None
                        args = (ptr(d_h), ptr(d_c[cw]), cw, ptr(d_deltas), ptr(d_rays), M, N, T_thresh, ds, ptr(bgr), rr.BG_SCALAR, ptr(d_near), ptr(d_far), ptr(ws), ptr(raw),
                                ptr(img), ptr(dep))
                        call(lib.foc_occ_tail_forward_sumsq, *args, ptr(sq)) if crit else call(lib.foc_occ_tail_forward, *args)
                        res = dict(weights_sum=ws, image_raw=raw, image=img, depth=dep, ray_sumsq=sq)
                        for with_ws in (True, False):
                            g_c, g_h0 = full((M, cw), torch.float16), full(M, torch.float16)
                            args = (ptr(g["grad_image"]), ptr(g["grad_ws"] if with_ws else None), ptr(d_h), ptr(d_c[cw]), cw, ptr(d_deltas), ptr(d_rays), ptr(counter),
                                    ptr(ws), ptr(raw), M, N, T_thresh, ds, ptr(bgr), rr.BG_SCALAR, ptr(g_c), ptr(g_h0))
                            call(lib.foc_occ_tail_backward_sumsq, *args, ptr(g["grad_sumsq"])) if crit else call(lib.foc_occ_tail_backward, *args)
                            res.update({f"grad_c[ws={with_ws}]": g_c, f"grad_h0[ws={with_ws}]": g_h0})
                        put(f"occ_tail{tag}[c_width={cw},bg_ray={bgr is not None},sumsq={crit}]", **res)


# ---------------------------------------------------------------- fixed-step family (fixedstep.hip) and the combiner (combine.hip)
def fixed(N, T, noisy, per_ray_bg, ds):
    rng = np.random.default_rng(1000 * N + 10 * T + 2 * noisy + per_ray_bg)
    M = N * T
    f32 = lambda a: cuda(np.asarray(a, np.float32))
    h = rng.normal(0, 2, (M, 16)); h[::7, 0] = rng.choice([15.0, -15.0, 16.5, -17.0, 15.0078125], len(h[::7]))
    h16, c16 = cuda(h.astype(np.float16)), cuda(rng.normal(0, 2, (M, 16)).astype(np.float16))
    d = rng.normal(0, 1, (N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = rng.uniform(0.1, 0.6, N)
    nears, fars, dirs = f32(near), f32(near + rng.uniform(0.5, 2.5, N)), f32(d)
    noise = f32(rng.random((N, T))) if noisy else None
    bg_ray, bg = (f32(rng.random((N, 3))) if per_ray_bg else None), 0.7
    thresh = 1e-3                                                          # weights on both sides of it
    g_img, g_ws, g_dp, g_sq = f32(rng.normal(0, 1, (N, 3))), f32(rng.normal(0, 0.5, N)), f32(rng.normal(0, 0.5, N)), f32(rng.normal(0, 1e-3, N))
    tag = f"[N={N},T={T},noise={noisy},bg_ray={per_ray_bg},ds={ds:g}]"

    width = 48 if ds == 2.0 else 32
    obj = cuda(rng.normal(0, 1, 16).astype(np.float16)) if width == 48 else None
    sigma, trans, w, ws, dp, cin = full(M), full(M), full(M), full(N), full(N), full((M, width), torch.float16)
    call(lib.foc_fixed_head_forward, ptr(h16), ptr(dirs), ptr(nears), ptr(fars), ptr(noise), N, T, ds, ptr(sigma), ptr(trans), ptr(w), ptr(ws), ptr(dp), ptr(cin), ptr(obj), width)
    g_w, g_cin, g_h = f32(rng.normal(0, 1, M)), cuda(rng.normal(0, 1, (M, width)).astype(np.float16)), full((M, 16), torch.float16)
    call(lib.foc_fixed_head_backward, ptr(h16), ptr(sigma), ptr(trans), ptr(nears), ptr(fars), ptr(noise), ptr(g_w), ptr(g_ws), ptr(g_dp), ptr(g_cin), N, T, ds, ptr(g_h), width)
    g_h_nc = full((M, 16), torch.float16)                                 # without grad_cin / grad_depth
    call(lib.foc_fixed_head_backward, ptr(h16), ptr(sigma), ptr(trans), ptr(nears), ptr(fars), ptr(noise), ptr(g_w), None, None, None, N, T, ds, ptr(g_h_nc), width)
    img, g_c, g_wc = full((N, 3)), full((M, 16), torch.float16), full(M)
    call(lib.foc_fixed_composite_forward, ptr(c16), ptr(w), ptr(bg_ray), bg, N, T, thresh, ptr(img))
    call(lib.foc_fixed_composite_backward, ptr(g_img), ptr(c16), ptr(w), ptr(bg_ray), bg, N, T, thresh, ptr(g_c), ptr(g_wc))
    put("fixed_head+composite" + tag, sigma=sigma, trans=trans, weights=w, weights_sum=ws, depth=dp, cin=cin, grad_h=g_h, grad_h_plain=g_h_nc, image=img, grad_c=g_c, grad_w=g_wc)

    for cw in (4, 16):
        c = c16[:, :4].contiguous() if cw == 4 else c16
        for crit in (False, True):
            sigma, trans, w, ws, dp, img, sq = full(M), full(M), full(M), full(N), full(N), full((N, 3)), full(N) if crit else None
            call(lib.foc_fixed_tail_forward, ptr(h16), ptr(c), ptr(nears), ptr(fars), ptr(noise), ptr(bg_ray), bg, N, T, ds, thresh, ptr(sigma), ptr(trans), ptr(w), ptr(ws), ptr(dp),
                 ptr(img), cw, ptr(sq))
            g_c, g_h0 = full((M, cw), torch.float16), full(M, torch.float16)
            call(lib.foc_fixed_tail_backward, ptr(g_img), ptr(g_ws), ptr(g_dp), ptr(c), ptr(sigma), ptr(trans), ptr(w), ptr(nears), ptr(fars), ptr(noise), ptr(bg_ray), bg, N, T, ds,
                 thresh, ptr(g_c), ptr(g_h0), cw, ptr(g_sq if crit else None))
            put(f"fixed_tail{tag}[c_width={cw},sumsq={crit}]", sigma=sigma, trans=trans, weights=w, weights_sum=ws, depth=dp, image=img, ray_sumsq=sq, grad_c=g_c, grad_h0=g_h0)

    for ray_block in (0, 64):
        rows = (N + 63) // 64 * 64 * T if ray_block else M
        sig_in, rgb_in = f32(np.exp(rng.normal(0, 2, rows))), f32(rng.random((rows, 3)))
        img, dp, ws, masked, sig_rm = full((N, 3)), full(N), full(N), full((M, 3)), full(M) if ray_block else None
        call(lib.foc_fixed_render_inference, ptr(sig_in), ptr(rgb_in), ptr(nears), ptr(fars), ptr(noise), ptr(bg_ray), bg, N, T, ds, thresh, ptr(img), ptr(dp), ptr(ws), ptr(masked),
             ray_block, ptr(sig_rm))
        img2, dp2, ws2, f4 = full((N, 3)), full(N), full(N), full((M, 4))
        call(lib.foc_fixed_field_pack, ptr(sig_in), ptr(rgb_in), ptr(nears), ptr(fars), ptr(noise), ptr(bg_ray), bg, N, T, ds, thresh, ptr(img2), ptr(dp2), ptr(ws2), ptr(f4), ray_block)
        put(f"fixed_inference{tag}[ray_block={ray_block}]", image=img, depth=dp, weights_sum=ws, rgb_masked=masked, sigma_raymajor=sig_rm, pack_image=img2, pack_depth=dp2,
            pack_weights_sum=ws2, field4=f4)


def combine(T):
    from focnerf_amd.combine import HipCombineOps as ops
    rng = np.random.default_rng(300 + T)
    N = 5
    near = rng.uniform(0.1, 0.6, N)
    nears, fars = cuda(near.astype(np.float32)), cuda((near + rng.uniform(0.5, 2.5, N)).astype(np.float32))
    fields = []
    for k in range(3):
        f = rng.random((N, T, 4)); f[..., 0] = np.exp(rng.normal(0, 2, (N, T)))
        fields.append(cuda(f.astype(np.float32)))
    fields[1][0, 0, 0] = NAN32                                             # torch.maximum's NaN propagation
    image4, depth = ops.composite(fields[0][..., 0].contiguous(), fields[0][..., 1:].contiguous(), nears, fars, 1.0)
    res = dict(fixed_image4=image4, fixed_depth=depth)
    for K in (1, 3):
        image4, depth, merged = ops.select_composite(fields[:K], nears, fars, (1.0, 0.0), want_merged=True)
        res.update({f"image4[K={K}]": image4, f"depth[K={K}]": depth, f"merged4[K={K}]": merged})
    image4, depth, att, merged, winner = ops.select_composite_attr(fields, nears, fars, (1.0, 0.0), 3, want_merged=True, want_winner=True)
    res.update(attr_image4=image4, attr_depth=depth, attr_merged4=merged, attr_winner=winner, obj_weights=att.weights, obj_depth=att.depth, instance=att.instance)
    put(f"combine[N={N},T={T}]", **res)


# ---------------------------------------------------------------- marching, inference composite and compaction (raymarching.hip)
MARCH_H = 32
MARCH_FORMS = {"two": 0, "row": 1, "lane": 2, "staged": 3}


def march_scene(bound, n_rays):
    """A random occupancy bitfield (fill 0.5) and rays from around the box towards its middle, with their ranges."""
    C = 1 + int(np.ceil(np.log2(bound)))
    rng = np.random.default_rng(40 + int(bound))
    bits = cuda(rng.integers(0, 256, C * MARCH_H ** 3 // 8).astype(np.uint8))
    o = rng.normal(0, 1, (n_rays, 3)); o *= 1.6 * bound / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.normal(0, 0.35 * bound, (n_rays, 3)) - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = cuda(o.astype(np.float32)), cuda(d.astype(np.float32))
    aabb = cuda(np.array([-bound] * 3 + [bound] * 3, np.float32))
    nears, fars = full(n_rays), full(n_rays)
    call(lib.foc_near_far_from_aabb, ptr(o), ptr(d), ptr(aabb), n_rays, 0.05, ptr(nears), ptr(fars))
    return dict(C=C, bits=bits, o=o, d=d, aabb=aabb, nears=nears, fars=fars, noises=cuda(rng.random(n_rays).astype(np.float32)))


def march_train(bound):
    sc = march_scene(bound, 130)
    C, H = sc["C"], MARCH_H
    for N in (1, 5, 130):
        for max_steps in (7, 64, 1024):
            scratch = torch.zeros(int(lib.foc_march_rays_train_scratch_bytes(N, max_steps)), dtype=torch.uint8, device="cuda")
            for dt_gamma in (0.0, 1 / 128, 0.013):
                for serial in (0, 1):
                    set_option("FOC_MARCH_SERIAL", serial)
                    for base in (0, 37):
                        # forms: plain; the field form with pad_align 0 / 128 and the box (ranges are outputs) or the ranges given
                        forms = [("plain", 0, False)] + [(f"field,pad_align={pa},aabb={box}", pa, box) for pa in (0, 128) for box in (True, False)]
                        for form, pad_align, box in forms:
                            field = form != "plain"

                            def run(M):
                                counter = cuda(np.array([base, 0], np.int32))
                                rays, deltas = full((N, 3), torch.int32), full((max(M, 1), 2))
                                xyzs, dirs, sh = full((max(M, 1), 3)), full((max(M, 1), 3)), full((max(M, 1), 16), torch.float16)
                                nears, fars = (full(N), full(N)) if box else (sc["nears"][:N].clone(), sc["fars"][:N].clone())
                                if field:
                                    call(lib.foc_march_rays_train_field, ptr(sc["o"]), ptr(sc["d"]), ptr(sc["bits"]), bound, dt_gamma, max_steps, N, C, H, M, ptr(nears),
                                         ptr(fars), ptr(xyzs), ptr(sh), ptr(deltas), ptr(rays), ptr(counter), ptr(sc["noises"]), ptr(scratch), pad_align,
                                         ptr(sc["aabb"]) if box else None, 0.05)
                                    return counter, dict(enc_in=xyzs, sh=sh, deltas=deltas, rays=rays, counter=counter, nears=nears, fars=fars)
                                call(lib.foc_march_rays_train, ptr(sc["o"]), ptr(sc["d"]), ptr(sc["bits"]), bound, dt_gamma, max_steps, N, C, H, M, ptr(nears), ptr(fars),
                                     ptr(xyzs), ptr(dirs), ptr(deltas), ptr(rays), ptr(counter), ptr(sc["noises"]), ptr(scratch))
                                return counter, dict(xyzs=xyzs, dirs=dirs, deltas=deltas, rays=rays, counter=counter)
                            counter, _ = run(base + N * max_steps)
                            end = int(counter[0])                                              # base + the samples marched
                            tag = f"march_train[bound={bound},N={N},max_steps={max_steps},dt_gamma={dt_gamma:g},serial={serial},base={base},{form}]"
                            put(tag + "[M=tight]", **run(end)[1])
                            if end > base:
                                put(tag + "[M=short]", **run(end - 1)[1])                      # the last ray with samples does not fit
    set_option("FOC_MARCH_SERIAL", -1)


def march_list(n_rays, length, seed):
    """A list of `length` entries into n_rays rays, about a fifth of them dead (-1) where there is more than one."""
    rng = np.random.default_rng(seed)
    lst = rng.permutation(n_rays)[:length].astype(np.int32)
    if length > 1:
        lst[rng.random(length) < 0.2] = -1
    return cuda(lst)


def march_infer(bound):
    sc = march_scene(bound, 300)
    C, H = sc["C"], MARCH_H
    rng = np.random.default_rng(60 + int(bound))
    # some rays start at their near plane, the others a little way in
    rays_t = torch.where(sc["nears"] < 1e30, sc["nears"] + cuda((rng.random(300) * (rng.random(300) < 0.5)).astype(np.float32)) * 0.5 * bound, sc["nears"])
    for L in (1, 70, 300):
        lst = march_list(300, L, L)
        for dt_gamma, max_steps in ((0.0, 64), (1 / 128, 64), (1 / 128, 1024), (0.013, 64), (0.013, 1024)):
            def run(fn, n_step, *tail):
                x, dd, dl = full((L * n_step, 3)), full((L * n_step, 3)), full((L * n_step, 2))
                call(fn, L, n_step, ptr(lst), ptr(rays_t), ptr(sc["o"]), ptr(sc["d"]), bound, dt_gamma, max_steps, C, H, ptr(sc["bits"]), ptr(sc["nears"]),
                     ptr(sc["fars"]), ptr(x), ptr(dd), ptr(dl), ptr(sc["noises"]), *tail)
                return dict(xyzs=x, dirs=dd, deltas=dl)
            for row_max in (0, 1 << 30):
                set_option("FOC_MARCH_RAYS_ROW_MAX", row_max)
                for n_step in (1, 3, 8, 16):
                    put(f"march_rays[bound={bound},L={L},dt_gamma={dt_gamma:g},max_steps={max_steps},n_step={n_step},row_max={row_max}]", **run(lib.foc_march_rays, n_step))
                for n_step in (1, 2, 4, 8, 16):
                    for form, code in MARCH_FORMS.items():
                        if row_max and form != "two":                      # the walkers of the two phases alone read FOC_MARCH_RAYS_ROW_MAX
                            continue
                        set_option("FOC_OCC_MARCH_FORM", code)
                        for flags in (0, 1, 3, 7):
                            if flags & 4 and not lib.foc_march_rays_two_phase_sample_major(L, n_step, flags):
                                continue
                            scratch = torch.zeros(L + 4, dtype=torch.int32, device="cuda")
                            put(f"march_rays_two_phase[bound={bound},L={L},dt_gamma={dt_gamma:g},max_steps={max_steps},n_step={n_step},row_max={row_max},form={form},flags={flags}]",
                                **run(lib.foc_march_rays_two_phase, n_step, ptr(scratch), flags))
    set_option("FOC_OCC_MARCH_FORM", -1)


def march_composite():
    n_rays = 1500
    for L in (70, 1300):                                                   # (1300: two blocks of the compaction's count)
        lst = march_list(n_rays, L, 7 + L)
        for n_step in (1, 2, 3, 4, 8, 16):
            rng = np.random.default_rng(100 * L + n_step)
            sig = np.exp(rng.normal(0, 2, (L, n_step))).astype(np.float32)
            rgb = rng.random((L, n_step, 3)).astype(np.float32)
            dl = rng.uniform(0.01, 0.2, (L, n_step, 2)).astype(np.float32)
            dl[np.arange(n_step)[None, :] >= rng.integers(0, n_step + 2, L)[:, None]] = 0.0      # a ray fills none, some or all of its slots
            state = [rng.random(n_rays).astype(np.float32), (0.9 * rng.random(n_rays)).astype(np.float32), rng.random(n_rays).astype(np.float32),
                     rng.random((n_rays, 3)).astype(np.float32)]
            for T_thresh in (1e-4, 0.5):
                tag = f"[L={L},n_step={n_step},T_thresh={T_thresh:g}]"
                alive, (t, ws, dp, im) = lst.clone(), map(cuda, state)
                call(lib.foc_composite_rays, L, n_step, T_thresh, ptr(alive), ptr(t), ptr(cuda(sig)), ptr(cuda(rgb)), ptr(cuda(dl)), ptr(ws), ptr(dp), ptr(im))
                put("composite_rays" + tag, rays_alive=alive, rays_t=t, weights_sum=ws, depth=dp, image=im)
                if n_step not in (2, 4, 8):                                # (2: the pointer-walking kernel with the compaction's count)
                    continue
                for sample_major in (0, 1):
                    lay = (lambda a: np.ascontiguousarray(np.moveaxis(a, 0, 1))) if sample_major else (lambda a: a)
                    for with_deaths in (False, True):
                        alive, (t, ws, dp, im) = lst.clone(), map(cuda, state)
                        out, n_out, blocks = full(L, torch.int32), full(1, torch.int32), torch.zeros(L // 1024 + 2, dtype=torch.int32, device="cuda")
                        deaths = torch.zeros(n_step + 1, 64, dtype=torch.int32, device="cuda") if with_deaths else None
                        call(lib.foc_composite_compact, L, n_step, T_thresh, ptr(alive), ptr(t), ptr(cuda(lay(sig))), ptr(cuda(lay(rgb))), ptr(cuda(lay(dl))), ptr(ws),
                             ptr(dp), ptr(im), ptr(out), ptr(n_out), ptr(blocks), ptr(deaths), 1, n_step + 1, sample_major)
                        put(f"composite_compact{tag}[sample_major={sample_major},deaths={with_deaths}]", rays_alive=alive, rays_t=t, weights_sum=ws, depth=dp, image=im,
                            out=out, n_out=n_out, deaths=deaths)
    for n in (1, 1023, 1025, 2100):
        lst = march_list(3000, n, n)
        out, n_out, scratch = full(n, torch.int32), full(1, torch.int32), torch.zeros(n // 1024 + 2, dtype=torch.int32, device="cuda")
        call(lib.foc_compact_alive, ptr(lst), n, ptr(out), ptr(n_out), ptr(scratch))
        put(f"compact_alive[n={n}]", out=out, n_out=n_out)


def march():
    saved = {name: get_option(name) for name in ("FOC_MARCH_SERIAL", "FOC_MARCH_RAYS_ROW_MAX", "FOC_OCC_MARCH_FORM")}
    for bound in (1.0, 2.0):
        march_train(bound)
        march_infer(bound)
    march_composite()
    for name, value in saved.items():
        set_option(name, value)


# ---------------------------------------------------------------- grid encoder (gridencoder.hip, gridencoder_nd.hip)
GRID_PRIMES = np.array([1, 2654435761, 805459861, 3674653429, 2097192037], np.uint64)


def grid_rows(cells, size, stride1, gridtype):
    """Row of every cell tuple [N, D] on a level of `size` rows — gridencoder.cu:50-84 in uint32 arithmetic."""
    m = np.uint64(0xFFFFFFFF)
    cells = cells.astype(np.uint64)
    index, stride = np.zeros(len(cells), np.uint64), 1
    for d in range(cells.shape[1]):
        if stride <= size:
            index = (index + cells[:, d] * np.uint64(stride)) & m
            stride = (stride * stride1) & 0xFFFFFFFF
    if gridtype == 0 and stride > size:
        index = np.zeros(len(cells), np.uint64)
        for d in range(cells.shape[1]):
            index ^= (cells[:, d] * GRID_PRIMES[d]) & m
    return (index % np.uint64(size)).astype(np.int64)


def grid_dtypes(C):
    return [(torch.float32, 0)] + ([(torch.float16, 1)] if C % 2 == 0 else [])


def grid_general():
    from focnerf_amd.gridencoder import level_offsets
    pls, H, log2_hash = 1.5, 4, 11
    S = float(np.log2(pls))
    for D in (2, 3, 4, 5):
        for L in (1, 3, 9):
            for ac in (False, True):
                off = level_offsets(D, L, pls, H, log2_hash, ac)
                d_off = cuda(off)
                for B in (1, 257, 600):
                    rng = np.random.default_rng(100 * D + 10 * L + B)
                    x = rng.random((B, D)).astype(np.float32)
                    if B > 8:
                        x[0], x[1], x[4] = 0.0, 1.0, np.float32(1.0) - np.float32(1e-7)
                        x[2, 0], x[3, D - 1], x[B - 2, 0] = -0.01, 1.0001, 2.5
                    d_x = cuda(x)
                    for C in (1, 2, 4, 8):
                        table = rng.uniform(-1, 1, (int(off[-1]), C)).astype(np.float32)
                        grad = (rng.standard_normal((L, B, C)) * 0.1).astype(np.float32)
                        for tdt, code in grid_dtypes(C):
                            d_t, d_g = cuda(table).to(tdt), cuda(grad).to(tdt)
                            d_g_bl = d_g.permute(1, 0, 2).reshape(B, L * C).contiguous()
                            for gridtype in (0, 1):
                                for interp in (0, 1):
                                    out, out_bl, dy = full((L, B, C), tdt), full((B, L * C), tdt), full((B, L * D * C), tdt)
                                    call(lib.foc_grid_encode_forward, ptr(d_x), ptr(d_t), ptr(d_off), ptr(out), B, D, C, L, S, H, ptr(dy), gridtype, int(ac), interp, code, None)
                                    call(lib.foc_grid_encode_forward_bl, ptr(d_x), ptr(d_t), ptr(d_off), ptr(out_bl), B, D, C, L, S, H, None, gridtype, int(ac), interp, code, None)
                                    dy_bl = full((B, L * D * C), tdt)
                                    call(lib.foc_grid_encode_forward_bl, ptr(d_x), ptr(d_t), ptr(d_off), ptr(out_bl), B, D, C, L, S, H, ptr(dy_bl), gridtype, int(ac), interp, code, None)
                                    res = dict(out=out, out_bl=out_bl, dy_dx=dy, dy_dx_bl=dy_bl)
                                    for bl, g in ((0, d_g), (1, d_g_bl)):
                                        ge, gi = torch.zeros(int(off[-1]), C, dtype=tdt, device="cuda"), full((B, D), tdt)
                                        call(lib.foc_grid_encode_backward, ptr(g), ptr(d_x), ptr(d_t), ptr(d_off), ptr(ge), B, D, C, L, S, H, ptr(dy), ptr(gi), gridtype, int(ac),
                                             interp, code, bl, None)
                                        res[f"grad_inputs[bl={bl}]"] = gi
                                    put(f"grid[D={D},C={C},L={L},B={B},{'f16' if code else 'f32'},gridtype={gridtype},ac={ac},interp={interp}]", **res)


def grid_exact_sums():
    from focnerf_amd.gridencoder import level_offsets
    H, B = 9, 257                                         # one level: scale = 2^0 * 9 - 1 = 8, resolution 9
    for D in (2, 3, 4, 5):
        rng = np.random.default_rng(500 + D)
        # backward: align_corners on, positions on multiples of 1/16 -> in-cell fractions 0 or 0.5, weights multiples of 2^-D
        off = level_offsets(D, 1, 1.0, H, 16, True)
        size = int(off[1])
        x = (rng.integers(0, 17, (B, D)) / 16.0).astype(np.float32)
        pos = x.astype(np.float64) * 8.0
        cell, frac = np.floor(pos), pos - np.floor(pos)
        for C in (1, 2, 4, 8):
            grad = rng.integers(-2, 3, (1, B, C)).astype(np.float32)
            load = np.zeros((size, C))                    # sum of |addends| per table element, float64
            for idx in range(1 << D):
                up = (idx >> np.arange(D)) & 1
                w = np.prod(np.where(up, frac, 1.0 - frac), axis=1)
                assert np.all(w * 32 == np.round(w * 32))                          # every addend a multiple of 2^-5
                np.add.at(load, grid_rows(cell + up, size, H, 0), np.abs(w[:, None] * grad[0]))
            assert load.max() < 64.0, load.max()                                   # below 2^6: fp16 / fp32 adds are exact in any order
            for tdt, code in grid_dtypes(C):
                d_g = cuda(grad).to(tdt)
                for bl, g in ((0, d_g), (1, d_g.permute(1, 0, 2).reshape(B, C).contiguous())):
                    ge = torch.zeros(size, C, dtype=tdt, device="cuda")
                    call(lib.foc_grid_encode_backward, ptr(g), ptr(cuda(x)), None, ptr(cuda(off)), ptr(ge), B, D, C, 1, 0.0, H, None, None, 0, 1, 0, code, bl, None)
                    put(f"grid_backward_exact[D={D},C={C},{'f16' if code else 'f32'},bl={bl}]", grad_embeddings=ge)
        # grad_total_variation: a tiled level, align_corners off, every point in a cell and a row of its own
        off = level_offsets(D, 1, 1.0, H, 16, False)
        size = int(off[1])
        n = min(200, 8 ** D // 2)
        flat = rng.permutation(8 ** D)[:n]
        cell = 1 + np.stack([(flat // 8 ** d) % 8 for d in range(D)], axis=1)       # cells 1..8 per axis
        xs = ((cell - 0.25) / 8.0).astype(np.float32)                               # floor(x * 8 + 0.5) = cell; exact in fp16
        rows = grid_rows(cell, size, H + 1, 1)
        assert len(np.unique(cell, axis=0)) == n and len(np.unique(rows)) == n
        for C in (1, 2, 4, 8):
            table = rng.uniform(-1, 1, (size, C)).astype(np.float32)
            for tdt, code in grid_dtypes(C):
                d_x = cuda(xs).to(tdt)
                assert np.array_equal(np.floor(d_x.float().cpu().numpy().astype(np.float64) * 8.0 + 0.5), cell)
                tv = torch.zeros(size, C, dtype=tdt, device="cuda")
                call(lib.foc_grad_total_variation, ptr(d_x), ptr(cuda(table).to(tdt)), ptr(tv), ptr(cuda(off)), 0.01, n, D, C, 1, 0.0, H, 1, 0, code)
                put(f"grid_tv_exact[D={D},C={C},{'f16' if code else 'f32'}]", grad=tv)


def grid():
    grid_general()
    grid_exact_sums()


# ---------------------------------------------------------------- the occupancy node and the native render loop, from Python
NODE_KINDS = ("plain", "linear_bg", "tcnn_legacy", "foc", "tcnn")
MARCHED = []         # samples marched by each training step of the node section (the summary says which remainders they leave)


def node_model(kind, bound=2):
    from focnerf_amd import network, network_foc, network_linear, network_tcnn, network_tcnn_legacy, synthetic
    torch.manual_seed(0)
    if kind == "plain":
        m = network.NeRFNetwork(bound=bound, cuda_ray=True).cuda()
    elif kind == "linear_bg":
        m = network_linear.NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05, bg_radius=32.0).cuda()
    elif kind == "tcnn_legacy":
        m = network_tcnn_legacy.NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05).cuda()
    else:
        m = {"foc": network_foc, "tcnn": network_tcnn}[kind].NeRFNetwork(bound=bound, cuda_ray=True).cuda()
    with torch.no_grad():
        m.encoder.embeddings.uniform_(-0.5, 0.5)
        if kind == "linear_bg":
            m.encoder_bg.embeddings.uniform_(-1.0, 1.0)
            for layer in list(m.sigma_net) + list(m.color_net):
                layer.weight.mul_(3.0)
    m.set_density_grid(synthetic.analytic_density_grid(bound, device="cuda"))
    return m


def node_rays(bound, n, seed, w=64):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(w, w, bound, 1, seed=seed, device="cuda")
    pick = torch.randperm(o.shape[1], generator=torch.Generator().manual_seed(seed))[:n].cuda()
    return o[:, pick].contiguous(), d[:, pick].contiguous()


def node_step(case, m, o, d, yolo, **kw):
    """One training step of `m.render` (the jitter seeded) -> the digests of its outputs and of every parameter gradient."""
    m.train()
    m.zero_grad(set_to_none=True)
    torch.manual_seed(7)
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(o, d, yolo, staged=False, dt_gamma=1 / 128, perturb=True, **kw)
        loss = torch.nn.functional.mse_loss(out["image"], 0.5 + 0.5 * torch.sin(3.0 * d)) + 1e-3 * out["weights_sum"].mean()
        crit = out.get("criterion_outside_mask")
        if crit is not None:
            loss = loss + 1e-3 * crit
    (loss * 4096.0).backward()
    grads = {"grad." + name: p.grad for name, p in m.named_parameters() if p.grad is not None}
    marched = m.step_counter[(m.local_step - 1) % 16]
    put(case, image=out["image"], depth=out["depth"], weights_sum=out["weights_sum"], criterion_outside_mask=crit, marched=marched, **grads)
    MARCHED.append(int(marched[0]))


def node():
    from focnerf_amd import deterministic
    bound = 2
    backgrounds = {1: None, 63: 0.25, 64: "ray", 65: None, 300: "ray"}
    with deterministic():
        for kind in NODE_KINDS:
            m = node_model(kind, bound)
            with_object = kind in ("foc", "tcnn")
            for n, bg in backgrounds.items():
                o, d = node_rays(bound, n, 3 + n)
                g = torch.Generator().manual_seed(n)
                bg_color = torch.rand(n, 3, generator=g).cuda() if bg == "ray" else bg
                feature = torch.randn(144, generator=g).cuda()
                masks = ((torch.rand(1, n, generator=g) < 0.5).cuda(), None) if with_object else (None,)
                for mask in masks:
                    yolo = (mask, None, feature) if with_object else None
                    for max_steps in (16, 64):
                        # the budgeted list (mean_count > 0) is what the one-call node takes: room for every sample; at 300 rays also a
                        # list that drops the last rays, and the unbudgeted list (cut to the samples marched) through the chain
                        lists = [("room", n * max_steps, False)] + ([("overflow", 2 * max_steps, False), ("all_rays", -1, True)] if n == 300 else [])
                        for name, mean_count, force_all_rays in lists:
                            for native in ("1", "0"):
                                os.environ["FOC_OCC_NATIVE_NODE"] = native
                                m.mean_count = mean_count
                                node_step(f"node[{kind},n={n},max_steps={max_steps},bg={bg},mask={mask is not None},list={name},native={native}]", m, o, d, yolo,
                                          max_steps=max_steps, bg_color=bg_color, force_all_rays=force_all_rays)
            os.environ.pop("FOC_OCC_NATIVE_NODE", None)
            # one evaluation view through the native render loop
            m.eval()
            o, d = node_rays(bound, 32 * 32, 5, w=32)
            yolo = (None, None, torch.randn(144, generator=torch.Generator().manual_seed(5)).cuda()) if with_object else None
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                out = m.render(o, d, yolo, staged=False, dt_gamma=1 / 128, max_steps=64, perturb=False, bg_color=1.0)
            put(f"render_loop[{kind}]", image=out["image"], depth=out["depth"])
            del m


# ---------------------------------------------------------------- fused MLP family (ffmlp.hip, field_fwd.hip, normals.hip) through the C ABI
MLP_ROWS = (1, 31, 33, 65, 129, 257)
MLP_PAIRS = ((1, 2), (1, 3), (2, 2), (2, 3), (3, 3))     # (sigma_layers, color_layers) the kernels of both networks are built for
ACT_RELU, ACT_SIGMOID, ACT_NONE = 0, 3, 6


def mlp_half(rng, shape, scale):
    return cuda((rng.standard_normal(shape) * scale).astype(np.float16))


def mlp_blob(rng, in_dim, hidden, layers):
    return mlp_half(rng, hidden * (in_dim + hidden * (layers - 1) + 16), 0.25)


def mlp_planes(x):
    """[B, in_dim] rows as the encoder's [in_dim / 2, B, 2] planes."""
    B, in_dim = x.shape
    return x.view(B, in_dim // 2, 2).permute(1, 0, 2).contiguous()


def mlp_plain():
    ws = torch.empty(max(int(lib.foc_ffmlp_backward_workspace_bytes(64, h, 3)) for h in (16, 32, 64, 128)), dtype=torch.uint8, device="cuda")
    for hidden in (16, 32, 64, 128):
        for layers in (1, 2, 3):
            for in_dim in (16, 32, 64):
                for act in (ACT_RELU, ACT_NONE, ACT_SIGMOID):
                    for B in MLP_ROWS:
                        rng = np.random.default_rng(((hidden * 10 + layers) * 100 + in_dim) * 1000 + 10 * B + act)
                        x, W, grad = mlp_half(rng, (B, in_dim), 1.0), mlp_blob(rng, in_dim, hidden, layers), mlp_half(rng, (B, 16), 0.1)
                        xp = mlp_planes(x)
                        tag = f"[hidden={hidden},layers={layers},in={in_dim},act={act},B={B}]"
                        f16 = lambda *shape: full(shape, torch.float16)
                        fb, out, out_inf, ib = f16(layers, B, hidden), f16(B, 16), f16(B, 16), f16(B, hidden)
                        call(lib.foc_ffmlp_forward, ptr(x), ptr(W), B, in_dim, 16, hidden, layers, act, ACT_NONE, ptr(fb), ptr(out))
                        call(lib.foc_ffmlp_inference, ptr(x), ptr(W), B, in_dim, 16, hidden, layers, act, ACT_NONE, ptr(ib), ptr(out_inf))
                        res = dict(outputs=out, forward_buffer=fb, inference=out_inf)
                        if act != ACT_SIGMOID:                               # the general activations are served on row-major inputs only
                            res["planar"] = f16(B, 16)
                            call(lib.foc_ffmlp_forward_planar, ptr(xp), ptr(W), B, in_dim, 16, hidden, layers, act, ACT_NONE, ptr(res["planar"]))
                        put("ffmlp_forward" + tag, **res)
                        for fused in (1, 0):
                            set_option("FOC_MLP_BWD_FUSED", fused)
                            one_pass = fused and hidden <= 64 and act != ACT_SIGMOID        # the shapes k_mlp_bwd_fused serves (in_dim <= 64, layers <= 4 here)
                            res = {}
                            # stored activations with the backward buffer; then (single-pass kernel only) re-evaluated ones, with and without it; then planar
                            forms = [("stored", fb, True, False)] + ([("recomp", None, False, False), ("recomp+bb", None, True, False), ("planar", None, False, True)] if one_pass else [])
                            for name, fwd, with_bb, planar in forms:
                                bb, gi, gw = f16(layers, B, hidden) if with_bb else None, f16(*((in_dim // 2, B, 2) if planar else (B, in_dim))), f16(W.numel())
                                if planar:
                                    call(lib.foc_ffmlp_backward_planar, ptr(grad), ptr(xp), ptr(W), B, in_dim, 16, hidden, layers, act, ACT_NONE, 1, ptr(gi), ptr(gw), ptr(ws), ws.numel())
                                else:
                                    call(lib.foc_ffmlp_backward, ptr(grad), ptr(x), ptr(W), ptr(fwd), B, in_dim, 16, hidden, layers, act, ACT_NONE, 1, ptr(bb), ptr(gi), ptr(gw),
                                         ptr(ws), ws.numel())
                                res.update({f"grad_inputs[{name}]": gi, f"grad_weights[{name}]": gw, f"backward_buffer[{name}]": bb})
                            put(f"ffmlp_backward{tag}[fused={fused}]", **res)
    set_option("FOC_MLP_BWD_FUSED", 1)


def mlp_head_forms(rng):
    """(suffix, object feature, input_pad) of an entry point and its _pad / _pad31 twins; input_pad None: the entry point takes none."""
    obj = mlp_half(rng, 16, 0.8)
    return (("", None, None), ("", obj, None), ("_pad", obj, 1.0), ("_pad31", None, 1.0))


def mlp_fields():
    T = 4                                                                   # samples per ray
    ws = torch.empty(int(lib.foc_ffmlp_backward_workspace_bytes(48, 64, 3)), dtype=torch.uint8, device="cuda")
    for B in MLP_ROWS:
        rng = np.random.default_rng(7000 + B)
        n_rays = (B + T - 1) // T
        x, hrows, ray_sh = mlp_half(rng, (B, 32), 1.0), mlp_half(rng, (B, 16), 0.7), mlp_half(rng, (n_rays, 16), 0.5)
        xp, g_h0 = mlp_planes(x), mlp_half(rng, B, 0.05)
        for suffix, obj, pad in mlp_head_forms(rng):
            pad_args = () if pad is None else (pad,)
            form = f"{suffix or 'plain'},obj={obj is not None}"
            ld0 = 48 if obj is not None else 32
            for layers in (2, 3):
                W = mlp_blob(rng, ld0, 64, layers)
                for cw in (4, 16):
                    grad = mlp_half(rng, (B, cw), 0.05)
                    for act in (ACT_RELU, ACT_NONE):
                        out, g_h, g_w = full((B, cw), torch.float16), full((B, 16), torch.float16), full(W.numel(), torch.float16)
                        g_obj = full(16) if obj is not None else None
                        call(getattr(lib, "foc_color_head_forward" + suffix), ptr(hrows), ptr(ray_sh), T, ptr(W), B, 64, layers, act, ptr(out), cw, ptr(obj), *pad_args)
                        call(getattr(lib, "foc_color_head_backward" + suffix), ptr(grad), ptr(hrows), ptr(ray_sh), T, ptr(g_h0), ptr(W), B, 64, layers, act, ptr(g_h), ptr(g_w),
                             ptr(ws), ws.numel(), cw, ptr(obj), ptr(g_obj), *pad_args)
                        put(f"color_head[{form},layers={layers},c_width={cw},act={act},B={B}]", outputs=out, grad_h=g_h, grad_w=g_w, grad_obj=g_obj)
            for nls, nlc in MLP_PAIRS:
                Ws, Wc = mlp_blob(rng, 32, 64, nls), mlp_blob(rng, ld0, 64, nlc)
                for act in (ACT_RELU, ACT_NONE):
                    for cw in (4, 16):
                        h, c = full((B, 16), torch.float16), full((B, cw), torch.float16)
                        call(getattr(lib, "foc_field_forward_train" + suffix), ptr(xp), ptr(Ws), nls, ptr(ray_sh), T, ptr(Wc), nlc, 64, act, B, ptr(h), ptr(c), cw, ptr(obj), *pad_args)
                        put(f"field_forward_train[{form},layers={nls}/{nlc},act={act},c_width={cw},B={B}]", h=h, c=c)
                # the inference of both networks: an object feature or a pad goes with the planes and ReLU
                for planar, dir_block in ((1, 0), (1, 64), (0, 0), (0, 64)):
                    if not planar and (obj is not None or pad is not None):
                        continue
                    for dir_div in (1, 4):
                        n_dirs = (B + dir_div - 1) // dir_div
                        dirs = rng.standard_normal((n_dirs, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
                        d_dirs = cuda(dirs.astype(np.float32))
                        for act in (ACT_RELU,) if (obj is not None or pad is not None) else (ACT_RELU, ACT_NONE):
                            sigma, rgb = full(B), full((B, 3))
                            call(getattr(lib, "foc_nerf_field_inference" + suffix), ptr(xp if planar else x), planar, ptr(d_dirs), dir_div, dir_block, n_dirs, ptr(Ws), nls, ptr(Wc), nlc,
                                 64, act, B, ptr(sigma), ptr(rgb), ptr(obj), *pad_args)
                            put(f"nerf_field_inference[{form},layers={nls}/{nlc},planar={planar},dir_block={dir_block},dir_div={dir_div},act={act},B={B}]", sigma=sigma, rgb=rgb)


def mlp_normals():
    from focnerf_amd.gridencoder import level_offsets
    pls, H, L = 1.5, 4, 16
    off = level_offsets(3, L, pls, H, 11)
    rng = np.random.default_rng(9000)
    table, d_off = cuda(rng.uniform(-0.5, 0.5, (int(off[-1]), 2)).astype(np.float16)), cuda(off)
    rot = np.linalg.qr(rng.standard_normal((3, 3)))[0].astype(np.float32)
    for M in MLP_ROWS:
        x = rng.random((M, 3)).astype(np.float32)
        if M > 8:
            x[0], x[1], x[2, 0] = 0.0, 1.0, -0.01                           # the box's corners and a point outside it
        d_x = cuda(x)
        for nls in (1, 2, 3):
            W = mlp_blob(rng, 32, 64, nls)
            for rot9 in (None, cuda(rot)):
                sigma, g_raw, n_rgb, g_enc = full(M), full((M, 3)), full((M, 3)), full((M, 32))
                call(lib.foc_field_normals, ptr(d_x), M, ptr(table), ptr(d_off), 3, 2, L, float(np.log2(pls)), H, 0, 0, 0, 1, None, ptr(W), nls, 64, ACT_RELU, ptr(rot9), ptr(sigma),
                     ptr(g_raw), ptr(n_rgb), ptr(g_enc))
                put(f"field_normals[layers={nls},rot={rot9 is not None},M={M}]", sigma=sigma, grad_raw=g_raw, normal_rgb=n_rgb, grad_enc=g_enc)


def mlp():
    saved = {name: get_option(name) for name in ("FOC_DETERMINISTIC", "FOC_MLP_BWD_FUSED")}
    try:
        set_option("FOC_DETERMINISTIC", 1)                                  # the weight gradients of the two-kernel backward: sums in a fixed order
        mlp_plain()
        mlp_fields()
        mlp_normals()
    finally:
        for name, value in saved.items():
            set_option(name, value)


def main():
    if "mlp" in SECTIONS:
        mlp()
    if "per_sample" in SECTIONS:
        per_sample()
    if "ragged" in SECTIONS:
        ragged()
    for N in (1, 5, 130) if "fixed" in SECTIONS else ():
        for T in (2, 65, 130):
            for noisy in (False, True):
                for per_ray_bg in (False, True):
                    for ds in (1.0, 2.0):
                        fixed(N, T, noisy, per_ray_bg, ds)
    for T in (2, 65, 130) if "combine" in SECTIONS else ():
        combine(T)
    if "march" in SECTIONS:
        march()
    if "grid" in SECTIONS:
        grid()
    if "node" in SECTIONS:
        node()
    text = json.dumps(OUT, indent=0, sort_keys=True)
    if not ARGS:
        print(text)
        return
    with open(ARGS[0], "w") as f:
        f.write(text + "\n")
    summary = {"cases": len(OUT), "outputs": sum(len(v) for v in OUT.values()), "sha256": hashlib.sha256(text.encode()).hexdigest()}
    if MARCHED:
        summary["node_marched"] = {"min": min(MARCHED), "max": max(MARCHED), "not_multiple_of_8": sum(c % 8 != 0 for c in MARCHED),
                                   "multiple_of_32": sum(c % 32 == 0 for c in MARCHED)}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
