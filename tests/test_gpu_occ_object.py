"""GPU: the object-conditioned networks (network_foc.py, network_tcnn.py) on the occupancy-grid path.

  1. the feature is used: two object features give two images (training and eval), the object encoder gets gradients, the criterion is there;
  2. the op chain (FOC_FUSED_OCC=0) is march_rays_train -> net(x, d, (None, None, obj16)) -> composite_rays_train, bit for bit;
  3. the node (occtrain._occ_train with the feature) against that chain, on the cases of tests/test_gpu_occtrain.py;
  4. the criterion kernels (foc_occ_tail_forward_sumsq / _backward_sumsq) against a float64 torch expression;
  5. the node as one library call against the call-by-call node, bit for bit;
  6. inference: the native loop against the Python loop, bit for bit;
  7. deterministic mode and graph replay;
  8. three hundred training steps and a checkpoint.
Tolerances are those of the tests named at each comparison; bounds stated here are derived where they stand."""
import math

import numpy as np
import pytest
import torch

from util import to_np

pytestmark = pytest.mark.gpu

FP16_EPS = 2.0 ** -10
# The loss scale of the fp16 tests next door (tests/test_gpu_network_tcnn_layout.py): without it the per-sample gradients of a 1500-ray
# mean-squared error are ~1e-6, far below fp16's smallest normal number 6.1e-5 — both routes would round them on the subnormal grid
# (steps of 6e-8), each at its own places, and the comparison would measure that rounding instead of the routes.
LOSS_SCALE = 4096.0
KINDS = ["foc", "tcnn"]
RENDER = dict(staged=False, dt_gamma=1 / 128, max_steps=1024)


def _cls(kind):
    from focnerf_amd import network_foc, network_tcnn
    return {"foc": network_foc.NeRFNetwork, "tcnn": network_tcnn.NeRFNetwork}[kind]


def _model(kind, bound=2, seed=0, density_scale=1):
    from focnerf_amd import synthetic
    torch.manual_seed(seed)
    m = _cls(kind)(bound=bound, cuda_ray=True, density_scale=density_scale).cuda()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    m.color_net.weights.data.mul_(1.5)
    m.set_density_grid(synthetic.analytic_density_grid(bound, device="cuda"))
    return m.train()


def _rays(bound, n, seed):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(64, 64, bound, 1, seed=seed, device="cuda")
    pick = torch.randperm(o.shape[1], generator=torch.Generator().manual_seed(seed))[:n].cuda()
    return o[:, pick].contiguous(), d[:, pick].contiguous()


def _yolo(n, seed, share=0.5, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(1, n, generator=g) < share).cuda(), None, (torch.randn(144, generator=g) * scale).cuda())


def _count_calls(monkeypatch, names):
    from focnerf_amd._lib import lib
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)
        monkeypatch.setattr(lib, n, lambda *a, _r=real, _n=n: (calls.__setitem__(_n, calls[_n] + 1), _r(*a))[1])
    return calls


def _step(m, o, d, yolo, monkeypatch, fused, seed=7, crit_weight=1e-3, **kw):
    """One training step (loss x LOSS_SCALE into the backward) -> (result, gradients of the table, both blobs, the object encoder's
    parameters and the encoded feature)."""
    monkeypatch.setenv("FOC_FUSED_OCC", "1" if fused else "0")
    for p in m.parameters():
        p.grad = None
    kept = {}

    def encode(y, dev):
        kept["obj16"] = type(m).encode_object_feature(m, y, dev)
        kept["obj16"].retain_grad()
        return kept["obj16"]
    m.encode_object_feature = encode
    try:
        torch.manual_seed(seed)                                  # the jitter of `perturb` comes from torch.rand(n) in both routes
        with torch.autocast("cuda", dtype=torch.float16):
            out = m.render(o, d, yolo, **RENDER, **kw)
            target = 0.5 + 0.5 * torch.sin(3.0 * d)
            loss = torch.nn.functional.mse_loss(out["image"], target) + 1e-3 * out["weights_sum"].mean()
            if out.get("criterion_outside_mask") is not None:
                loss = loss + crit_weight * out["criterion_outside_mask"]
        (loss * LOSS_SCALE).backward()
        torch.cuda.synchronize()
    finally:
        del m.encode_object_feature
    # every gradient stays in the units the backward ran in (the scaled loss): the bounds below are stated in those units
    grads = {"embeddings": m.encoder.embeddings.grad.clone(), "sigma_net": m.sigma_net.weights.grad.clone(), "color_net": m.color_net.weights.grad.clone(),
             "obj16": kept["obj16"].grad.clone()}
    grads.update({"yolo." + k: p.grad.clone() for k, p in m.yolo_feat_encoder.named_parameters()})
    return out, grads


def _encoder_abs_jacobian(m, yolo):
    """{parameter name: sum over the 16 outputs k of |d obj16[k] / d parameter|} of the object encoder at `yolo`, in the autocast mode of `_step`."""
    names, params = zip(*m.yolo_feat_encoder.named_parameters())
    with torch.autocast("cuda", dtype=torch.float16):
        obj16 = type(m).encode_object_feature(m, yolo, torch.device("cuda"))
    total = [torch.zeros_like(p, dtype=torch.float64) for p in params]
    for k in range(obj16.numel()):
        for t, g in zip(total, torch.autograd.grad(obj16.reshape(-1)[k], params, retain_graph=True, allow_unused=True)):
            if g is not None:
                t += g.double().abs()
    return dict(zip(names, total))


def _same_bits(a, b):
    a, b = to_np(a), to_np(b)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


# ---------------------------------------------------------------- 1. the feature is used
@pytest.mark.parametrize("kind", KINDS)
def test_the_object_feature_reaches_the_image_and_the_encoder(kind, monkeypatch):
    m = _model(kind)
    o, d = _rays(2, 1500, 3)
    a_yolo, b_yolo = _yolo(1500, 1), _yolo(1500, 2)
    out_a, g = _step(m, o, d, a_yolo, monkeypatch, True, perturb=False, force_all_rays=True)
    out_b, _ = _step(m, o, d, b_yolo, monkeypatch, True, perturb=False, force_all_rays=True)
    assert "criterion_outside_mask" in out_a and float(out_a["criterion_outside_mask"]) > 0
    assert not torch.equal(out_a["image"], out_b["image"])
    assert torch.equal(out_a["weights_sum"], out_b["weights_sum"])          # the density does not know the object
    enc = [k for k in g if k.startswith("yolo.")]
    assert enc and all(float(g[k].abs().max()) > 0 and bool(torch.isfinite(g[k]).all()) for k in enc), {k: float(g[k].abs().max()) for k in enc}
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ea = m.render(o, d, a_yolo, perturb=False, bg_color=1.0, **RENDER)
        eb = m.render(o, d, b_yolo, perturb=False, bg_color=1.0, **RENDER)
        plain = m.render(o, d, perturb=False, bg_color=1.0, **RENDER)
    assert "criterion_outside_mask" in ea and ea["criterion_outside_mask"] is None
    assert not torch.equal(ea["image"], eb["image"]) and torch.equal(ea["depth"], eb["depth"])
    assert "criterion_outside_mask" not in plain                             # no yolo_details: the call it always was
    m.train()
    with torch.autocast("cuda", dtype=torch.float16):
        no_mask = m.render(o, d, (None, None, a_yolo[2]), perturb=False, **RENDER)
    assert "criterion_outside_mask" in no_mask and no_mask["criterion_outside_mask"] is None
    assert torch.equal(no_mask["image"], out_a["image"])


# ---------------------------------------------------------------- 2. the op chain
@pytest.mark.parametrize("kind", KINDS)
def test_op_chain_is_the_public_ops_with_the_encoded_feature(kind, monkeypatch):
    from focnerf_amd import raymarching
    from focnerf_amd.renderer import _MARCH_ALIGN
    m = _model(kind, seed=1)
    o, d = _rays(2, 1200, 4)
    yolo = _yolo(1200, 5)
    monkeypatch.setenv("FOC_FUSED_OCC", "0")
    with torch.autocast("cuda", dtype=torch.float16):
        got = m.render(o, d, yolo, perturb=False, force_all_rays=True, **RENDER)
        o2, d2 = o[0].contiguous(), d[0].contiguous()
        near, far = raymarching.near_far_from_aabb(o2, d2, m._aabb(), m.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device="cuda")
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(o2, d2, m.bound, m.density_bitfield, m.cascade, m.grid_size, near, far, counter, m.mean_count,
                                                                False, _MARCH_ALIGN, True, 1 / 128, 1024)
        obj16 = m.encode_object_feature(yolo, o.device)
        sigmas, rgbs = m(xyzs, dirs, (None, None, obj16))
        ws, depth, image = raymarching.composite_rays_train(sigmas, rgbs, deltas, rays, 1e-4)
        image = image + (1 - ws).unsqueeze(-1)
        depth = torch.clamp(depth - near, min=0) / (far - near)
    assert float(ws.max()) > 0.5
    assert _same_bits(got["image"].view(-1, 3), image) and _same_bits(got["weights_sum"], ws) and _same_bits(got["depth"].view(-1), depth)
    # the criterion of the chain: float64 over the same list
    s64 = sigmas.detach().double()
    outside = ~yolo[0].reshape(-1)
    total = torch.zeros((), dtype=torch.float64, device="cuda")
    for index, first, count in rays.tolist():
        if count > 0 and first + count <= s64.shape[0] and bool(outside[index]):
            total += (s64[first: first + count] ** 2).sum()
    assert float(got["criterion_outside_mask"]) == pytest.approx(float(total.sqrt()), rel=1e-5)


# ---------------------------------------------------------------- 3. the node against the chain
@pytest.mark.parametrize("case", ["all_rays", "budget", "budget_overflow", "per_ray_bg", "grey_bg_scaled"])
@pytest.mark.parametrize("kind", KINDS)
def test_object_node_equals_the_op_chain(kind, case, monkeypatch):
    """Same sample list: weights_sum and depth bit for bit (the density network runs the same kernels), image within 1e-4 (the object's share
    enters layer 0 as a start value rather than as columns: tests/test_gpu_network_foc.py), gradients of the table and both blobs within
    4e-3 of their range (tests/test_gpu_occtrain.py), the encoded feature's within 1e-2 scale + 1e-6 M (test_gpu_network_foc.py), the
    criterion within 1e-5 (an fp32 sum in another order).

    The feature's bound, in the units the backward ran in (the loss x LOSS_SCALE; nothing is divided out): the chain sums M per-sample
    gradients of the object columns, each rounded to fp16, the node sums delta_0 in fp32 first — 1e-2 of the range for the fp16 factors,
    1e-6 per sample of the list for the per-sample rounding, M = the samples the list holds. The encoder's parameters receive
    J^T grad_obj16 in fp32 on both routes with the same J (the encoder's forward is the same call), so their gradients differ by at most
    |J|^T tol(obj16) elementwise, plus the fp32 rounding of those 16-term sums (1e-5 of |J|^T |grad_obj16|)."""
    bound, n = 2, 1500
    m = _model(kind, density_scale=2 if case == "grey_bg_scaled" else 1)
    o, d = _rays(bound, n, 3)
    yolo = _yolo(n, 11)
    kw = dict(perturb=True, force_all_rays=case == "all_rays", bg_color=None)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        m.render(o, d, perturb=False, force_all_rays=True, **RENDER)            # fills step_counter
    total = int(m.step_counter[(m.local_step - 1) % 16, 0])
    assert total > 1000
    if case.startswith("budget"):
        m.mean_count = total + 500 if case == "budget" else total // 2        # a list with room to spare / one that drops the last rays
    if case == "per_ray_bg":
        kw["bg_color"] = torch.rand(n, 3, device="cuda")
    if case == "grey_bg_scaled":
        kw["bg_color"] = 0.25
    ref, g_ref = _step(m, o, d, yolo, monkeypatch, False, **kw)
    got, g_got = _step(m, o, d, yolo, monkeypatch, True, **kw)
    for k in ("depth", "weights_sum"):
        assert _same_bits(ref[k], got[k]), f"{case}: {k} differs, max {np.nanmax(np.abs(to_np(ref[k]) - to_np(got[k])))}"
    diff = float((ref["image"] - got["image"]).abs().max())
    print(f"\n{kind} {case}: image max |node - chain| {diff:.3e}; criterion {float(ref['criterion_outside_mask']):.6g} vs {float(got['criterion_outside_mask']):.6g}")
    assert diff <= 1e-4, f"{case}: image differs by {diff}"
    assert to_np(ref["weights_sum"]).max() > 0.5
    assert float(got["criterion_outside_mask"]) == pytest.approx(float(ref["criterion_outside_mask"]), rel=1e-5)
    if case == "budget_overflow":
        assert (to_np(got["weights_sum"]) == 0).sum() > (to_np(_step(m, o, d, yolo, monkeypatch, True, perturb=True, force_all_rays=True)[0]["weights_sum"]) == 0).sum()
    for name in ("embeddings", "sigma_net", "color_net"):
        a, b = to_np(g_ref[name]).astype(np.float64), to_np(g_got[name]).astype(np.float64)
        scale = np.abs(a).max()
        print(f"  grad {name}: off by {np.abs(a - b).max() / scale:.2e} of its range")
        assert scale > 0 and np.abs(a - b).max() <= 4e-3 * scale, f"{case}: grad {name} off by {np.abs(a - b).max() / scale:.2e} of its range"
    a, b = to_np(g_ref["obj16"]).astype(np.float64), to_np(g_got["obj16"]).astype(np.float64)
    scale, M = np.abs(a).max(), (total // 2 if case == "budget_overflow" else total)
    tol = 1e-2 * scale + 1e-6 * M
    print(f"  grad obj16: max diff {np.abs(a - b).max():.3e}, scale {scale:.3e}, bound {tol:.3e} (M {M})")
    assert scale > 0 and np.abs(a - b).max() <= tol, f"{case}: grad obj16 {np.abs(a - b).max()} vs scale {scale}, bound {tol}"
    assert scale > 4 * tol, "the bound would pass a zero gradient"
    absj = _encoder_abs_jacobian(m, yolo)
    for name, j in absj.items():
        pa, pb = to_np(g_ref["yolo." + name]).astype(np.float64), to_np(g_got["yolo." + name]).astype(np.float64)
        bound = to_np(j) * (tol + 1e-5 * scale)
        print(f"  grad yolo.{name}: max diff {np.abs(pa - pb).max():.3e}, scale {np.abs(pa).max():.3e}, largest bound {bound.max():.3e}")
        assert np.abs(pa).max() > 0 and (np.abs(pa - pb) <= bound).all(), f"{case}: grad yolo.{name} off by {np.abs(pa - pb).max()} (bound {bound.max()})"


# ---------------------------------------------------------------- 4. the criterion kernels
def _ragged_case(seed=0):
    """A hand-made ragged list: rays of 1..150 samples (more than one block of 64 among them), an empty ray, rays dense enough to stop early,
    and a last ray that does not fit the list (budget overflow). -> tensors and the float64 transmittance bookkeeping."""
    g = torch.Generator().manual_seed(seed)
    counts = [150, 1, 64, 65, 0, 130, 17, 90, 128, 40, 70, 33]
    N = len(counts)
    order = torch.randperm(N, generator=g).tolist()                      # ray n of the list is image row order[n]
    firsts, at = [], 0
    for c in counts:
        firsts.append(at)
        at += c
    marched = at
    M = marched - 20                                                     # the last ray (33 samples) overflows the budget
    M_alloc = ((M + 127) // 128) * 128 + 128                             # rows behind the last ray: zeroed by the spare workgroups
    rays = torch.tensor([[order[i], firsts[i], counts[i]] for i in range(N)], dtype=torch.int32)
    h = (torch.randn(M_alloc, 16, generator=g) * 0.7).half()
    h0 = torch.randn(M_alloc, generator=g) * 1.5 - 1.0
    for i in (0, 5, 8):                                                  # dense rays: sigma ~ e^6, dt 0.02 -> opaque after a few samples
        h0[firsts[i] + 5: firsts[i] + counts[i]] = 6.0 + torch.rand(counts[i] - 5, generator=g)
    h[:, 0] = h0.half()
    c = (torch.randn(M_alloc, 4, generator=g)).half()
    deltas = torch.stack([torch.full((M_alloc,), 0.02), torch.full((M_alloc,), 0.02)], 1).contiguous()
    nears, fars = torch.full((N,), 0.2), torch.full((N,), 4.0)
    counter = torch.tensor([marched, N], dtype=torch.int32)
    return dict(N=N, M=M_alloc, budget=M, rays=rays.cuda(), h=h.cuda(), c=c.cuda(), deltas=deltas.cuda(), nears=nears.cuda(), fars=fars.cuda(),
                counter=counter.cuda(), counts=counts, firsts=firsts, order=order)


def _tail(case, M, sumsq, grad_image, grad_ws, grad_sumsq):
    """Forward and backward of the ragged tail on `case` with list length M; sumsq / grad_sumsq None: the plain entry points."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    N = case["N"]
    out = torch.empty(N * 8, dtype=torch.float32, device="cuda")
    ws, depth, raw, image = out[:N], out[N: 2 * N], out[2 * N: 5 * N].view(N, 3), out[5 * N:].view(N, 3)
    st = stream_of(out)
    fwd = (ptr(case["h"]), ptr(case["c"]), 4, ptr(case["deltas"]), ptr(case["rays"]), M, N, 1e-4, 1.0, None, 1.0, ptr(case["nears"]), ptr(case["fars"]),
           ptr(ws), ptr(raw), ptr(image), ptr(depth))
    if sumsq is not None:
        check(lib.foc_occ_tail_forward_sumsq(*fwd, ptr(sumsq), st), "occ_tail_forward_sumsq")
    else:
        check(lib.foc_occ_tail_forward(*fwd, st), "occ_tail_forward")
    grad_c = torch.full((M, 4), float("nan"), dtype=torch.float16, device="cuda")
    grad_h0 = torch.full((M,), float("nan"), dtype=torch.float16, device="cuda")
    bwd = (ptr(grad_image), ptr(grad_ws), ptr(case["h"]), ptr(case["c"]), 4, ptr(case["deltas"]), ptr(case["rays"]), ptr(case["counter"]), ptr(ws), ptr(raw), M, N,
           1e-4, 1.0, None, 1.0, ptr(grad_c), ptr(grad_h0))
    if grad_sumsq is not None:
        check(lib.foc_occ_tail_backward_sumsq(*bwd, ptr(grad_sumsq), st), "occ_tail_backward_sumsq")
    else:
        check(lib.foc_occ_tail_backward(*bwd, st), "occ_tail_backward")
    torch.cuda.synchronize()
    return dict(ws=ws.clone(), depth=depth.clone(), image=image.clone(), grad_c=grad_c, grad_h0=grad_h0)


def test_criterion_kernels_against_float64():
    """ray_sumsq against float64 (rtol 1e-5: an fp32 sum of at most 1024 terms of relative error ~1e-7 each) and the criterion's gradient
    on h[:,0] against autograd of the float64 expression sqrt(sum over outside rays of sum over ALL their samples of exp(h0)^2), times
    trunc_exp's factor exp(clamp(h0, -15, 15)) / exp(h0) where the clamp acts. The kernel forms the value in fp32 and rounds it to fp16 once:
    it may land one fp16 step from the rounded float64 value where that lies at a rounding boundary, so the bound is one fp16 ulp
    (2^-10 relative) of the value; where the compositing gradient joins it, the plain kernel's own fp16 rounding adds half an ulp."""
    case = _ragged_case()
    N, M, budget = case["N"], case["budget"], case["budget"]
    rays = case["rays"].tolist()
    g = torch.Generator().manual_seed(9)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.randperm(N, generator=g)[: N // 2]] = True                # True: inside the object mask
    mask[case["order"][0]] = False                                       # a dense ray outside the mask, one inside
    mask[case["order"][5]] = True
    outside = (~mask).cuda()

    # ---- float64 reference, from rays, h[:,0] and the mask
    h0 = case["h"][:budget, 0].double().detach().requires_grad_(True)
    sigma = torch.exp(h0)
    ref_sumsq = torch.zeros(N, dtype=torch.float64, device="cuda")
    row_ray = torch.full((budget,), -1, dtype=torch.long)
    stopped_after = {}
    for n, (index, first, count) in enumerate(rays):
        if count == 0 or first + count > budget:
            continue
        ref_sumsq[index] = ref_sumsq[index] + (sigma[first: first + count] ** 2).sum()
        row_ray[first: first + count] = index
        T = torch.cumprod(torch.exp(-sigma[first: first + count].detach() * 0.02), 0)
        below = torch.nonzero(T < 1e-4)
        if below.numel() and int(below[0]) < count - 1:
            stopped_after[n] = int(below[0])
    assert stopped_after, "no ray of the case ends early"
    assert any(first + count > budget for _, first, count in rays), "no ray of the case overflows the budget"
    assert any(mask[rays[n][0]] for n in stopped_after) and any(not mask[rays[n][0]] for n in stopped_after)
    crit = torch.sqrt((ref_sumsq * outside.double()).sum())
    # the loss hands the criterion the gradient g = 2e-3 crit, so that fixedstep._masked_norm's gradient of ray_sumsq, g / (2 crit), is 1e-3
    # on every ray outside the mask: the per-row values then lie inside fp16's range for densities from e^-6 to e^7
    (crit * (2e-3 * crit.detach())).backward()
    x = h0.detach()
    ref_grad = h0.grad * torch.exp(x.clamp(-15, 15)) / torch.exp(x)       # trunc_exp's backward (activation.py) in place of exp's
    coef = (outside.double() * 1e-3).float().contiguous()

    # ---- forward
    sumsq = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
    zero_img = torch.zeros(N, 3, device="cuda")
    only = _tail(case, budget, sumsq, zero_img, None, coef)
    plain0 = _tail(case, budget, None, zero_img, None, None)
    assert torch.allclose(sumsq.double(), ref_sumsq.detach(), rtol=1e-5, atol=0), (sumsq, ref_sumsq)
    for n, (index, first, count) in enumerate(rays):
        if count == 0 or first + count > budget:
            assert float(sumsq[index]) == 0.0
    for k in ("ws", "depth", "image"):
        assert torch.equal(only[k], plain0[k]), k                        # everything else: the bits of the plain kernels

    # ---- backward, criterion alone (a zero image gradient: the compositing terms vanish exactly)
    got = only["grad_h0"].double()
    assert bool(torch.isfinite(got).all()) and not plain0["grad_h0"].any() and not only["grad_c"].any()
    ref16 = ref_grad.half().double()
    err = (got[:budget] - ref16).abs()
    bound = FP16_EPS * ref16.abs() + 2.0 ** -24                           # one fp16 step of the value (the smallest subnormal below that)
    assert bool((err <= bound).all()), f"criterion gradient: worst {float((err - bound).max()):.3e} over the bound at row {int((err - bound).argmax())}"
    inside_rows = torch.tensor([r >= 0 and bool(mask[r]) for r in row_ray.tolist()]).cuda()
    outside_rows = torch.tensor([r >= 0 and not bool(mask[r]) for r in row_ray.tolist()]).cuda()
    assert not got[:budget][inside_rows].any() and float((got[:budget][outside_rows] != 0).double().mean()) > 0.9
    assert not got[:budget][(row_ray < 0).cuda()].any() and not got[budget:].any()      # the ray that does not fit, the rows behind the list
    behind = torch.zeros(budget, dtype=torch.bool)
    for n, k in stopped_after.items():
        behind[rays[n][1] + k + 1: rays[n][1] + rays[n][2]] = True
    behind = behind.cuda()
    assert float(got[:budget][behind & outside_rows].abs().min()) > 0    # rows behind an early stop of a ray outside the mask: the criterion alone

    # ---- backward with a compositing gradient as well
    g_img = torch.randn(N, 3, generator=g).cuda()
    g_ws = (torch.randn(N, generator=g) * 0.1).cuda()
    both = _tail(case, budget, torch.empty(N, device="cuda"), g_img, g_ws, coef)
    plain = _tail(case, budget, None, g_img, g_ws, None)
    assert torch.equal(both["grad_c"], plain["grad_c"])
    gb, gp = both["grad_h0"].double()[:budget], plain["grad_h0"].double()[:budget]
    assert torch.equal(gb[inside_rows], gp[inside_rows]) and float(gp[inside_rows & ~behind].abs().max()) > 0      # inside the mask: the compositing gradient alone
    assert not gb[inside_rows & behind].any() and not gp[behind].any()                                           # ... and zero behind an early stop
    err = (gb[behind & outside_rows] - ref16[behind & outside_rows]).abs()
    assert bool((err <= FP16_EPS * ref16[behind & outside_rows].abs() + 2.0 ** -24).all())
    want = gp + ref_grad
    err = (gb - want).abs()[outside_rows]
    bound = (FP16_EPS * want.abs() + 0.5 * FP16_EPS * gp.abs() + 2.0 ** -23)[outside_rows]
    assert bool((err <= bound).all()), f"compositing + criterion: worst {float((err - bound).max()):.3e} over the bound"


# ---------------------------------------------------------------- 5. one call against call by call
@pytest.mark.parametrize("case", ["budget", "budget_overflow", "per_ray_bg", "grey_bg_scaled"])
@pytest.mark.parametrize("mode", ["default", "deterministic"])
@pytest.mark.parametrize("kind", KINDS)
def test_object_node_as_one_library_call_equals_the_call_by_call_node(kind, mode, case, monkeypatch):
    """tests/test_gpu_occtrain.py::test_node_as_one_library_call_equals_the_call_by_call_node for the object node: the same kernels on the
    same buffers in the same order — outputs, the criterion and every gradient bit for bit. The table's gradient is compared in
    deterministic mode only: with gradients in fp16's normal range (LOSS_SCALE) the chunks of a multi-chunk slot of the binned grid backward
    meet through fp16 atomics in arrival order, so in the default mode even one route does not repeat its own table
    gradient to the bit. Everything else — outputs, criterion, both blobs, the feature, the encoder — meets no atomic and is pinned in the
    default mode as well, where the one call binds `precounted` itself."""
    import contextlib
    import focnerf_amd
    with focnerf_amd.deterministic() if mode == "deterministic" else contextlib.nullcontext():
        _one_call_against_call_by_call(kind, case, monkeypatch, skip=() if mode == "deterministic" else ("embeddings",))


def _one_call_against_call_by_call(kind, case, monkeypatch, skip):
    bound, n = 2, 1500
    m = _model(kind, density_scale=2 if case == "grey_bg_scaled" else 1)
    o, d = _rays(bound, n, 3)
    yolo = _yolo(n, 12)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        m.render(o, d, perturb=False, force_all_rays=True, **RENDER)            # fills step_counter
    total = int(m.step_counter[(m.local_step - 1) % 16, 0])
    m.mean_count = total // 2 if case == "budget_overflow" else total + 500
    kw = dict(perturb=True, force_all_rays=False, bg_color={"per_ray_bg": torch.rand(n, 3, device="cuda"), "grey_bg_scaled": 0.25}.get(case))
    names = ["foc_occ_train_forward_obj", "foc_occ_train_backward_obj", "foc_occ_train_forward", "foc_occ_train_backward"]

    calls = _count_calls(monkeypatch, names)

    def step(native, seed):
        before = dict(calls)
        monkeypatch.setenv("FOC_OCC_NATIVE_NODE", "1" if native else "0")
        out, grads = _step(m, o, d, yolo, monkeypatch, True, seed=seed, **kw)
        return out, grads, {k: calls[k] - before[k] for k in calls}
    ref, g_ref, made = step(False, 7)
    assert not any(made.values()), made
    got, g_got, made = step(True, 7)
    assert made == {"foc_occ_train_forward_obj": 1, "foc_occ_train_backward_obj": 1, "foc_occ_train_forward": 0, "foc_occ_train_backward": 0}
    for k in ("image", "depth", "weights_sum", "criterion_outside_mask"):
        assert _same_bits(ref[k].reshape(-1), got[k].reshape(-1)), f"{case}: {k} differs"
    assert to_np(got["weights_sum"]).max() > 0.5
    for name in g_ref:
        if name in skip:
            continue
        assert torch.equal(g_ref[name], g_got[name]), f"{case}: grad {name} differs by {float((g_ref[name].double() - g_got[name].double()).abs().max())}"
        assert float(g_ref[name].abs().max()) > 0, name
    ref2, g_ref2, _ = step(False, 8)                                     # a second step reuses the workspaces and spends a fresh ticket
    got2, g_got2, _ = step(True, 8)
    assert torch.equal(ref2["image"], got2["image"]) and all(torch.equal(g_ref2[k], g_got2[k]) for k in g_ref2 if k not in skip)
    assert not torch.equal(got["image"], got2["image"])


# ---------------------------------------------------------------- 6. inference
@pytest.mark.parametrize("kind", KINDS)
def test_native_inference_loop_equals_the_python_loop(kind, monkeypatch):
    """As tests/test_gpu_network.py for the plain network: the same image and depth bit for bit, on views from outside the box (its one-ulp
    caveat concerns cameras inside the box with fewer than half of the rays alive; that test, too, pins bits on such views and states the
    caveat for the rest)."""
    from focnerf_amd import synthetic
    from focnerf_amd.field import field_plan
    bound = 2
    m = _model(kind, bound, seed=3).eval()
    o, d = synthetic.make_view_rays(48, 48, bound, 1, seed=2, device="cuda")
    yolo = _yolo(o.shape[1], 4)
    kw = dict(staged=False, perturb=False, dt_gamma=1 / 128, max_steps=1024, bg_color=1.0, T_thresh=1e-4)
    calls = _count_calls(monkeypatch, ["foc_occ_render_step", "foc_occ_render_step_pad"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert field_plan(m).native_loop_object and not field_plan(m).native_loop
        b = m.render(o, d, yolo, device_compaction=False, **kw)           # the reference's loop
        assert not any(calls.values())
        dflt = m.render(o, d, yolo, **kw)                                 # default: the native loop
        c = m.render(o, d, yolo, device_compaction=True, **kw)
        reached = dict(calls)
        monkeypatch.setenv("FOC_RENDER_NATIVE", "0")
        e = m.render(o, d, yolo, device_compaction=True, **kw)            # Python loop, late count
        assert dict(calls) == reached
        monkeypatch.delenv("FOC_RENDER_NATIVE")
        zero = m.render(o, d, **kw)                                       # no yolo_details: the Python loop with a zero feature, as ever
        assert dict(calls) == reached
        for max_steps, thresh in ((100, 1e-4), (1024, 0.3)):
            kw2 = dict(kw, max_steps=max_steps, T_thresh=thresh)
            p, q = m.render(o, d, yolo, device_compaction=False, **kw2), m.render(o, d, yolo, device_compaction=True, **kw2)
            assert torch.equal(p["image"], q["image"]) and torch.equal(p["depth"], q["depth"]), (max_steps, thresh)
    step = "foc_occ_render_step_pad" if kind == "tcnn" else "foc_occ_render_step"
    assert reached[step] >= 2 and sum(reached.values()) == reached[step], reached
    for other in (dflt, c, e):
        assert torch.equal(b["image"], other["image"]) and torch.equal(b["depth"], other["depth"])
    assert (b["image"] < 0.99).any(), "the view should hit the object"
    assert not torch.equal(zero["image"], b["image"])


def test_tcnn_forward_with_an_encoded_feature_agrees_with_the_torch_colour_path(monkeypatch):
    """network_tcnn.NeRFNetwork.forward under no_grad and autocast with an encoded feature runs the whole-field kernel (so that the two
    inference loops evaluate the same thing), on a cuda_ray=False model too. Against what that call evaluated before, network_foc's forward
    with the torch colour path: the density within 16 fp16 steps of its value, rgb (<= 1) within 16 FP16_EPS — the bound of the project's
    other fused-against-torch comparisons (tests/test_gpu_network_tcnn_layout.py)."""
    from focnerf_amd import network_foc, network_tcnn
    torch.manual_seed(5)
    m = network_tcnn.NeRFNetwork(bound=1, cuda_ray=False).cuda().eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    m.color_net.weights.data.mul_(1.5)
    x = torch.rand(1000, 3, device="cuda") * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(1000, 3, device="cuda"), dim=-1)
    yolo = (None, None, torch.randn(16, device="cuda") * 0.8)
    calls = _count_calls(monkeypatch, ["foc_nerf_field_inference_pad"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        sigma, rgb = m(x, d, yolo)
        assert calls["foc_nerf_field_inference_pad"] == 1, calls
        sigma_ref, rgb_ref = network_foc.NeRFNetwork.forward(m, x, d, yolo)
        assert calls["foc_nerf_field_inference_pad"] == 1, calls      # the torch colour path
    sigma, rgb, sigma_ref, rgb_ref = sigma.float().reshape(-1), rgb.float().reshape(-1, 3), sigma_ref.float().reshape(-1), rgb_ref.float().reshape(-1, 3)
    assert float(rgb_ref.std()) > 1e-2 and float(sigma_ref.max()) > 0
    assert float(((sigma - sigma_ref).abs() - 16 * FP16_EPS * sigma_ref.abs()).max()) <= 1e-6, float((sigma - sigma_ref).abs().max())
    assert float((rgb - rgb_ref).abs().max()) <= 16 * FP16_EPS, float((rgb - rgb_ref).abs().max())


# ---------------------------------------------------------------- 7. determinism and graph replay
N_OPT_STEPS = 8


def _adam(model, **kw):
    return torch.optim.Adam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True, **kw)


def _batches(n, seed):
    import bench
    dev = torch.device("cuda", 0)
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    return [bench.sample_batch(poses, intr, dev, gen) for _ in range(n)]


def _object_step(m, opt, scaler, yolo, o, d, t):
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(o, d, yolo, staged=False, perturb=True, force_all_rays=False, dt_gamma=1 / 128, max_steps=1024, bg_color=None)
        loss = torch.nn.functional.mse_loss(out["image"], t) + 1e-8 * out["criterion_outside_mask"]
    opt.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    return loss


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kind", KINDS)
def test_object_steps_repeat_bit_for_bit_in_deterministic_mode(kind):
    """tests/test_gpu_deterministic.py::test_whole_steps_repeat_bit_for_bit for the object node: eight optimizer steps twice from one seed,
    the occupancy grid updated after steps 2 and 5 (before the first update the list is unbudgeted: the call-by-call route; after it the
    one-call node) — every parameter, every loss and the occupancy state agree."""
    import bench
    import focnerf_amd

    def run():
        torch.manual_seed(0)
        m = _model(kind, seed=0)
        yolo = bench.foc_yolo_details(torch.device("cuda", 0), bench.NUM_RAYS, 7)
        opt, scaler = _adam(m), torch.amp.GradScaler("cuda")
        torch.manual_seed(1234)
        losses = []
        for i, (o, d, t) in enumerate(_batches(N_OPT_STEPS, 4)):
            losses.append(_object_step(m, opt, scaler, yolo, o, d, t).detach().clone())
            if i in (2, 5):
                if i == 5:
                    m.iter_density = 16
                with torch.autocast("cuda", dtype=torch.float16):
                    m.update_extra_state()
        torch.cuda.synchronize()
        extra = {"density_grid": m.density_grid.clone(), "density_bitfield": m.density_bitfield.clone(), "step_counter": m.step_counter.clone(),
                 "mean_count": torch.tensor(int(m.mean_count))}
        return {k: v.detach().clone() for k, v in m.state_dict().items()}, losses, extra
    with focnerf_amd.deterministic():
        (p0, l0, e0), (p1, l1, e1) = run(), run()
    assert len(l0) == N_OPT_STEPS and all(bool(torch.isfinite(v)) for v in l0), [float(v) for v in l0]
    assert int(e0["mean_count"]) > 0                                     # the later steps were budgeted
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert _same(a, b), f"loss of step {i}: {float(a)!r} vs {float(b)!r}"
    moved = [k for k in p0 if k.startswith("yolo_feat_encoder")]
    assert moved
    for k in p0:
        assert torch.equal(p0[k], p1[k]) if not p0[k].is_floating_point() else _same(p0[k], p1[k]), k
    for k in e0:
        assert torch.equal(e0[k], e1[k]), k


@pytest.mark.parametrize("kind", KINDS)
def test_object_step_graph_replay_gives_the_eager_parameters(kind):
    """tests/test_gpu_deterministic.py::test_graph_replay_gives_the_eager_parameters for the budgeted object step: no host synchronisation,
    so it captures; two replays equal eager steps four and five from the same state (GraphedStep warms up with three eager steps)."""
    import bench
    import focnerf_amd
    from focnerf_amd.graph import GraphedStep
    dev = torch.device("cuda", 0)
    batch = _batches(1, 9)[0]
    yolo = bench.foc_yolo_details(dev, bench.NUM_RAYS, 7)

    def make():
        torch.manual_seed(0)
        m = _model(kind, seed=0)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            m.render(batch[0], batch[1], perturb=False, force_all_rays=True, **RENDER)
        m.mean_count = int(m.step_counter[(m.local_step - 1) % 16, 0]) + 4096
        m.local_step = 0
        opt, scaler = _adam(m, capturable=True), torch.amp.GradScaler("cuda")
        torch.manual_seed(4321)
        return m, (lambda o, d, t: _object_step(m, opt, scaler, yolo, o, d, t))

    def params(m):
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    with focnerf_amd.deterministic():
        m, step = make()
        eager = []
        for i in range(5):
            step(*batch)
            if i >= 3:
                eager.append(params(m))
        m, step = make()
        g = GraphedStep(step, batch)
        for want in eager:
            g(*batch)
            got = params(m)
            for k in want:
                if k == "step_counter":       # bookkeeping, not the step's result: eager steps walk the 16 slots, a replay rewrites the slot it captured
                    continue
                assert torch.equal(want[k], got[k]) if not want[k].is_floating_point() else _same(want[k], got[k]), k
    key = next(k for k in eager[0] if k.startswith("yolo_feat_encoder"))
    assert not _same(eager[0][key], eager[1][key])


# ---------------------------------------------------------------- 8. training end to end
@pytest.mark.parametrize("kind", KINDS)
def test_training_with_an_object_on_the_occupancy_grid_and_checkpoints(kind, tmp_path, monkeypatch):
    """The scene and schedule of tests/test_gpu_network_tcnn_legacy.py::test_training_on_the_occupancy_grid_and_checkpoints with a fixed
    object feature, a mask over half the rays and the trainer's loss (+ 1e-8 criterion); then a checkpoint saved after rendering on the op
    route, loaded into a fresh network and rendered on the fused route."""
    from focnerf_amd import synthetic
    from focnerf_amd.checkpoint import load_checkpoint, save_checkpoint
    torch.manual_seed(0)
    bound = 1
    net = _cls(kind)(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05).cuda().train()
    o, d = synthetic.make_view_rays(48, 48, bound, 1, seed=1, device="cuda")
    n = o.shape[1]
    mask = torch.zeros(1, n, dtype=torch.bool, device="cuda")
    mask[:, ::2] = True
    yolo = (mask, None, torch.randn(144, generator=torch.Generator().manual_seed(3)).cuda())
    target = (0.5 + 0.4 * torch.sin(3 * d)).float()
    opt = torch.optim.Adam(net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    losses, crits = [], []
    for it in range(300):
        if it % 16 == 0:
            with torch.autocast("cuda", dtype=torch.float16):
                net.update_extra_state()
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.render(o, d, yolo, perturb=True, bg_color=1.0, **RENDER)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target) + 1e-8 * out["criterion_outside_mask"]
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
        crits.append(float(out["criterion_outside_mask"].detach()))
    assert all(math.isfinite(v) for v in losses + crits) and all(torch.isfinite(p).all() for p in net.parameters())
    assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:10]), f"loss {np.mean(losses[:10]):.4g} -> {np.mean(losses[-10:]):.4g}"

    ro, rd = synthetic.make_view_rays(40, 40, bound, 1, seed=2, device="cuda")
    yolo_view = (None, None, yolo[2])
    kw = dict(perturb=False, bg_color=1.0, **RENDER)
    net.eval()
    monkeypatch.setenv("FOC_RENDER_NATIVE", "0")
    monkeypatch.setenv("FOC_FUSED_OCC", "0")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        b = net.render(ro, rd, yolo_view, device_compaction=False, **kw)["image"].float()         # the op route
    path = str(tmp_path / "object_ops.pth")
    save_checkpoint(net, path)
    monkeypatch.delenv("FOC_RENDER_NATIVE")
    monkeypatch.delenv("FOC_FUSED_OCC")
    other = _cls(kind)(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05).cuda()
    assert load_checkpoint(other, path) == ([], [])
    assert torch.equal(other.density_bitfield, net.density_bitfield)
    other.eval()
    calls = _count_calls(monkeypatch, ["foc_occ_render_step", "foc_occ_render_step_pad"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = other.render(ro, rd, yolo_view, **kw)["image"].float()                                # the fused route: the native loop
    assert sum(calls.values()) >= 1, calls
    assert float(b.std()) > 1e-2
    assert float((a - b).abs().max()) <= 16 * FP16_EPS, f"checkpoint render: max |fused - ops| = {float((a - b).abs().max()):.3g}"
    # and one training forward of the loaded network on both routes
    other.train()
    imgs = {}
    for fused in (False, True):
        monkeypatch.setenv("FOC_FUSED_OCC", "1" if fused else "0")
        with torch.autocast("cuda", dtype=torch.float16):
            imgs[fused] = other.render(ro, rd, (mask[:, :ro.shape[1]], None, yolo[2]), force_all_rays=True, **kw)["image"].detach().float()
    assert float((imgs[True] - imgs[False]).abs().max()) <= 16 * FP16_EPS
