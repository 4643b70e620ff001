"""Float64 reference of the occupancy-grid path's compositing on ragged sample lists, and the per-element magnitudes its tolerances need:
the training composite (raymarching.cu:500-693: k_composite_train_fwd / _bwd), its tail form (legacy/nerf/renderer.py:256-322: k_occ_tail_*)
and the inference burst (raymarching.cu:818-905: k_composite_rays, k_composite_rays_pre).

`train()` pads the rays of a list rays [N,3] = (output row, offset, count) to [N, Tmax] with a validity mask and writes the operation as
plain CPU torch float64 expressions; autograd produces the backward (`train_backward()`):

    alpha_i = 1 - exp(-sigma_i dt0_i)      T_after_i = prod_{j<=i} (1 - alpha_j)      w_i = alpha_i T_after_{i-1}      t_i = sum_{j<=i} dt1_j
    weights_sum, depth, image = sum_{i<=stop} (w_i, w_i t_i, w_i rgb_i)
    tail form: sigma = density_scale * trunc_exp(h0), rgb = half(sigmoid(c)), image = raw + (1 - weights_sum) bg,
               depth = clamp(depth - near, 0) / (far - near) (no gradient), ray_sumsq = sum over ALL the ray's samples of exp(h0)^2

A ray with count == 0 or offset + count > M gives zeros (tail form: the background, depth 0, sumsq 0) and takes no gradient; rays[:, 0], a
permutation, decides the output row. h0 and c are fp16 values, deltas / nears / fars fp32 values; only the half rounding of sigmoid(c)
stays as a rounding point (fixed_tail_ref.py: _HalfSigmoid, clear_of_half_midpoints).

`stop` — the first sample with T_after < T_thresh, or the ray's last sample — is an ARGUMENT: a discontinuous decision that fp32 may
take one sample earlier or later when T_after lies within rounding of the threshold. `stop_candidates()` lists, per ray, the stops float64
cannot exclude: a sample is undecided when |T_after_i - T_thresh| <= bound(T_after_i); T_after never increases, so the candidates are the
undecided samples from the first one on plus the first sample clearly below the threshold (the last sample if there is none). A ray with
one candidate is decided. A caller compares all of a ray's outputs with the reference at ONE candidate.

`burst()` is the inference recurrence, per listed ray (entries < 0 skipped), from the given accumulators: per slot stop if dt0 == 0;
T = 1 - weights_sum; w = alpha T; accumulate w, w t (after t += dt1), w rgb; stop after the accumulation if T < T_thresh. What was
accumulated and whether the ray died are arguments (`n_acc`, `died`: `burst_stops()` / `burst_candidates()`); a ray that died keeps its
rays_t, a survivor writes it.

Tolerances (`train_magnitudes()`, `burst_magnitudes()`): first-order magnitudes by the rules of fixed_tail_ref.py's docstring, bound
C * 2^-24 * (T + K) * mag with T the ray's sample count (the burst: n_step). Specific to these kernels:
  * alpha uses __expf: the product a = -sigma dt0 is rounded, then a * log2(e) is rounded AGAIN before the hardware exp2, which moves the
    result by up to |a| ulps of it: exp(a) carries exp(a) (mag(a) + |a| + 1). sigma = expf(h0) and the sigmoid use expf (mag(a) + 1).
  * the backward's `final - acc` (the colour behind sample i) cancels towards the end of a ray: it carries mag(final) + mag(acc_i) +
    |final - acc_i|, the magnitudes of its terms, never a bound relative to the result.
`fast_exp()` models __expf for the fp32 evaluation (dtype=torch.float32) that test_ragged_ref.py holds to the bound.

`mutant=` names a deliberately wrong variant of one expression (MUTANTS). They exist so that test_ragged_ref.py can show that the bound
notices each of them on the fp32 CPU evaluation; a reference value is never computed with one.
"""
import numpy as np
import torch

from fixed_tail_ref import U, _HalfSigmoid, _TruncExp, clear_of_half_midpoints

C, K = 2.0, 16
TINY = 2.0 ** -126
LOG2E = np.float32(1.4426950408889634)
MUTANTS = ("T_carry", "t_carry", "colour_carry", "lane_lt_first", "stop_before_fwd", "ds_backward", "no_bg_grad", "unclamped",
           "sumsq_before_stop", "T_after_test", "dead_rays_t")


def fast_exp(a):
    """__expf: exp2(fl32(a * log2 e)) in an fp32 evaluation, exp in float64."""
    return torch.exp2(a * LOG2E) if a.dtype == torch.float32 else torch.exp(a)


# ---------------------------------------------------------------- ragged lists
def layout(rays, M):
    """rays [N,3] int (output row, offset, count) -> the padded view: fits [N], valid [N,Tmax], rows [N,Tmax] (flat row, 0 where invalid)."""
    rays = np.asarray(rays, np.int64)
    index, offset, count = rays[:, 0], rays[:, 1], rays[:, 2]
    assert np.array_equal(np.sort(index), np.arange(len(index))), "rays[:, 0] must be a permutation"
    fits = (count > 0) & (offset + count <= M)
    Tmax = max(int(count[fits].max(initial=0)), 1)
    col = np.arange(Tmax)[None, :]
    valid = fits[:, None] & (col < count[:, None])
    rows = np.where(valid, offset[:, None] + col, 0)
    return dict(index=index, offset=offset, count=count, fits=fits, valid=valid, rows=rows, Tmax=Tmax, col=col, M=int(M),
                inverse=np.argsort(index), T=np.where(fits, count, 1).astype(np.float64))


def gather(L, a):
    """Flat per-sample array [M, ...] -> padded [N, Tmax, ...], zeros where invalid."""
    a = np.asarray(a)
    g = a[L["rows"]] if a.shape[0] > 0 else np.zeros(L["rows"].shape + a.shape[1:], a.dtype)
    return np.where(L["valid"].reshape(L["valid"].shape + (1,) * (a.ndim - 1)), g, np.zeros((), a.dtype))


def by_list(L, a):
    """Per-output-row array [N, ...] -> list order."""
    return np.asarray(a)[L["index"]]


def _chunk_cumop(x, op, carry):
    """cumsum / cumprod along the last axis in chunks of 64; carry=False forgets the chunks before (a mutant)."""
    if carry:
        return op(x, -1)
    n = x.shape[-1]
    pad = (-n) % 64
    fill = torch.ones if op is torch.cumprod else torch.zeros
    xp = torch.cat([x, fill(x.shape[:-1] + (pad,), dtype=x.dtype)], -1)
    return op(xp.view(x.shape[:-1] + (-1, 64)), -1).reshape(x.shape[:-1] + (-1,))[..., :n]


def train(rays, M, deltas, stop, sigma=None, rgb=None, h0=None, c=None, density_scale=1.0, bg=None, nears=None, fars=None, T_thresh=None,
          dtype=torch.float64, mutant=None, half_rgb=True):
    """The training composite on the list (module docstring). Density as sigma [M] (fp32 values) or the logit h0 [M] (fp16 values, tail
    form); colour as rgb [M,3] or the logits c [M,3]. stop [N] (list order): the last accumulated sample of each ray; None: the natural
    stop of this evaluation (T_thresh). bg (None, a scalar or [N,3] by output row), nears, fars [N] by output row: the tail form's image
    and depth. h0 / c may also be padded torch leaves [N,Tmax(,3)] (gradcheck; half_rgb=False: sigmoid without its fp16 rounding). Returns a dict of tensors: outputs by OUTPUT row, per-sample values padded [N,Tmax] in list order (graph kept)."""
    L = layout(rays, M)
    f = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    valid = torch.from_numpy(L["valid"])
    col = torch.from_numpy(L["col"])
    deltas = np.asarray(deltas, np.float32).reshape(-1, 2)
    dt0, dt1 = f(gather(L, deltas[:, 0])), f(gather(L, deltas[:, 1]))
    out = dict(L=L, dtype=dtype, density_scale=float(density_scale), dt0=dt0, dt1=dt1, valid=valid)
    ds = float(density_scale)
    if h0 is not None:
        h0p = h0 if torch.is_tensor(h0) else f(gather(L, np.asarray(h0).astype(np.float64))).requires_grad_(True)
        e = torch.exp(h0p) if mutant == "unclamped" else _TruncExp.apply(h0p)
        sig = e if ds == 1.0 else (e + (ds - 1.0) * e.detach() if mutant == "ds_backward" else ds * e)
        out.update(h0=h0p, e=e)
    else:
        sig = f(gather(L, sigma)).requires_grad_(True)
        out["sigma_leaf"] = sig
    if c is not None:
        cp = c if torch.is_tensor(c) else f(gather(L, np.asarray(c).astype(np.float64))).requires_grad_(True)
        y = _HalfSigmoid.apply(cp) if half_rgb else torch.sigmoid(cp)
        out["c"] = cp
    else:
        y = f(gather(L, rgb)).requires_grad_(True)
        out["rgb_leaf"] = y
    a = -sig * dt0
    ex = fast_exp(a)
    alpha = torch.where(valid, 1 - ex, torch.zeros_like(ex))
    om = 1 - alpha
    Ta = _chunk_cumop(om, torch.cumprod, mutant != "T_carry")
    Tb = torch.cat([torch.ones_like(Ta[:, :1]), Ta[:, :-1]], -1)
    if mutant == "T_carry":
        Tb = torch.where(col % 64 == 0, torch.ones_like(Tb), Tb)
    t = _chunk_cumop(torch.where(valid, dt1, torch.zeros_like(dt1)), torch.cumsum, mutant != "t_carry")
    last = torch.from_numpy(np.maximum(L["count"] - 1, 0))
    if stop is None:
        stop = natural_stop(Ta.detach(), L, T_thresh)
    stop = torch.as_tensor(np.asarray(stop), dtype=torch.int64)
    act = valid & (col <= stop[:, None])
    if mutant == "lane_lt_first":                                   # drops the sample that crossed the threshold (first = 64 when none did)
        crossed = Ta.detach().gather(1, stop[:, None].clamp(max=L["Tmax"] - 1))[:, 0] < T_thresh
        act = valid & torch.where(crossed[:, None], col < stop[:, None], col <= stop[:, None])
    w = torch.where(act, alpha * Tb, torch.zeros_like(alpha))
    wy = w[..., None] * y
    ws, depth, raw = w.sum(-1), (w * t).sum(-1), wy.sum(-2)
    if mutant == "colour_carry":                                    # the backward's running colour restarts at every chunk: gradient only
        before = (torch.cumsum(wy, -2) - wy).detach()
        carry = before[:, (L["col"][0] // 64) * 64, :]
        raw = raw - (torch.where(act, (sig - sig.detach()) * dt0, torch.zeros_like(sig))[..., None] * carry).sum(-2)
    inv = torch.from_numpy(L["inverse"])
    out.update(sigma=sig, rgb=y, a=a, ex=ex, alpha=alpha, om=om, T_after=Ta, T_before=Tb, t=t, act=act, stop=stop, weights=w,
               weights_sum=ws[inv], depth_raw=depth[inv], image_raw=raw[inv], last=last)
    if bg is None:
        out.update(image=out["image_raw"], depth=out["depth_raw"])
        return out
    bgv = f(np.array(np.broadcast_to(np.asarray(bg, np.float64).reshape(-1, 1) if np.ndim(bg) == 0 else np.asarray(bg), (len(L["index"]), 3))))
    near, far = f(nears), f(fars)
    rest = 1 - (out["weights_sum"].detach() if mutant == "no_bg_grad" else out["weights_sum"])
    out["image"] = out["image_raw"] + rest[:, None] * bgv
    out["depth"] = (out["depth_raw"].detach() - near).clamp(min=0) / (far - near)
    if h0 is not None:
        e2 = torch.where(valid, e * e, torch.zeros_like(e))
        if mutant == "sumsq_before_stop":
            e2 = torch.where(act, e2, e2.detach())
        out["sumsq"] = e2.sum(-1)[inv]
    out.update(bg=bgv, near=near, far=far)
    return out


def natural_stop(T_after, L, T_thresh):
    """[N]: the first valid sample with T_after < T_thresh, or the ray's last sample."""
    below = (T_after < T_thresh) & torch.from_numpy(L["valid"])
    first = torch.where(below.any(-1), below.to(torch.int64).argmax(-1), torch.from_numpy(np.maximum(L["count"] - 1, 0)))
    return first


def train_backward(fwd, grad_image, grad_ws=None, grad_sumsq=None):
    """Gradients of sum(grad_image * image) + sum(grad_ws * weights_sum) + sum(grad_sumsq * sumsq) (by output row; None: absent) with
    respect to the leaves, padded [N,Tmax(,3)] in list order: grad_sigma / grad_rgb (composite form) or grad_h0 / grad_c (tail form)."""
    f = lambda a: torch.as_tensor(np.asarray(a)).to(fwd["dtype"])
    outs, gouts = [fwd["image"]], [f(grad_image)]
    if grad_ws is not None:
        outs.append(fwd["weights_sum"]); gouts.append(f(grad_ws))
    if grad_sumsq is not None:
        outs.append(fwd["sumsq"]); gouts.append(f(grad_sumsq))
    names = [(k, n) for k, n in (("sigma_leaf", "grad_sigma"), ("rgb_leaf", "grad_rgb"), ("h0", "grad_h0"), ("c", "grad_c")) if k in fwd]
    grads = torch.autograd.grad(outs, [fwd[k] for k, _ in names], gouts, retain_graph=True, allow_unused=True)
    return {n: (g if g is not None else torch.zeros_like(fwd[k])) for (k, n), g in zip(names, grads)}


def _scan_mag(Tb_first_mag, om, m_om, Ta):
    """mag(T_after_i) = mag(T_after_{i-1}) om_i + T_after_{i-1} mag(om_i) + T_after_i."""
    m = torch.zeros_like(Ta)
    prev_m, prev_T = Tb_first_mag, torch.ones_like(Ta[:, 0])
    for i in range(Ta.shape[1]):
        m[:, i] = prev_m * om[:, i] + prev_T * m_om[:, i] + Ta[:, i]
        prev_m, prev_T = m[:, i], Ta[:, i]
    return m


def _prefix(x):
    return torch.cumsum(x, 1)


def train_magnitudes(fwd, grad_image=None, grad_ws=None, grad_sumsq=None):
    """Per-element first-order magnitudes (module docstring) of train()'s outputs (by output row) and, with grad_image, of
    train_backward()'s gradients (padded, list order). T_after's are returned padded too (stop_candidates)."""
    with torch.no_grad():
        L = fwd["L"]
        f = lambda a: torch.as_tensor(np.asarray(a)).to(torch.float64)
        d = lambda k: fwd[k].detach().to(torch.float64)
        sig, y, a, ex, alpha, om, Ta, Tb, t, w = (d(k) for k in ("sigma", "rgb", "a", "ex", "alpha", "om", "T_after", "T_before", "t", "weights"))
        dt0, dt1, valid, act = fwd["dt0"].to(torch.float64), fwd["dt1"].to(torch.float64), fwd["valid"], fwd["act"]
        ds = fwd["density_scale"]
        z = torch.zeros_like(sig)
        if "h0" in fwd:
            e = d("e")
            m_e = e.clone()                                             # expf
            m_sig = m_e if ds == 1.0 else ds * m_e + sig.abs()
        else:
            e, m_e, m_sig = None, None, z
        m_a = m_sig * dt0.abs() + a.abs()
        m_ex = ex * (m_a + a.abs() + 1)                                 # __expf
        m_alpha = torch.where(valid, m_ex + alpha.abs(), z)
        m_om = torch.where(valid, m_alpha + om.abs(), z)
        m_Ta = _scan_mag(torch.zeros_like(Ta[:, 0]), om, m_om, Ta)
        m_Tb = torch.cat([torch.zeros_like(m_Ta[:, :1]), m_Ta[:, :-1]], -1)
        m_w = torch.where(act, m_alpha * Tb + alpha.abs() * m_Tb + w.abs(), z)
        m_t = _prefix(torch.where(valid, dt1.abs(), z))
        m_ws = m_w.sum(-1) + w.abs().sum(-1)
        wt = w * t
        m_depth = (m_w * t.abs() + w.abs() * m_t + 2 * wt.abs()).sum(-1)
        wy = w[..., None] * y
        m_wy = m_w[..., None] * y.abs() + wy.abs()
        m_raw = (m_wy + wy.abs()).sum(-2)
        inv = torch.from_numpy(L["inverse"])
        out = dict(T_after=m_Ta, weights=m_w, weights_sum=m_ws[inv], depth_raw=m_depth[inv], image_raw=m_raw[inv])
        ws_l, raw_l = w.sum(-1), wy.sum(-2)
        rest = 1 - ws_l
        m_rest = m_ws + rest.abs()
        tail = "bg" in fwd
        if tail:
            idx = torch.from_numpy(L["index"])
            bg, near, far = fwd["bg"][idx].to(torch.float64), fwd["near"][idx].to(torch.float64), fwd["far"][idx].to(torch.float64)
            img = raw_l + rest[:, None] * bg
            m_img = m_raw + m_rest[:, None] * bg.abs() + (rest[:, None] * bg).abs() + img.abs()
            dd = wt.sum(-1) - near
            m_dd = m_depth + dd.abs()
            den = far - near
            q = dd.clamp(min=0) / den
            m_dn = m_dd / den.abs() + dd.clamp(min=0) * den.abs() / (den * den) + q.abs()
            out.update(image=m_img[inv], depth=m_dn[inv])
            if e is not None:
                out["sumsq"] = torch.where(valid, 4 * e * e, z).sum(-1)[inv]
        else:
            out.update(image=out["image_raw"], depth=out["depth_raw"])
        if grad_image is None:
            return out
        idx = torch.from_numpy(L["index"])
        g = f(grad_image)[idx]                                          # list order
        gws = f(grad_ws)[idx] if grad_ws is not None else torch.zeros_like(ws_l)
        m_gws = torch.zeros_like(gws)
        if tail:                                                        # image = raw + (1 - ws) bg: the opacity's gradient takes -(g . bg)
            gb = (g * bg).sum(-1)
            m_gws = 2 * (g * bg).abs().sum(-1) + gws.abs() + (gws - gb).abs()
            gws = gws - gb
        # grad_sigma = dt0 (sum_c g_c (T_after rgb_c - (final_c - acc_c)) + gws (1 - ws))
        acc = _prefix(wy)
        m_acc = _prefix(m_wy) + _prefix(wy.abs())
        diff = raw_l[:, None, :] - acc
        m_diff = m_raw[:, None, :] + m_acc + diff.abs()
        Ty = Ta[..., None] * y
        inner = Ty - diff
        m_inner = m_Ta[..., None] * y.abs() + Ty.abs() + m_diff + inner.abs()
        gin = g[:, None, :] * inner
        m_gin = g[:, None, :].abs() * m_inner + gin.abs()
        wst = gws * rest
        m_wst = m_gws * rest.abs() + gws.abs() * m_rest + wst.abs()
        tot = gin.sum(-1) + wst[:, None]
        m_tot = m_gin.sum(-1) + gin.abs().sum(-1) + m_wst[:, None] + tot.abs()
        gs = dt0 * tot
        m_gs = torch.where(act, dt0.abs() * m_tot + gs.abs(), z)
        gs = torch.where(act, gs, z)
        m_grgb = torch.where(act[..., None], g[:, None, :].abs() * m_w[..., None] + (g[:, None, :] * w[..., None]).abs(), torch.zeros_like(wy))
        if "h0" not in fwd:
            out.update(grad_sigma=m_gs, grad_rgb=m_grgb)
            return out
        if ds != 1.0:
            gs = ds * gs
            m_gs = ds * m_gs + gs.abs()
        gsq2 = 2 * f(grad_sumsq)[idx] if grad_sumsq is not None else torch.zeros_like(ws_l)
        ce = torch.where(valid, gsq2[:, None] * e, z)
        gs2 = gs + ce
        m_gs2 = m_gs + torch.where(valid, gsq2.abs()[:, None] * m_e, z) + ce.abs() + gs2.abs()
        e_lo, e_hi = float(np.exp(-15.0)), float(np.exp(15.0))
        cf = e.clamp(e_lo, e_hi)
        m_cf = torch.where((e > e_lo) & (e < e_hi), m_e, cf)
        out["grad_h0"] = torch.where(valid, m_gs2 * cf + gs2.abs() * m_cf + (gs2 * cf).abs(), z)
        yy = (y * (1 - y)).abs()
        out["grad_c"] = m_grgb * yy + 2 * (g[:, None, :] * w[..., None]).abs() * yy
        # the tail rounds grad_rgb = g w to fp16 before the sigmoid's factor (torch's half sigmoid backward): a second fp16 rounding
        # point, half an fp16 ulp of g w carried through y (1 - y). Callers add it to the half-ulp allowance of the stored value.
        out["grad_rgb_half"] = (g[:, None, :] * w[..., None]).abs()
        out["yy"] = yy
        return out


magnitudes = train_magnitudes


def stop_candidates(fwd, mags, T_thresh):
    """Per ray (list order) the stops float64 cannot exclude (module docstring), each a list of sample indices; fwd from train() with
    stop=None or any stop (T_after does not depend on it)."""
    L = fwd["L"]
    Ta = fwd["T_after"].detach().numpy()
    bound = C * U * (L["T"][:, None] + K) * np.asarray(mags["T_after"]) + (L["T"][:, None] + K) * TINY
    res = []
    for r in range(len(L["count"])):
        n = int(L["count"][r]) if L["fits"][r] else 0
        if n == 0 or T_thresh <= 0:                                   # T_after >= 0 in every evaluation: never below a threshold of 0
            res.append([max(n - 1, 0)])
            continue
        tr, b = Ta[r, :n], bound[r, :n]
        clear = np.nonzero(tr < T_thresh - b)[0]
        end = int(clear[0]) if clear.size else n - 1
        und = [int(i) for i in np.nonzero(np.abs(tr - T_thresh) <= b)[0] if i < end]
        res.append(und + [end])
    return res


def stops_of(cands, k):
    """The k-th candidate of every ray (its last one where it has fewer)."""
    return np.array([c[min(k, len(c) - 1)] for c in cands], np.int64)


# ---------------------------------------------------------------- the inference burst
def burst_stops(n_step, T_thresh, dt0, T_test):
    """(n_acc, died) from the slot tests: dt0 [n,n_step], T_test [n,n_step] the transmittance each slot's test sees."""
    n = dt0.shape[0]
    n_acc, died = np.full(n, n_step, np.int64), np.zeros(n, bool)
    for r in range(n):
        for j in range(n_step):
            if dt0[r, j] == 0:
                n_acc[r], died[r] = j, True
                break
            if T_test[r, j] < T_thresh:
                n_acc[r], died[r] = j + 1, True
                break
    return n_acc, died


def burst(n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, n_acc=None, died=None, dtype=torch.float64,
          mutant=None):
    """The inference burst (module docstring) on ray-major sample arrays [n_alive * n_step(, 3 | 2)]. n_acc / died [n_alive] (entries of
    skipped list rows ignored): how many slots each listed ray accumulates and whether it ends; None: this evaluation's own decisions.
    Returns the new rays_alive, rays_t, weights_sum, depth, image (numpy, float64 values) and T [n_alive,n_step], the transmittance each
    slot's test sees; n_acc, died."""
    alive = np.asarray(rays_alive, np.int64)
    n = alive.shape[0]
    listed = alive >= 0
    idx = np.where(listed, alive, 0)
    f = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)
    sg, dl, cl = f(sigmas).view(n, n_step), f(deltas).view(n, n_step, 2), f(rgbs).view(n, n_step, 3)
    ws, dp, im, t = f(weights_sum)[idx], f(depth)[idx], f(image)[idx], f(rays_t)[idx]
    dt0 = np.asarray(deltas, np.float32).reshape(n, n_step, 2)[:, :, 0]
    hist = dict(ws=[ws], dp=[dp], im=[im], t=[t], T=[])
    for j in range(n_step):
        alpha = 1 - fast_exp(-sg[:, j] * dl[:, j, 0])
        T = 1 - ws
        w = alpha * T
        ws = ws + w
        t = t + dl[:, j, 1]
        dp = dp + w * t
        im = im + w[:, None] * cl[:, j]
        hist["T"].append((1 - ws) if mutant == "T_after_test" else T)
        for k, v in (("ws", ws), ("dp", dp), ("im", im), ("t", t)):
            hist[k].append(v)
    Ts = torch.stack(hist["T"], 1)
    if n_acc is None:
        n_acc, died = burst_stops(n_step, T_thresh, dt0, Ts.numpy())
    sel = torch.as_tensor(np.asarray(n_acc, np.int64))
    pick = lambda k: torch.stack(hist[k], 1)[torch.arange(n), sel].to(torch.float64).numpy()
    out_ws, out_dp, out_im, out_t = (np.asarray(a, np.float64).copy() for a in (weights_sum, depth, image, rays_t))
    died = np.asarray(died, bool)
    rows = idx[listed]
    out_ws[rows], out_dp[rows], out_im[rows] = pick("ws")[listed], pick("dp")[listed], pick("im")[listed]
    keep_t = listed if mutant == "dead_rays_t" else listed & ~died
    out_t[idx[keep_t]] = pick("t")[keep_t]
    new_alive = np.where(listed & died, -1, alive)
    return dict(rays_alive=new_alive, rays_t=out_t, weights_sum=out_ws, depth=out_dp, image=out_im, T=Ts.to(torch.float64).numpy(),
                n_acc=np.asarray(n_acc, np.int64), died=died, listed=listed, index=idx)


def burst_magnitudes(n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image):
    """Magnitudes after each number of accumulated slots: dict of [n_alive, n_step + 1(, 3)] for weights_sum, depth, image, rays_t, and
    T [n_alive, n_step] for the transmittance the slot tests see. The given accumulators are exact."""
    alive = np.asarray(rays_alive, np.int64)
    n = alive.shape[0]
    idx = np.where(alive >= 0, alive, 0)
    f = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    sg, dl, cl = f(sigmas).view(n, n_step), f(deltas).view(n, n_step, 2), f(rgbs).view(n, n_step, 3)
    ws, dp, im, t = f(weights_sum)[idx], f(depth)[idx], f(image)[idx], f(rays_t)[idx]
    # each accumulator is a reduction: the magnitudes of its terms (M_*) plus the absolute values of the start value and the terms once (S_*).
    # weights_sum feeds back into its own next term, w = alpha (1 - ws): ws' = ws + alpha (1 - ws) carries mag(ws) (1 - alpha) — the two
    # occurrences of ws are the same number. The rule for independent operands, mag(ws) (1 + alpha), would double at every opaque sample.
    M_ws, M_dp, M_im = torch.zeros_like(ws), torch.zeros_like(dp), torch.zeros_like(im)
    S_ws, S_dp, S_im, S_t = ws.abs(), dp.abs(), im.abs(), t.abs()
    res = dict(weights_sum=[M_ws], depth=[M_dp], image=[M_im], rays_t=[0 * S_t], T=[])
    for j in range(n_step):
        a = -sg[:, j] * dl[:, j, 0]
        ex = torch.exp(a)
        alpha = 1 - ex
        m_alpha = ex * (2 * a.abs() + 1) + alpha.abs()
        m_ws = M_ws + (S_ws if j else 0 * S_ws)                          # the given accumulator is exact until something is added to it
        T = 1 - ws
        m_T = m_ws + T.abs()
        w = alpha * T
        m_w = m_alpha * T.abs() + alpha.abs() * m_T + w.abs()
        ws = ws + w
        M_ws, S_ws = M_ws * (1 - alpha).abs() + m_alpha * T.abs() + alpha.abs() * T.abs() + w.abs(), S_ws + w.abs()
        t = t + dl[:, j, 1]
        S_t = S_t + dl[:, j, 1].abs()
        wt = w * t
        dp = dp + wt
        M_dp, S_dp = M_dp + m_w * t.abs() + w.abs() * S_t + wt.abs(), S_dp + wt.abs()
        wc = w[:, None] * cl[:, j]
        im = im + wc
        M_im, S_im = M_im + m_w[:, None] * cl[:, j].abs() + wc.abs(), S_im + wc.abs()
        res["T"].append(m_T)
        for k, v in (("weights_sum", M_ws + S_ws), ("depth", M_dp + S_dp), ("image", M_im + S_im), ("rays_t", S_t)):
            res[k].append(v)
    return {k: torch.stack(v, 1).numpy() for k, v in res.items()}


def burst_candidates(n_step, T_thresh, deltas, T, m_T):
    """Per listed row the (n_acc, died) pairs float64 cannot exclude: the slot test T < T_thresh is undecided when |T - T_thresh| <=
    bound(T). dt0 == 0 is exact."""
    n = T.shape[0]
    dt0 = np.asarray(deltas, np.float32).reshape(n, n_step, 2)[:, :, 0]
    bound = C * U * (n_step + K) * m_T + (n_step + K) * TINY
    res = []
    for r in range(n):
        c = []
        for j in range(n_step):
            if dt0[r, j] == 0:
                c.append((j, True))
                break
            if T_thresh > 0 and abs(T[r, j] - T_thresh) <= bound[r, j]:
                c.append((j + 1, True))
                continue
            if T[r, j] < T_thresh:
                c.append((j + 1, True))
                break
        else:
            c.append((n_step, False))
        res.append(c)
    return res


def burst_args(b):
    return (b["n_step"], b["T_thresh"], b["rays_alive"], b["rays_t"], b["sigmas"], b["rgbs"], b["deltas"], b["weights_sum"], b["depth"], b["image"])


def burst_match(b, got):
    """got: rays_alive, rays_t, weights_sum, depth, image after the burst. Every listed row against the reference at each of its
    candidate decisions: the accumulators and a survivor's rays_t within the bound, the kill decision equal, a dead ray's rays_t
    untouched. Returns (per-row worst ratio at the best candidate, 0 for skipped rows; name -> worst ratio; rows with > 1 candidate)."""
    args = burst_args(b)
    n_step = b["n_step"]
    ref0 = burst(*args)
    m = burst_magnitudes(n_step, *args[2:])
    cands = burst_candidates(n_step, b["T_thresh"], b["deltas"], ref0["T"], m["T"])
    listed, idx = ref0["listed"], ref0["index"]
    n = len(cands)
    rows = np.arange(n)
    best, per = np.full(n, np.inf), {}
    for k in range(max(len(c) for c in cands)):
        pick = [c[min(k, len(c) - 1)] for c in cands]
        n_acc, died = np.array([p[0] for p in pick], np.int64), np.array([p[1] for p in pick], bool)
        ref = burst(*args, n_acc=n_acc, died=died)
        r = {name: per_ray(ratios(np.asarray(got[name])[idx], ref[name][idx], m[name][rows, n_acc], n_step)) for name in ("weights_sum", "depth", "image")}
        r["rays_t"] = ratios(np.asarray(got["rays_t"])[idx], ref["rays_t"][idx], np.where(died, 0.0, m["rays_t"][rows, n_acc]), n_step)
        r["kill"] = np.where(np.asarray(got["rays_alive"]) == ref["rays_alive"], 0.0, np.inf)
        ray = np.where(listed, np.max(np.stack(list(r.values())), 0), 0.0)
        better = ray < best
        best = np.where(better, ray, best)
        for name, v in r.items():
            per[name] = np.where(better, np.where(listed, v, 0.0), per.get(name, np.zeros(n)))
    undecided = np.array([len(c) > 1 for c in cands]) & listed
    return best, {name: float(v.max(initial=0.0)) for name, v in per.items()}, undecided


# ---------------------------------------------------------------- comparison
def ratios(got, want, mag, T, half=False, extra=None):
    """Elementwise (|got - want| - allowance) / (2^-24 (T + K) mag), allowance = (T + K) 2^-126 on fp32 values, half an fp16 ulp (+ extra)
    on fp16 ones; inf where a non-finite value sits at another place than float64's (fixed-step _check's rules: a float64 value within
    the bound of fp16's overflow may land on either side, one beyond it must give the same inf). T broadcasts against the arrays."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    mag = np.nan_to_num(np.asarray(mag, np.float64), nan=0.0, posinf=np.inf)
    T = np.asarray(T, np.float64)
    scale = U * (T + K) * mag
    if half:
        with np.errstate(over="ignore"):
            want16 = want.astype(np.float16).astype(np.float64)
        border = np.isfinite(want) & (np.abs(np.abs(want) - 65520.0) <= C * scale + 32.0)
        fin = np.isfinite(want16)
        big = np.maximum(np.abs(np.where(np.isfinite(got), got, 0)), np.abs(np.where(fin, want, 0)))
        ax = np.maximum(big, 2.0 ** -14)
        allow = 0.5 * 2.0 ** (np.floor(np.log2(ax)) - 10) + (0.0 if extra is None else extra)
    else:
        want16, border, fin = want, np.zeros(want.shape, bool), np.isfinite(want)
        allow = (T + K) * TINY + np.zeros_like(want)
    r = np.zeros(np.broadcast(got, want, scale).shape)
    both = fin & np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.maximum(np.abs(got - want) - allow, 0.0)
        rr = np.where(err > 0, err / np.where(scale > 0, scale, 0.0), 0.0)
    r = np.where(both, rr, 0.0)
    misplaced = ~((np.isfinite(got) == fin) | border)
    over = np.isfinite(want) & ~fin & ~border
    with np.errstate(invalid="ignore"):
        misplaced |= over & (got != want16)
    return np.where(misplaced, np.inf, r)


def per_ray(r):
    """Worst ratio of each ray: max over every axis but the first."""
    r = np.asarray(r)
    return r.reshape(r.shape[0], -1).max(1, initial=0.0) if r.size else np.zeros(r.shape[0])


# ---------------------------------------------------------------- the cases both test files use
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1024)


def _finish(rng, name, counts, h0, T_thresh, ds=1.0, cut=0, far_ray=False, permute=True, dt_scale=None):
    """Offsets, the list, the cut M, colour logits, deltas and incoming gradients around per-ray h0 rows."""
    N = len(counts)
    counts = np.asarray(counts, np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    total = int(counts.sum())
    if cut:                                                          # the last `cut` rays with samples do not fit
        nz = np.nonzero(counts)[0]
        first_out = nz[-cut]
        M = int(offs[first_out] + counts[first_out] - 1) if not far_ray else int(offs[nz[-1]] - 1)
        M = max(M, 1)
    else:
        M = (total + 127) // 128 * 128 if total else 128             # the list's 128-row pad behind counter[0]
    index = rng.permutation(N) if permute else np.arange(N)
    rays = np.stack([index, offs, counts], 1).astype(np.int32)
    rows = max(total, M)
    h = np.concatenate([np.asarray(x, np.float64) for x in h0] + [rng.normal(0, 1, rows - total)]).astype(np.float16)
    c = rng.normal(0, 2, (rows, 3)).astype(np.float16)
    special = rng.random((rows, 3)) < 0.15
    c[special] = rng.choice(np.array([7.0, 12.0, -12.0], np.float16), int(special.sum()))
    c = clear_of_half_midpoints(c)
    dt0 = rng.uniform(2e-3, 2e-2, rows)
    if dt_scale is not None:
        dt0 = dt0 * np.concatenate([np.full(n, s) for n, s in zip(counts, dt_scale)] + [np.ones(rows - total)])
    deltas = np.stack([dt0, dt0 * rng.uniform(0.8, 1.5, rows)], 1).astype(np.float32)
    nears = rng.uniform(0.05, 0.6, N).astype(np.float32)
    fars = (nears + rng.uniform(0.5, 2.5, N)).astype(np.float32)
    grads = dict(grad_image=rng.normal(0, 1, (N, 3)), grad_ws=rng.normal(0, 0.5, N), grad_sumsq=rng.normal(0, 1, N) * 10.0 ** rng.uniform(-10, -3, N))
    return dict(name=name, N=N, M=M, total=total, rays=rays, h0=h[:M], c=c[:M], deltas=deltas[:M], nears=nears, fars=fars,
                bg=rng.random((N, 3)).astype(np.float32), T_thresh=float(T_thresh), density_scale=float(ds), grads={k: v.astype(np.float32) for k, v in grads.items()})


def random_case(N, seed, T_thresh, ds=1.0, cut=0, far_ray=False):
    """Ray r has regime (r + seed) % 6: transparent; typical; opaque from a random sample on; at trunc_exp's clamp on short steps;
    typical with sigma = 0 samples (h0 = -inf); dense. Counts from COUNTS."""
    rng = np.random.default_rng(seed)
    counts = rng.choice(COUNTS, N)
    if N >= 5:
        counts[:len(COUNTS)] = rng.permutation(COUNTS)[:N]             # every length at the larger N
    h0, scale = [], []
    for r, n in enumerate(counts):
        reg = (r + seed) % 6
        x = rng.normal(0, 2, n)
        s = 1.0
        if reg == 0:
            x = rng.uniform(-16, -8, n)
        elif reg == 2 and n:
            p = int(rng.integers(0, n))
            x[p:] = rng.uniform(4, 16.5, n - p)
        elif reg == 3:
            x = rng.choice([14.5, -14.5, 15.0, -15.0, 15.0078125, -15.0078125, 16.5, 0.5, -1.0], n)
            s = 1e-6
        elif reg == 4:
            x[rng.random(n) < 0.3] = -np.inf
        elif reg == 5:
            x = rng.normal(3, 1, n)
        h0.append(x); scale.append(s)
    return _finish(rng, f"random[{N},{seed}]", counts, h0, T_thresh, ds=ds, cut=cut, far_ray=far_ray, dt_scale=scale)


def constructed_case(pairs, seed, T_thresh, ds=1.0):
    """Decided stops: ray (count, p) has T_after = 2 T_thresh after sample p - 1 and T_thresh / 2 after sample p (p None: transparent
    enough never to stop; with T_thresh = 0 the rays turn opaque, T_after reaches 0, and nothing stops them). sigma = ds * exp(h0)."""
    rng = np.random.default_rng(seed)
    counts, h0 = [], []
    dt = 0.01
    for n, p in pairs:
        x = rng.normal(0, 1, n)
        if T_thresh == 0 and n:
            x[n // 2:] = 14.0
        elif p is not None:
            if p > 0:
                x[:p] = np.log(-np.log(2 * T_thresh) / p / dt)
            x[p] = np.log(-np.log(0.25 if p > 0 else T_thresh / 2) / dt)
        else:
            x[:] = rng.uniform(-12, -6, n)
        counts.append(n); h0.append(x - np.log(ds))
    d = _finish(rng, f"constructed[{len(pairs)},{T_thresh:g}]", counts, h0, T_thresh, ds=ds)
    d["deltas"][:, 0] = dt
    d["stops"] = [p for _, p in pairs]
    return d


# ---------------------------------------------------------------- a case's values in the form the tests compare
BG_SCALAR = 0.7
TERMS = ("grad_image", "grad_ws", "grad_sumsq")
HALF_OUTPUTS = ("grad_h0", "grad_c")


def composite_inputs(case):
    """What the separate composite kernels are fed: sigma = fl32(density_scale exp(h0)), rgb = half(sigmoid(c)), both fp32 arrays."""
    sig = (case["density_scale"] * np.exp(case["h0"].astype(np.float64))).astype(np.float32)
    rgb = (1.0 / (1.0 + np.exp(-case["c"].astype(np.float64)))).astype(np.float16).astype(np.float32)
    return sig, rgb


def grads_of(case, on, form):
    """The incoming gradients with only the terms in `on` (grad_image absent: zeros, it is always read; the others None = NULL)."""
    g = {k: (case["grads"][k] if k in on else None) for k in TERMS}
    if g["grad_image"] is None:
        g["grad_image"] = np.zeros_like(case["grads"]["grad_image"])
    if form == "composite":
        del g["grad_sumsq"]
    return g


def combos(form):
    """One incoming gradient term at a time, then all of them together."""
    terms = TERMS if form == "tail" else TERMS[:2]
    return [(t,) for t in terms] + [terms]


def evaluate(case, form, stop, on=None, bg_ray=True, dtype=torch.float64, mutant=None, mags=False):
    """train() + train_backward() (+ train_magnitudes()) of a case as numpy float64 arrays: the outputs in LIST order, the gradients padded
    [N,Tmax(,3)]. form "composite" (k_composite_train_*) or "tail" (k_occ_tail_*); `on`: the incoming gradient terms (None: forward only).
    Returns (values, magnitudes or None, fwd)."""
    kw = dict(T_thresh=case["T_thresh"], dtype=dtype, mutant=mutant)
    if form == "composite":
        sig, rgb = composite_inputs(case)
        fwd = train(case["rays"], case["M"], case["deltas"], stop, sigma=sig, rgb=rgb, **kw)
        names = ("weights_sum", "depth", "image")
    else:
        fwd = train(case["rays"], case["M"], case["deltas"], stop, h0=case["h0"], c=case["c"], density_scale=case["density_scale"],
                    bg=case["bg"] if bg_ray else BG_SCALAR, nears=case["nears"], fars=case["fars"], **kw)
        names = ("weights_sum", "image_raw", "image", "depth", "sumsq")
    L = fwd["L"]
    vals = {k: by_list(L, fwd[k].detach().to(torch.float64).numpy()) for k in names}
    g = grads_of(case, on, form) if on is not None else {}
    if on is not None:
        vals.update({k: v.to(torch.float64).numpy() for k, v in train_backward(fwd, **g).items()})
    m = None
    if mags:
        m = {k: (by_list(L, v.numpy()) if k in names else v.numpy()) for k, v in train_magnitudes(fwd, **g).items()}
    return vals, m, fwd


def compare(got, want, mags, L, half=HALF_OUTPUTS):
    """name -> per-ray worst ratio [N] (list order) of every output in `want` that `got` has."""
    res = {}
    for k, w in want.items():
        if k not in got:
            continue
        T = L["T"].reshape((-1,) + (1,) * (w.ndim - 1))
        extra = None
        if k == "grad_c" and k in half:                              # the second fp16 rounding point (train_magnitudes)
            q = np.maximum(mags["grad_rgb_half"], 2.0 ** -14)
            extra = 0.5 * 2.0 ** (np.floor(np.log2(q)) - 10) * mags["yy"]
        res[k] = per_ray(ratios(got[k], w, mags[k], T, half=k in half, extra=extra))
    return res


def match(cands, want_fn, got, L, half=HALF_OUTPUTS):
    """Every ray against the reference at each of its candidate stops (want_fn(stops) -> (values, magnitudes)): the best candidate per
    ray. Returns (per-ray worst ratio over all outputs at that candidate, the stop chosen, name -> worst ratio over the rays)."""
    N = len(cands)
    best, chosen, per = np.full(N, np.inf), stops_of(cands, 0), {}
    for k in range(max(len(c) for c in cands)):
        stops = stops_of(cands, k)
        want, mags = want_fn(stops)
        r = compare(got, want, mags, L, half)
        ray = np.max(np.stack(list(r.values())), 0)
        better = ray < best
        best = np.where(better, ray, best)
        chosen = np.where(better, stops, chosen)
        for name, v in r.items():
            per[name] = np.where(better, v, per.get(name, np.zeros(N)))
    return best, chosen, {name: float(v.max(initial=0.0)) for name, v in per.items()}


_P37 = [(1, 0), (2, 0), (65, 0), (63, 62), (64, 63), (65, 63), (65, 64), (129, 62), (129, 63), (129, 64), (128, 127), (129, 127), (129, 128),
        (200, 127), (200, 128), (200, 199), (1024, 1023), (1024, 64), (1024, 128), (0, None), (64, None), (2, 1), (127, 126), (127, 63),
        (200, 64), (0, None), (128, 63), (128, 64), (63, 0), (1, None), (2, None), (65, None), (129, None), (1024, 63), (1024, 127), (64, 62),
        (200, None)]


# seeds of the random cases, chosen so that no ray of a case has more than one stop candidate (test_ragged_ref.py asserts the cap)
SEEDS = (1, 101, 201, 301, 404, 502, 601, 703)


def train_cases():
    """Every case of the training and tail tests (both files)."""
    return [
        random_case(1, SEEDS[0], 1e-4, ds=2.0), random_case(3, SEEDS[1], 1e-3), random_case(4, SEEDS[2], 1e-2, ds=2.0), random_case(5, SEEDS[3], 0.0),
        random_case(37, SEEDS[4], 1e-4, cut=3), random_case(37, SEEDS[5], 1e-3, ds=2.0), random_case(5, SEEDS[6], 1e-2, cut=2, far_ray=True),
        random_case(37, SEEDS[7], 1e-2, ds=2.0),
        constructed_case(_P37, 20, 1e-4, ds=2.0), constructed_case([(65, 0), (64, 63), (65, 64), (129, 128), (200, 199)], 21, 1e-2),
        constructed_case([(63, 62), (128, 63), (129, 64), (200, 127)], 22, 1e-3, ds=2.0), constructed_case([(65, None), (129, None), (1024, None)], 23, 0.0),
    ]


def burst_case(n_alive, n_step, seed, T_thresh):
    """A burst: n_rays = n_alive + 7 accumulators, the list a shuffled choice of them with -1 entries. Listed row r has regime
    (r + seed) % 8: typical from zero accumulators; typical from random ones; 1 - weights_sum = 2 T_thresh then an opaque sample;
    1 - weights_sum = T_thresh / 2; the burst ends on dt0 == 0 at slot 0; in the middle; opaque samples; transparent."""
    rng = np.random.default_rng(seed)
    n_rays = n_alive + 7
    alive = rng.permutation(n_rays)[:n_alive].astype(np.int32)
    if n_alive > 2:
        alive[rng.random(n_alive) < 0.1] = -1
    sig = np.exp(rng.normal(1.5, 1.5, (n_alive, n_step))).astype(np.float32)
    dt0 = rng.uniform(2e-3, 2e-2, (n_alive, n_step)).astype(np.float32)
    dl = np.stack([dt0, dt0 * rng.uniform(0.8, 1.5, (n_alive, n_step)).astype(np.float32)], -1)
    rgb = rng.random((n_alive, n_step, 3)).astype(np.float32)
    ws = (rng.random(n_rays) * 0.9).astype(np.float32)
    dp = (ws * rng.uniform(0.5, 2.0, n_rays)).astype(np.float32)
    im = (ws[:, None] * rng.random((n_rays, 3))).astype(np.float32)
    t = rng.uniform(0.1, 3.0, n_rays).astype(np.float32)
    for r in range(n_alive):
        i, reg = int(alive[r]), (r + seed) % 8
        if i < 0:
            continue
        if reg == 0:
            ws[i], dp[i], im[i] = 0, 0, 0
        elif reg == 2:
            ws[i] = np.float32(1 - 2 * T_thresh)
            sig[r, 0] = 3e4
        elif reg == 3:
            ws[i] = np.float32(1 - 0.5 * T_thresh)
        elif reg == 4:
            dl[r, 0, 0] = 0
        elif reg == 5:
            dl[r, n_step // 2, 0] = 0
        elif reg == 6:
            sig[r, rng.integers(0, n_step):] = 2e4
        elif reg == 7:
            sig[r] = 1e-3
    return dict(name=f"burst[{n_alive}x{n_step},{seed}]", n_alive=n_alive, n_step=n_step, n_rays=n_rays, T_thresh=float(T_thresh), rays_alive=alive,
                rays_t=t, sigmas=sig.reshape(-1), rgbs=rgb.reshape(-1, 3), deltas=dl.reshape(-1, 2), weights_sum=ws, depth=dp, image=im)


# (n_alive, n_step, form): form "aligned" (16-byte aligned arrays: the register-resident kernels at 4, 8, 16), "offset" (arrays 4 bytes
# off: the pointer-walking kernel), "compact" (foc_composite_compact on sample-major arrays)
BURSTS = [(1, 1, "aligned"), (63, 3, "aligned"), (64, 4, "aligned"), (65, 8, "aligned"), (1025, 16, "aligned"),
          (1025, 4, "offset"), (63, 8, "offset"), (64, 16, "offset"),
          (65, 3, "compact"), (1025, 4, "compact"), (1, 8, "compact"), (64, 16, "compact"), (63, 1, "compact")]
BURST_THRESH = (1e-4, 1e-3, 1e-2, 0.0)


def burst_cases():
    return [(form, burst_case(n, s, 40 + j, BURST_THRESH[j % 4])) for j, (n, s, form) in enumerate(BURSTS)]
