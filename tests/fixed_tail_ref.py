"""Float64 reference of the fixed-step compositing tail (nerf/renderer.py run(), from the density logit to image / depth), and the
per-element magnitudes its tolerances need.

`tail()` writes the operation as plain CPU torch float64 expressions and lets autograd produce the backward (`tail_backward()`):

    sigma   = trunc_exp(h0)                     (forward exp, backward exp(clamp(h0, -15, 15)))
    alpha   = 1 - exp(-delta * density_scale * sigma)
    weights = alpha * cumprod([1, 1 - alpha + 1e-15])[:-1]
    rgb     = half(sigmoid(c))                  (torch.sigmoid on a half tensor; its backward uses that fp16 y)
    image   = sum w * rgb * [w > thresh] + (1 - sum w) * bg
    depth   = sum w * clamp((z - near) / (far - near), 0, 1)
    sumsq   = sum trunc_exp(h0)^2               (the samples' share of the outside-mask criterion)

Only the quantisation that belongs to the operation stays: h0 and c are fp16 values, rgb is rounded to fp16, and the sample depths z
and the deltas are fp32 INPUTS, formed by the caller with the torch expressions of run(). Everything else is float64.

The `w > thresh` decision is an input (`mask`): the GPU tests take it from the kernel's fp32 weights after those have been checked
against this reference, so a weight within rounding of the threshold cannot make the two sides keep different colours.

The fp16 rounding of sigmoid(c) is part of the operation, but an fp32 evaluation of sigmoid lands on the other side of an fp16
rounding midpoint when the exact value lies within a few fp32 ulps of it. `clear_of_half_midpoints()` moves such logits by 1/16, so
that every fp32 evaluation of the logits a test draws rounds to the fp16 value computed here.

Tolerances (`magnitudes()`): an fp32 evaluation of the same operation differs from this reference by at most c * 2^-24 * (T + k) * mag
per element, where mag is the magnitude of the terms that meet in that element, carried through each operation to first order:
exact inputs carry 0; a sum or difference carries the magnitudes of its operands plus |result| (its own rounding); a product a * b
carries mag(a)|b| + |a|mag(b) + |ab|; a quotient a / b carries mag(a)/|b| + |a|mag(b)/b^2 + |a/b|; exp(a) carries exp(a)(mag(a) + 1).
A reduction over T samples (the transmittance scan, the composite sums, the backward's suffix sum) carries the sum of the terms'
magnitudes plus the sum of their absolute values once: its up to T - 1 partial results are each bounded by that sum, whatever the
order of association. That is where T comes from. c and k are stated with the tests that use them.

For the backward the magnitude of dL/dalpha_i is |g_i| T_i + sum_{j>i} |g_j w_j| / om_i, with the magnitudes T_i, w_j and om_i carry
from the forward, multiplied through delta * density_scale * exp(-x) and the trunc_exp factor. dL/dalpha cancels by construction on
opaque rays (torch's own cumprod backward divides the same way), so a bound relative to the result alone would flag behaviour that
belongs to the operation.
"""
import numpy as np
import torch

U = 2.0 ** -24          # fp32: half an ulp of 1


class _TruncExp(torch.autograd.Function):
    """activation.py's trunc_exp: exp(x) forward, g * exp(clamp(x, -15, 15)) backward."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * torch.exp(x.clamp(-15, 15))


class _HalfSigmoid(torch.autograd.Function):
    """torch.sigmoid on a half tensor: y = half(sigmoid(c)); backward g * y * (1 - y) with that fp16 y."""

    @staticmethod
    def forward(ctx, c):
        y = torch.sigmoid(c).to(torch.float16).to(c.dtype)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * y * (1 - y)


def clear_of_half_midpoints(c, margin_ulps=64, max_steps=8):
    """fp16 logits -> fp16 logits whose float64 sigmoid lies at least `margin_ulps` fp32 ulps away from every fp16 rounding midpoint
    (each offending logit moves up by 1/16, as often as needed: one fp16 step near 0 would barely move the sigmoid)."""
    c = np.array(c, dtype=np.float16)
    for _ in range(max_steps):
        y = 1.0 / (1.0 + np.exp(-c.astype(np.float64)))
        y16 = y.astype(np.float16)
        nb = np.nextafter(y16, np.where(y > y16.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)))
        mid = (y16.astype(np.float64) + nb.astype(np.float64)) / 2
        bad = np.abs(y - mid) < margin_ulps * U * np.maximum(y, 2.0 ** -126)
        if not bad.any():
            return c
        c[bad] = (c[bad].astype(np.float32) + 0.0625).astype(np.float16)
    raise AssertionError("clear_of_half_midpoints: logits stay at an fp16 rounding midpoint")


def tail(z, delta, near, far, bg, density_scale, mask, h0=None, c=None, sigma=None, rgb=None, half_rgb=True, dtype=torch.float64):
    """One ray per row: z, delta [N,T] (fp32 values), near, far [N], bg [N,3]; mask [N,T] bool (w > thresh as decided by the caller).
    The density enters as the logit h0 [N,T] (through trunc_exp) or as sigma [N,T]; the colour as the logits c [N,T,3] (through
    half(sigmoid)) or as rgb [N,T,3]. h0 / c become leaves that require grad (unless they already require it). Returns a dict of tensors (graph kept).
    dtype=torch.float32 evaluates the same expressions in fp32 (the bound's own test: an fp32 evaluation stays within it)."""
    f = lambda a: torch.as_tensor(a).to(dtype)
    z, delta, near, far, bg = f(z), f(delta), f(near), f(far), f(bg)
    mask = torch.as_tensor(mask, dtype=torch.bool)
    out = {}
    if h0 is not None:
        h0 = f(h0)
        h0 = h0 if h0.requires_grad else h0.detach().requires_grad_(True)
        sigma = _TruncExp.apply(h0)
        out["h0"] = h0
    else:
        sigma = f(sigma)
    if c is not None:
        c = f(c)
        c = c if c.requires_grad else c.detach().requires_grad_(True)
        rgb = _HalfSigmoid.apply(c) if half_rgb else torch.sigmoid(c)
        out["c"] = c
    else:
        rgb = f(rgb)
    alpha = 1 - torch.exp(-delta * density_scale * sigma)
    om = 1 - alpha + 1e-15
    trans = torch.cumprod(torch.cat([torch.ones_like(om[:, :1]), om[:, :-1]], -1), -1)
    w = alpha * trans
    ws = w.sum(-1)
    # the reference queries colour only where w > thresh (gather -> MLP -> scatter): a masked sample contributes no term at all
    image = torch.where(mask[..., None], w[..., None] * rgb, torch.zeros_like(rgb)).sum(-2) + (1 - ws)[:, None] * bg
    oz = ((z - near[:, None]) / (far - near)[:, None]).clamp(0, 1)
    depth = (w * oz).sum(-1)
    sumsq = (sigma * sigma).sum(-1)
    out.update(sigma=sigma, alpha=alpha, om=om, trans=trans, weights=w, weights_sum=ws, image=image, depth=depth, sumsq=sumsq, oz=oz,
               rgb=rgb, mask=mask, z=z, delta=delta, near=near, far=far, bg=bg, density_scale=float(density_scale), dtype=dtype)
    return out


def tail_backward(fwd, grad_image, grad_ws=None, grad_depth=None, grad_sumsq=None):
    """Gradients of sum(grad_image * image) + sum(grad_ws * weights_sum) + sum(grad_depth * depth) + sum(grad_sumsq * sumsq) with respect
    to h0 (grad_h0 [N,T]), c (grad_c [N,T,3]) and the weights through the image alone (grad_w [N,T]: what the separate composite
    backward hands the density head). A term that is None is absent.

    A ray whose grad_depth is 0 takes no depth term at all: the kernels skip `0 * oz`, and oz is NaN on a ray that misses the box
    (near = far). That is the contract — a caller that asks for no depth gradient gets finite rows — so the reference applies the same
    rule instead of torch's 0 * NaN."""
    f = lambda a: torch.as_tensor(a).to(fwd["dtype"])
    outs, gouts = [fwd["image"]], [f(grad_image)]
    if grad_ws is not None:
        outs.append(fwd["weights_sum"]); gouts.append(f(grad_ws))
    if grad_depth is not None:
        gd = f(grad_depth)
        oz = torch.where((gd != 0)[:, None], fwd["oz"], torch.zeros_like(fwd["oz"]))
        outs.append((fwd["weights"] * oz).sum(-1)); gouts.append(gd)
    if grad_sumsq is not None:
        outs.append(fwd["sumsq"]); gouts.append(f(grad_sumsq))
    leaves = [fwd[k] for k in ("h0", "c") if k in fwd]
    grads = torch.autograd.grad(outs, leaves, gouts, retain_graph=True, allow_unused=True)
    res = {}
    for k, g in zip([k for k in ("h0", "c") if k in fwd], grads):
        res["grad_" + k] = g if g is not None else torch.zeros_like(fwd[k])
    res["grad_w"], = torch.autograd.grad([fwd["image"]], [fwd["weights"]], [f(grad_image)], retain_graph=True)
    return res


def _suffix_after(x):
    """sum_{j>i} x_j along the last axis."""
    return torch.flip(torch.cumsum(torch.flip(x, [-1]), -1), [-1]) - x


def magnitudes(fwd, grad_image=None, grad_ws=None, grad_depth=None, grad_sumsq=None):
    """Per-element magnitudes (module docstring) of the forward outputs, and — when grad_image is given — of the backward's
    grad_h0 / grad_c / grad_w for those incoming gradients. The operations are the ones an fp32 evaluation performs; NaN where the
    value is NaN (rays that miss the box)."""
    with torch.no_grad():
        f = lambda a: torch.as_tensor(a).to(torch.float64)
        sig, alpha, om, T, w = (fwd[k].detach() for k in ("sigma", "alpha", "om", "trans", "weights"))
        delta, z, near, far, bg = fwd["delta"], fwd["z"], fwd["near"], fwd["far"], fwd["bg"]
        y, mask = fwd["rgb"].detach(), fwd["mask"]
        ds = fwd["density_scale"]
        m_sig = sig.clone() if "h0" in fwd else torch.zeros_like(sig)           # exp's rounding; sigma given as input: exact
        # values signed (a delta can come out negative in fp32 on a very short ray), magnitudes of absolute values
        dsd = delta * ds
        dds = dsd.abs()
        m_dds = dds if ds != 1.0 else torch.zeros_like(dds)
        x = dsd * sig
        m_x = m_dds * sig + dds * m_sig + x.abs()
        ex = torch.exp(-x)
        m_ex = ex * (m_x + 1)
        m_alpha = m_ex + alpha.abs()
        m_om = m_alpha + (1 - alpha).abs() + om
        # transmittance scan: mag(T_{i+1}) = mag(T_i) om_i + T_i mag(om_i) + T_{i+1}
        m_T = torch.zeros_like(T)
        for i in range(1, T.shape[1]):
            m_T[:, i] = m_T[:, i - 1] * om[:, i - 1] + T[:, i - 1] * m_om[:, i - 1] + T[:, i]
        m_w = m_alpha * T + alpha.abs() * m_T + w.abs()
        m_ws = m_w.sum(-1) + w.abs().sum(-1)
        oz_raw = (z - near[:, None]) / (far - near)[:, None]
        m_oz = 3 * oz_raw.abs()
        oz = fwd["oz"]
        m_depth = (m_w * oz + w.abs() * m_oz + 2 * (w * oz).abs()).sum(-1)
        wm = torch.where(mask, w.abs(), torch.zeros_like(w))[..., None]
        m_r = (torch.where(mask, m_w, torch.zeros_like(m_w))[..., None] * y + 2 * wm * y).sum(-2)
        rest = (1 - fwd["weights_sum"].detach())[:, None]
        m_image = m_r + (m_ws[:, None] + rest.abs()) * bg.abs() + (rest * bg).abs() + fwd["image"].detach().abs()
        m_sumsq = (2 * sig * m_sig + 2 * sig * sig).sum(-1)
        out = dict(sigma=m_sig.clone() if "h0" in fwd else None, trans=m_T, weights=m_w, weights_sum=m_ws, depth=m_depth, image=m_image,
                   sumsq=m_sumsq)
        if grad_image is None:
            return out
        g = f(grad_image)
        gws = f(grad_ws) if grad_ws is not None else torch.zeros_like(near)
        gdp = f(grad_depth) if grad_depth is not None else torch.zeros_like(near)
        gsq2 = 2 * f(grad_sumsq) if grad_sumsq is not None else torch.zeros_like(near)
        # composite backward: gw = -(g . bg) + [mask] (g . y)
        gy = (g[:, None, :] * y).abs().sum(-1)
        m_gw = 2 * (g * bg).abs().sum(-1)[:, None] + 2 * torch.where(mask, gy, torch.zeros_like(gy))
        gw_val = -(g * bg).sum(-1)[:, None] + torch.where(mask, (g[:, None, :] * y).sum(-1), torch.zeros_like(gy))
        on = (gdp != 0)[:, None]
        gdo = gdp[:, None] * torch.where(on, oz, torch.zeros_like(oz))
        gi = gw_val + gws[:, None] + gdo
        m_gi = m_gw + gws.abs()[:, None] + (gw_val + gws[:, None]).abs() + torch.where(on, gdp.abs()[:, None] * m_oz + 2 * gdo.abs(), torch.zeros_like(gi)) \
            + gi.abs()
        gwi = gi * w
        m_gwi = m_gi * w.abs() + gi.abs() * m_w + gwi.abs()
        S = _suffix_after(gwi)
        m_S = _suffix_after(m_gwi) + _suffix_after(gwi.abs())
        q = S / om
        m_q = m_S / om + S.abs() * m_om / (om * om) + q.abs()
        p = gi * T
        m_p = m_gi * T + gi.abs() * m_T + p.abs()
        da = p - q
        m_da = m_p + m_q + da.abs()
        dsig = da * dsd * ex
        m_dsig = (m_da * dds + da.abs() * m_dds + (da * dds).abs()) * ex + (da * dds).abs() * m_ex + dsig.abs()
        dsig2 = dsig + gsq2[:, None] * sig
        m_dsig2 = m_dsig + (gsq2[:, None] * m_sig).abs() + dsig2.abs()
        e_lo, e_hi = float(np.exp(-15.0)), float(np.exp(15.0))
        cf = sig.clamp(e_lo, e_hi)
        m_cf = torch.where((sig > e_lo) & (sig < e_hi), m_sig, cf)
        m_dh0 = m_dsig2 * cf + dsig2.abs() * m_cf + (dsig2 * cf).abs()
        yy = y * (1 - y)
        m_gc = torch.where(mask[..., None], g[:, None, :].abs() * (m_w[..., None] * yy + 3 * w.abs()[..., None] * yy), torch.zeros_like(y))
        out.update(grad_h0=m_dh0, grad_c=m_gc, grad_w=m_gw)
        return out
