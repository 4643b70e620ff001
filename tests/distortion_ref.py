"""Float64 reference of the per-ray distortion the training tails return (include/focnerf.h foc_fixed_tail_forward_dist /
foc_occ_tail_forward_dist) and of its backward, for both sample layouts, on top of fixed_tail_ref.py and ragged_ref.py (imported, unchanged):

    dist = sum_i (1/3) delta_i w_i^2 + 2 sum_i w_i (m_i W_<i - WM_<i),      W_<i = sum_{j<i} w_j,   WM_<i = sum_{j<i} w_j m_j
    G_i  = d dist / d w_i = (2/3) delta_i w_i + 2 (m_i (W_<i - W_>i) + (WM_>i - WM_<i))

fixed-step: w = the tail's raw weights, m = (z - near) + delta / 2, interval delta (fp32 inputs, as FsSample forms them); a ray with
!(far > near) has dist = 0, ray_wm = 0 and takes no distortion gradient. ragged: w = the composite's weights (0 behind the stop), m = the
running sum t of dt1, interval dt0; a ray that does not fit has 0. m and delta carry no gradient; autograd carries the gradient of
sum(grad_dist * dist) through the family's own graph to h0 (`fixed_backward`, `ragged_evaluate`).

Magnitudes (the rules of fixed_tail_ref.py's docstring; the bound is C * 2^-24 * (T + K) * mag, C = 2, K = 16, as in both families): `mag` is
the sum of absolute values of every term entering an output. A term that is itself a running sum (W_<i, WM_<i, their counterparts behind
the sample, the running sum of G_j w_j) enters with the magnitudes plus the absolute values of ITS terms — it counts twice: once for its own
summation, once for the outer one it enters. For the sums behind / in front of a sample that a backward forms as total - other side -
own, the magnitude is that of the total (the forward's output, with the forward's magnitude) plus the whole ray's sum of |terms|: a bound
that holds whichever side the kernel walks from. The distortion's share B of grad_h0 goes through the family's backward chain on its own
(the chain is linear in the gradient of the weights, and every magnitude rule is sub-additive), and
mag(grad_h0) = mag(A, the family's own terms, from the family's file) + mag(B) + |A + B|.
"""
import numpy as np
import torch

import fixed_tail_ref as F
import ragged_ref as R
from fixed_tail_ref import U  # noqa: F401

C, K = R.C, R.K


def _front(x):
    """sum_{j<i} x_j along the last axis."""
    return torch.cumsum(x, -1) - x


def distortion(w, m, delta):
    """Per ray (last axis in depth order): (dist, sum w m). The graph runs through w only."""
    m, delta = m.detach(), delta.detach() if torch.is_tensor(delta) else delta
    wm = w * m
    return ((1.0 / 3.0) * delta * (w * w) + 2 * (w * (m * _front(w) - _front(wm)))).sum(-1), wm.sum(-1)


def pairwise(w, m, delta):
    """The O(T^2) definition: sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i."""
    return (w[..., :, None] * w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum((-1, -2)) + ((w * w) * delta).sum(-1) / 3


def weight_gradient(w, m, delta):
    """G_i in closed form (module docstring)."""
    wm = w * m
    Wb, WMb = _front(w), _front(wm)
    Wa, WMa = w.sum(-1, keepdim=True) - Wb - w, wm.sum(-1, keepdim=True) - WMb - wm
    return (2.0 / 3.0) * delta * w + 2 * (m * (Wb - Wa) + (WMa - WMb))


def magnitudes(w, m_w, m, m_m, delta, m_W_total):
    """float64 tensors [N,T] (m_W_total [N]: the magnitude of the forward's weights_sum) -> dict of the magnitudes of dist [N], wm [N] and
    G [N,T], and G itself."""
    aw, wm = w.abs(), w * m
    m_wm = m_w * m.abs() + aw * m_m + wm.abs()
    Wb, WMb = _front(w), _front(wm)
    m_Wb, m_WMb = _front(m_w) + _front(aw), _front(m_wm) + _front(wm.abs())
    mWb = m * Wb
    inner = mWb - WMb
    m_inner = m_m * Wb.abs() + m.abs() * m_Wb + mWb.abs() + m_WMb + inner.abs()
    bi = 2 * w * inner
    m_bi = 2 * (m_w * inner.abs() + aw * m_inner) + bi.abs()
    uni = delta * w * w / 3
    m_uni = (2.0 / 3.0) * delta.abs() * aw * m_w + 3 * uni.abs()
    m_dist = (m_uni + m_bi).sum(-1) + (uni.abs() + bi.abs()).sum(-1)
    m_WM_total = m_wm.sum(-1) + wm.abs().sum(-1)
    # the backward: one side of a sample is a running sum, the other total - that side - own (module docstring: one bound for both)
    W, WM = w.sum(-1, keepdim=True), wm.sum(-1, keepdim=True)
    Wa, WMa = W - Wb - w, WM - WMb - wm
    S_w, S_wm = (m_w.sum(-1) + aw.sum(-1))[:, None], m_WM_total[:, None]
    side = lambda tot, m_tot, S, own, x: m_tot[:, None] + S + own + tot.abs() + x.abs()
    m_Wb2, m_Wa2 = side(W, m_W_total, S_w, m_w, Wb), side(W, m_W_total, S_w, m_w, Wa)
    m_WMb2, m_WMa2 = side(WM, m_WM_total, S_wm, m_wm, WMb), side(WM, m_WM_total, S_wm, m_wm, WMa)
    d1, d2 = Wb - Wa, WMa - WMb
    m_d1, m_d2 = m_Wb2 + m_Wa2 + d1.abs(), m_WMb2 + m_WMa2 + d2.abs()
    t1 = m * d1
    m_t1 = m_m * d1.abs() + m.abs() * m_d1 + t1.abs()
    inn = t1 + d2
    m_inn = m_t1 + m_d2 + inn.abs()
    un = (2.0 / 3.0) * delta * w
    m_un = (2.0 / 3.0) * delta.abs() * m_w + 2 * un.abs()
    G = un + 2 * inn
    return dict(dist=m_dist, wm=m_WM_total, G=G, m_G=m_un + 2 * m_inn + G.abs())


# ---------------------------------------------------------------- fixed-step layout (fixed_tail_ref.tail)
def fixed(fwd):
    """fixed_tail_ref.tail()'s result -> dict(dist [N], wm [N], w, m, delta [N,T], live [N]) in the evaluation's dtype (graph kept)."""
    live = (fwd["far"] > fwd["near"])
    z = torch.zeros_like(fwd["z"])
    m = (fwd["z"] - fwd["near"][:, None]) + 0.5 * fwd["delta"]
    w = torch.where(live[:, None], fwd["weights"], z)
    m, delta = torch.where(live[:, None], m, z), torch.where(live[:, None], fwd["delta"], z)
    dist, wm = distortion(w, m, delta)
    return dict(dist=dist, wm=wm, w=w, m=m, delta=delta, live=live)


def fixed_backward(fwd, dd, grad_dist, **grads):
    """fixed_tail_ref.tail_backward() of the family's terms plus sum(grad_dist * dist): grad_h0 [N,T], grad_c [N,T,3]."""
    res = F.tail_backward(fwd, **grads)
    g, = torch.autograd.grad([dd["dist"]], [fwd["h0"]], [torch.as_tensor(grad_dist).to(fwd["dtype"])], retain_graph=True)
    return dict(grad_h0=res["grad_h0"] + g, grad_c=res["grad_c"])


def fixed_magnitudes(fwd, dd, grad_dist=None, **grads):
    """Magnitudes of dist, wm and — with grad_dist — of fixed_backward()'s grad_h0 / grad_c (float64 fwd)."""
    A = F.tail_backward(fwd, **grads)["grad_h0"] if grad_dist is not None else None
    with torch.no_grad():
        base = F.magnitudes(fwd, **grads)
        z = torch.zeros_like(dd["w"])
        live = dd["live"][:, None]
        m_w = torch.where(live, torch.nan_to_num(base["weights"], nan=0.0), z)
        m_m = torch.where(live, (fwd["z"] - fwd["near"][:, None]).abs() + dd["m"].abs(), z)
        mg = magnitudes(dd["w"].detach(), m_w, dd["m"], m_m, dd["delta"], torch.where(dd["live"], torch.nan_to_num(base["weights_sum"], nan=0.0), z[:, 0]))
        out = dict(dist=mg["dist"], wm=mg["wm"])
        if grad_dist is None:
            return out
        gd = torch.as_tensor(grad_dist).to(torch.float64)[:, None]
        e = gd * mg["G"]
        gi, m_gi = e, gd.abs() * mg["m_G"] + 2 * e.abs()
        # the density head's backward for this share of the weights' gradient (fixed_tail_ref.magnitudes, its rules and names)
        sig, alpha, om, T, w = (fwd[k].detach() for k in ("sigma", "alpha", "om", "trans", "weights"))
        ds = fwd["density_scale"]
        dsd = fwd["delta"] * ds
        dds = dsd.abs()
        m_dds = dds if ds != 1.0 else torch.zeros_like(dds)
        x = dsd * sig
        m_x = m_dds * sig + dds * sig + x.abs()
        ex = torch.exp(-x)
        m_ex = ex * (m_x + 1)
        m_om = m_ex + alpha.abs() + (1 - alpha).abs() + om
        m_T = base["trans"]
        gwi = gi * w
        m_gwi = m_gi * w.abs() + gi.abs() * base["weights"] + gwi.abs()
        S = F._suffix_after(gwi)
        m_S = F._suffix_after(m_gwi) + F._suffix_after(gwi.abs())
        q = S / om
        m_q = m_S / om + S.abs() * m_om / (om * om) + q.abs()
        p = gi * T
        m_p = m_gi * T + gi.abs() * m_T + p.abs()
        da = p - q
        m_da = m_p + m_q + da.abs()
        dsig = da * dsd * ex
        m_dsig = (m_da * dds + da.abs() * m_dds + (da * dds).abs()) * ex + (da * dds).abs() * m_ex + dsig.abs()
        e_lo, e_hi = float(np.exp(-15.0)), float(np.exp(15.0))
        cf = sig.clamp(e_lo, e_hi)
        m_cf = torch.where((sig > e_lo) & (sig < e_hi), sig, cf)
        B = dsig * cf
        m_B = torch.where(live, m_dsig * cf + dsig.abs() * m_cf + B.abs(), z)
        out.update(grad_h0=base["grad_h0"] + m_B + (A + torch.where(live, B, z)).abs(), grad_c=base["grad_c"])
        return out


FIXED_T = (2, 63, 64, 65, 128, 129, 200)
FIXED_N = (1, 3, 4, 5, 37)


def fixed_case(N, T, cfg):
    """The draw of test_gpu_fixed_tail_reference.py for N x T (transparent, typical, opaque, clamp and box-missing rays), configuration `cfg`
    (0: noise, the sums of sigma^2, a per-ray background, c_width 4, density_scale 1; 1: none of them, c_width 16, density_scale 3), and its
    incoming gradients: all the family's terms plus grad_dist (every fourth ray exactly 0)."""
    from test_gpu_fixed_tail_reference import TERMS, _draw, _grads_of
    d = _draw(N, T, 100 * T + 10 * N + cfg)
    g = {k: v for k, v in _grads_of(d, TERMS if cfg == 0 else TERMS[:3]).items() if v is not None}
    gd = d["rng"].normal(0, 1, N).astype(np.float32)
    gd[::4] = 0.0
    if N == 1:
        gd[:] = 0.7
    return d, g, gd, dict(noise=cfg == 0, sumsq=cfg == 0, bg_ray=cfg == 0, c_width=(4, 16)[cfg], ds=(1.0, 3.0)[cfg], thresh=(1e-10, 1e-4)[cfg])


# ---------------------------------------------------------------- ragged layout (ragged_ref.train, tail form)
def grad_dist_of(case):
    """The incoming grad_dist [N] of a ragged case, by output row: N(0, 1), every fifth ray exactly 0 (the plain backward's bits there)."""
    g = np.random.default_rng(9000 + 7 * case["N"] + case["total"]).normal(0, 1, case["N"]).astype(np.float32)
    g[::5] = 0.0
    return g


def ragged_evaluate(case, stop, on=None, grad_dist=None, bg_ray=True, dtype=torch.float64, mags=False):
    """ragged_ref.evaluate(case, "tail", ...) with ray_dist / ray_wm [N] (list order) added to the values, sum(grad_dist * dist) to the loss
    whose gradients it returns (grad_dist [N] by output row; `on` as there), and their magnitudes to the magnitudes."""
    vals, m, fwd = R.evaluate(case, "tail", stop, on=on, bg_ray=bg_ray, dtype=dtype, mags=mags)
    L = fwd["L"]
    w, t, dt0 = fwd["weights"], fwd["t"], fwd["dt0"]
    dist, wm = distortion(w, t, dt0)
    vals.update(ray_dist=dist.detach().to(torch.float64).numpy(), ray_wm=wm.detach().to(torch.float64).numpy())
    gd = None
    if grad_dist is not None and on is not None:
        gd = torch.as_tensor(R.by_list(L, grad_dist)).to(dtype)
        g, = torch.autograd.grad([dist], [fwd["h0"]], [gd], retain_graph=True)
        A = vals["grad_h0"]
        vals["grad_h0"] = A + g.to(torch.float64).numpy()
    if not mags:
        return vals, None, fwd
    with torch.no_grad():
        d = lambda k: fwd[k].detach().to(torch.float64)
        base = R.train_magnitudes(fwd, **(R.grads_of(case, on, "tail") if on is not None else {}))
        w, t, dt0, Ta, act, valid = d("weights"), d("t"), d("dt0"), d("T_after"), fwd["act"], fwd["valid"]
        z = torch.zeros_like(w)
        m_t = torch.cumsum(torch.where(valid, d("dt1").abs(), z), 1)
        m_ws = torch.as_tensor(R.by_list(L, base["weights_sum"].numpy()))
        mg = magnitudes(w, base["weights"], t, m_t, dt0, m_ws)
        m.update(ray_dist=mg["dist"].numpy(), ray_wm=mg["wm"].numpy())
        if gd is None:
            return vals, m, fwd
        gd = gd.to(torch.float64)[:, None]
        G, m_G = mg["G"], mg["m_G"]
        Gw = G * w
        m_Gw = m_G * w.abs() + G.abs() * base["weights"] + Gw.abs()
        P, m_P = torch.cumsum(Gw, 1), torch.cumsum(m_Gw, 1) + torch.cumsum(Gw.abs(), 1)
        two = 2 * d("weights").new_tensor(vals["ray_dist"])[:, None]
        rest = two - P
        m_rest = 2 * mg["dist"][:, None] + m_P + rest.abs()
        GT = G * Ta
        m_GT = m_G * Ta + G.abs() * base["T_after"] + GT.abs()
        inn = GT - rest
        m_inn = m_GT + m_rest + inn.abs()
        e = gd * inn
        m_e = gd.abs() * m_inn + 2 * e.abs()
        gs = torch.where(act, dt0 * e, z)
        m_gs = torch.where(act, dt0.abs() * m_e + gs.abs(), z)
        ds = fwd["density_scale"]
        if ds != 1.0:
            gs = ds * gs
            m_gs = ds * m_gs + gs.abs()
        ex = d("e")
        e_lo, e_hi = float(np.exp(-15.0)), float(np.exp(15.0))
        cf = ex.clamp(e_lo, e_hi)
        m_cf = torch.where((ex > e_lo) & (ex < e_hi), ex, cf)
        m_B = torch.where(valid, m_gs * cf + gs.abs() * m_cf + (gs * cf).abs(), z)
        m["grad_h0"] = m["grad_h0"] + m_B.numpy() + np.abs(vals["grad_h0"])
    return vals, m, fwd
