"""Float64 reference of the DIFFERENTIABLE depth of the occupancy-grid training tail (include/focnerf.h foc_occ_tail_forward_depth /
_backward_depth), on top of ragged_ref.py and distortion_ref.py (imported, unchanged):

    depth_raw = sum_{i<=stop} w_i t_i        depth = clamp(depth_raw - near, min=0) / (far - near)        t_i = sum_{j<=i} dt1_j

with the graph kept (ragged_ref.train detaches it for the reference's semantics): `evaluate` adds sum(grad_depth * depth) to the loss whose
gradient torch.autograd.grad carries to h0. t, near and far carry no gradient, so grad_c takes nothing from the depth.

`term()` is the kernel's closed form (csrc/ragged.h ot_depth_scale / ot_depth_bwd_step), per ray and sample:

    s = (depth_raw - near < 0 || !(far > near)) ? 0 : grad_depth / (far - near)
    grad_sigma_i += dt0_i s (T_after_i t_i - (depth_raw - D_acc_i))     on the samples that count,     D_acc_i = sum_{j<=i} w_j t_j

evaluated in a given dtype from a forward of that dtype (test_depth_ref.py: float64 against autograd, fp32 against the bound) with
`mutant=` naming a deliberately wrong variant (MUTANTS); a reference value is never computed with one.

Magnitudes (the rules of fixed_tail_ref.py's docstring, as distortion_ref.py applies them): the sum of the absolute values of every term
entering an output. D_acc is a running sum: it enters with the magnitudes plus the absolute values of ITS terms; the total depth_raw enters
with the forward's own magnitude. The depth's share B of grad_h0 goes through the density chain on its own and
mag(grad_h0) = mag(the other terms, from their files) + mag(B) + |their sum|.

Cases: ragged_ref.train_cases() with nears / fars REPLACED (`cases()`): as drawn, 130 of their 156 fitting rays are clamped and a wrong
depth gradient would pass. Per ray (output row k) from the float64 depth_raw at the natural stop, m = 0.05 max(1, |depth_raw|):
k % 4 != 3: near = depth_raw - m (unclamped); k % 4 == 3: near = depth_raw + m (clamped); far = near + the case's own (far - near).
On 4 of the 156 fitting rays (dense rays of 128 .. 1024 samples whose first-order magnitude of depth_raw is 250 .. 6600) the forward bound
itself exceeds 0.05: there m is 4 x that bound instead, so that the condition below holds for them too; clamped stays clamped.
`clamp_is_decided()` is the condition the tests assert on the reference alone: no fitting ray has |depth_raw - near| within the forward
bound of depth_raw, at any stop candidate of the ray — fp32 then takes float64's clamp branch.
"""
import numpy as np
import torch

import distortion_ref as D
import ragged_ref as R
from fixed_tail_ref import U

C, K = R.C, R.K
MUTANTS = ("no_depth", "D_exclusive", "no_clamp", "no_span", "t_carry", "behind_stop")


# ---------------------------------------------------------------- cases
_CASES = None


def cases():
    """ragged_ref.train_cases() with nears / fars replaced (module docstring) and a `grad_depth` [N] by output row: N(0, 1), seeded per
    case, both signs, every fifth ray from the second on exactly 0. Built once."""
    global _CASES
    if _CASES is None:
        _CASES = []
        for d in R.train_cases():
            _, mags, fwd = R.evaluate(d, "tail", None, mags=True)
            L = fwd["L"]
            raw = fwd["depth_raw"].detach().numpy()                      # by output row
            bound = C * U * (L["T"][L["inverse"]] + K) * mags["depth_raw"]     # by output row, as ragged_ref.evaluate leaves this magnitude
            m = np.maximum(0.05 * np.maximum(1.0, np.abs(raw)), 4.0 * bound)
            clamped = np.arange(d["N"]) % 4 == 3
            span = d["fars"].astype(np.float64) - d["nears"].astype(np.float64)
            near = np.where(clamped, raw + m, raw - m).astype(np.float32)
            d = dict(d, nears=near, fars=(near.astype(np.float64) + span).astype(np.float32), clamped=clamped)
            g = np.random.default_rng(7000 + 7 * d["N"] + d["total"]).normal(0, 1, d["N"]).astype(np.float32)
            g[1::5] = 0.0
            d["grad_depth"] = g
            _CASES.append(d)
    return _CASES


def clamp_is_decided(case, cands):
    """Per stop candidate: every fitting ray's |depth_raw - near| against the forward bound C 2^-24 (T + K) mag(depth_raw) (+ (T + K) 2^-126).
    Returns the smallest margin |depth_raw - near| / bound over the fitting rays and candidates (> 1: decided) and the number of fitting rays
    float64 leaves unclamped at the natural stop."""
    worst, unclamped = np.inf, 0
    for k in range(max(len(c) for c in cands)):
        vals, mags, fwd = R.evaluate(case, "tail", R.stops_of(cands, k), mags=True)
        L = fwd["L"]
        raw = R.by_list(L, fwd["depth_raw"].detach().numpy())
        bound = C * U * (L["T"] + K) * R.by_list(L, mags["depth_raw"]) + (L["T"] + K) * R.TINY
        near = R.by_list(L, case["nears"]).astype(np.float64)
        fits = L["fits"]
        if fits.any():
            worst = min(worst, float((np.abs(raw - near)[fits] / bound[fits]).min()))
        if k == 0:
            unclamped = int(((raw - near >= 0) & fits).sum())
    return worst, unclamped


# ---------------------------------------------------------------- the float64 statement
def depth_of(fwd):
    """ragged_ref.train()'s result -> the normalised depth [N] by output row, graph kept."""
    return (fwd["depth_raw"] - fwd["near"]).clamp(min=0) / (fwd["far"] - fwd["near"])


def term(fwd, grad_depth, mutant=None):
    """The kernel's closed form (module docstring) in fwd's dtype: the depth's share of grad_h0, padded [N,Tmax] in list order."""
    L, dtype = fwd["L"], fwd["dtype"]
    with torch.no_grad():
        idx = torch.from_numpy(L["index"])
        w, Ta, dt0, act, valid = fwd["weights"], fwd["T_after"], fwd["dt0"], fwd["act"], fwd["valid"]
        t = fwd["t"]
        if mutant == "t_carry":
            t = R._chunk_cumop(torch.where(valid, fwd["dt1"], torch.zeros_like(t)), torch.cumsum, False)
        raw, near, far = fwd["depth_raw"][idx], fwd["near"][idx], fwd["far"][idx]
        g = torch.as_tensor(np.asarray(grad_depth)).to(dtype)[idx]
        zero = torch.zeros_like(g)
        s = g if mutant == "no_span" else g / (far - near)
        if mutant != "no_clamp":
            s = torch.where((raw - near < 0) | ~(far > near), zero, s)
        if mutant == "no_depth":
            s = zero
        wt = w * t
        D_acc = torch.cumsum(wt, -1)
        if mutant == "D_exclusive":
            D_acc = D_acc - wt
        inner = s[:, None] * (Ta * t - (raw[:, None] - D_acc))
        gs = torch.where(valid if mutant == "behind_stop" else act, dt0 * inner, torch.zeros_like(w))
        ds = fwd["density_scale"]
        if ds != 1.0:
            gs = ds * gs
        e = fwd["e"]
        cf = e.clamp(float(np.exp(-15.0)), float(np.exp(15.0)))
        return torch.where(valid, gs * cf, torch.zeros_like(w))


def evaluate(case, stop, on=None, grad_depth=None, grad_dist=None, bg_ray=True, dtype=torch.float64, mags=False):
    """distortion_ref.ragged_evaluate() (ragged_ref.evaluate() of the tail form plus the distortion) with depth_raw [N] (list order) added to
    the values and sum(grad_depth * depth) to the loss whose gradients it returns (grad_depth [N] by output row; None: absent), and their
    magnitudes to the magnitudes. Returns (values, magnitudes or None, fwd)."""
    vals, m, fwd = D.ragged_evaluate(case, stop, on=on, grad_dist=grad_dist, bg_ray=bg_ray, dtype=dtype, mags=mags)
    L = fwd["L"]
    vals["depth_raw"] = R.by_list(L, fwd["depth_raw"].detach().to(torch.float64).numpy())
    gd = None
    if grad_depth is not None and on is not None:
        gd = torch.as_tensor(np.asarray(grad_depth)).to(dtype)
        g, = torch.autograd.grad([depth_of(fwd)], [fwd["h0"]], [gd], retain_graph=True)
        vals["grad_h0"] = vals["grad_h0"] + g.to(torch.float64).numpy()
    if not mags:
        return vals, None, fwd
    m["depth_raw"] = R.by_list(L, m["depth_raw"])                     # ragged_ref.evaluate leaves this one by output row
    if gd is None:
        return vals, m, fwd
    with torch.no_grad():
        d = lambda k: fwd[k].detach().to(torch.float64)
        base = R.train_magnitudes(fwd)
        w, t, dt0, Ta, act, valid = d("weights"), d("t"), d("dt0"), d("T_after"), fwd["act"], fwd["valid"]
        z = torch.zeros_like(w)
        idx = torch.from_numpy(L["index"])
        m_w, m_Ta = base["weights"], base["T_after"]
        m_t = torch.cumsum(torch.where(valid, d("dt1").abs(), z), 1)
        raw, m_raw = d("depth_raw")[idx], base["depth_raw"][idx]
        near, far = d("near")[idx], d("far")[idx]
        g = gd.to(torch.float64)[idx]
        den = far - near
        live = (raw - near >= 0) & (far > near)
        s = torch.where(live, g / den, torch.zeros_like(g))
        m_s = torch.where(live, g.abs() * den.abs() / (den * den) + s.abs(), torch.zeros_like(g))
        wt = w * t
        m_wt = m_w * t.abs() + w.abs() * m_t + wt.abs()
        D_acc = torch.cumsum(wt, 1)
        m_D = torch.cumsum(m_wt, 1) + torch.cumsum(wt.abs(), 1)
        rest = raw[:, None] - D_acc
        m_rest = m_raw[:, None] + m_D + rest.abs()
        Tt = Ta * t
        m_Tt = m_Ta * t.abs() + Ta * m_t + Tt.abs()
        inn = Tt - rest
        m_inn = m_Tt + m_rest + inn.abs()
        e = s[:, None] * inn
        m_e = s.abs()[:, None] * m_inn + m_s[:, None] * inn.abs() + e.abs()
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
        m["depth_term"] = m_B.numpy()
        m["grad_h0"] = m["grad_h0"] + m_B.numpy() + np.abs(vals["grad_h0"])
    return vals, m, fwd
