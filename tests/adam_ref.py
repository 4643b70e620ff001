"""float64 statement of one optimizer step of focnerf_amd.optim (csrc/optim.hip): unscale, skip rule, L2 weight decay, moments, bias
corrections, update, and the loss scale's update rule; plus the fp32 error bounds the GPU tests hold the kernels to. numpy only.

Checked by tests/test_optim_host.py against torch.optim.Adam on CPU float64 tensors and against torch._amp_update_scale_'s rule."""
import numpy as np

U = 2.0 ** -24          # one fp32 rounding: relative error at most U


def scale_rule(scale, tracker, found_inf, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch._amp_update_scale_: (scale, tracker) after a step, in fp32 arithmetic as the kernel does it."""
    scale = np.float32(scale)
    if found_inf:
        return float(scale * np.float32(backoff_factor)), 0
    successful = int(tracker) + 1
    if successful == int(growth_interval):
        with np.errstate(over="ignore"):
            grown = scale * np.float32(growth_factor)
        return float(grown if np.isfinite(grown) else scale), 0
    return float(scale), successful


def adam_step(p, grad_scaled, m, v, step, *, scale=1.0, lr, betas, eps, weight_decay=0.0):
    """One step of one tensor in float64. `grad_scaled` carries the loss scale `scale`; `step` is the counter BEFORE the step.
    Returns a dict: skipped, p, m, v, step (after), and the intermediates the bounds need (g, denom, step_size, bc2_sqrt)."""
    p, grad_scaled, m, v = (np.asarray(a, dtype=np.float64) for a in (p, grad_scaled, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    if not np.isfinite(grad_scaled).all():
        return {"skipped": True, "p": p, "m": m, "v": v, "step": float(step)}
    t = float(step) + 1.0
    g = grad_scaled * (1.0 / float(scale))
    if weight_decay != 0:
        g = g + float(weight_decay) * p
    m_new = m + (g - m) * (1.0 - b1)
    v_new = b2 * v + (1.0 - b2) * g * g
    step_size = float(lr) / (1.0 - b1 ** t)
    bc2_sqrt = np.sqrt(1.0 - b2 ** t)
    denom = np.sqrt(v_new) / bc2_sqrt + float(eps)
    p_new = p - step_size * m_new / denom
    return {"skipped": False, "p": p_new, "m": m_new, "v": v_new, "step": t, "g": g, "denom": denom, "step_size": step_size, "bc2_sqrt": bc2_sqrt}


def any_nonfinite(grads):
    return any(not np.isfinite(np.asarray(g)).all() for g in grads)


def ulp32(x):
    """Spacing of fp32 at |x| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def fp32_bounds(ref, p_old, m_old, *, scale, betas, weight_decay=0.0):
    """Largest |kernel - float64| the fp32 path of csrc/optim.hip may show, per element, for `ref = adam_step(...)` computed from the
    kernel's own fp32 inputs. Counted from the kernel's operations, each correctly rounded (relative error <= U = 2^-24 per rounding):

      g   = grad * inv_scale                exact when the scale is a power of two (every scale the tests use); otherwise inv_scale =
                                            fp32(1 / scale) and the product round: 2 U |g|
            fma(wd32, p, g)                 only with weight decay: wd32 = fp32(wd) moves the product by U |wd p|, the fma rounds: U |g|
                                            -> dg = the sum of these (0 for a power-of-two scale without weight decay)
      v   = fma(omb2_32, g * g, b2_32 * v)  b2_32 and the product b2 v: 2 U on that term; omb2_32 and g * g: 2 U on that term; the fma: U
                                            -> 3 U v <= 3 ulp(v): the bound is 4 ulp(v_ref), plus (1 - b2)(2 |g| dg + dg^2) where dg != 0
      m   = fma(g - m, omb1_32, m)          g - m rounds (U |g - m| <= 2 U max), omb1_32 rounds (U), both times (1 - b1) <= 1, the fma
                                            rounds (U |m_new| <= U max) -> below 4 U max(|m_old|, |g|), plus (1 - b1) dg
      p   = p - step32 * m / (sqrt(v) / bc2_32 + eps32)
                                            sqrt(v): 1.5 U from v's 3 U, U of its own; bc2_32, the division, eps32 + the addition, step32,
                                            the product, the division: 7 U; m: 4 U max / |m| -> below 16 U step_size max(|m_old|, |g|) /
                                            denom, plus half an ulp of p for the subtraction; where dg != 0 its share through m and v.
    These are the bounds of the feature's specification with the dg terms spelled out; nothing here is fitted to an output."""
    b1, b2 = float(betas[0]), float(betas[1])
    g, denom, step_size = np.abs(ref["g"]), ref["denom"], ref["step_size"]
    s = float(scale)
    dg = np.zeros_like(g) if s > 0 and np.log2(s) == np.floor(np.log2(s)) else 2 * U * g
    if weight_decay != 0:
        dg = dg + U * (np.abs(float(weight_decay) * np.asarray(p_old, dtype=np.float64)) + g)
    mx = np.maximum(np.abs(np.asarray(m_old, dtype=np.float64)), g)
    dv_extra = (1.0 - b2) * (2.0 * g * dg + dg * dg)
    dm_extra = (1.0 - b1) * dg
    sqrt_v = np.sqrt(ref["v"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ddenom_extra = np.where(sqrt_v > 0, dv_extra / (2.0 * sqrt_v * ref["bc2_sqrt"]), np.sqrt(dv_extra) / ref["bc2_sqrt"])
    dp_extra = step_size * (dm_extra / denom + np.abs(ref["m"]) * ddenom_extra / (denom * denom))
    return {"v": 4.0 * ulp32(ref["v"]) + dv_extra,
            "m": 4.0 * U * mx + dm_extra,
            "p": 0.5 * ulp32(ref["p"]) + 16.0 * U * step_size * mx / denom + dp_extra}
