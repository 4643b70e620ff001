"""Regularisers on the compositing weights, as plain torch expressions.

`ray_distortion` is the distortion term of mip-NeRF 360 per ray: the value the fused training tails return as `results['distortion']`
(include/focnerf.h foc_fixed_tail_forward_dist / foc_occ_tail_forward_dist), for the routes on which the weights exist as an autograd
tensor. `results['distortion'].mean()` is the reference's `loss.eff_distloss(w, m, interval)`.
"""
import torch


def ray_distortion(weights, m, interval):
    """weights, m [..., T] in depth order, interval [..., T] or a scalar -> [...]:

        sum_i interval_i w_i^2 / 3  +  2 sum_i w_i (m_i W_i - V_i),    W_i = sum_{j<i} w_j,  V_i = sum_{j<i} w_j m_j

    which equals sum_ij w_i w_j |m_i - m_j| + sum_i w_i^2 interval_i / 3 for non-decreasing m. The sums in front of a sample are the
    running sums shifted by one place, so the cost is linear in T. Only the weights carry a gradient: m and interval are detached."""
    m = m.detach()
    interval = interval.detach() if torch.is_tensor(interval) else interval
    wm = weights * m

    def in_front(x):
        running = torch.cumsum(x, dim=-1)
        return torch.cat([torch.zeros_like(running[..., :1]), running[..., :-1]], dim=-1)

    within = interval * weights * weights / 3
    between = 2 * weights * (m * in_front(weights) - in_front(wm))
    return (within + between).sum(dim=-1)
