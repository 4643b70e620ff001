"""GPU: the occupancy-grid path's compositing kernels against the float64 reference of the operation (tests/ragged_ref.py), through the raw
ABI so that no MLP noise enters: the training composite (foc_composite_rays_train_forward / _backward: k_composite_train_fwd / _bwd), the
one-kernel tail (foc_occ_tail_forward / _backward and the _sumsq twins: k_occ_tail_fwd / _bwd) and the inference burst (foc_composite_rays,
foc_composite_compact: k_composite_rays, k_composite_rays_pre<4|8|16>, both sample layouts).

Cases (ragged_ref.train_cases / burst_cases; test_ragged_ref.py holds an fp32 CPU evaluation of the same cases to the same bound): ray
lengths from {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1024}, 1 / 3 / 4 / 5 / 37 rays (four rays per workgroup, a ragged last one), rays that
are transparent, typical, opaque from a random sample on, at trunc_exp's clamp (h0 = +-14.5, +-15, +-15.0078125, 16.5), with sigma = 0
samples, colour logits +7 and +-12; constructed rays whose T_after is 2 T_thresh before and T_thresh / 2 after a stop at sample 0, 62, 63, 64,
127, 128 or the last one, and opaque rays with T_thresh = 0 that never stop; T_thresh 1e-4, 1e-3, 1e-2, 0; lists cut so that the last rays do
not fit (one with offset > M), a permuted rays[:, 0], rows behind counter[0] up to the 128-row pad. Bursts of 1, 3, 4, 8, 16 slots over 1, 63,
64, 65, 1025 list entries with -1 entries, ending on dt0 == 0 at slot 0 and in the middle, from accumulators that are zero, random, and
2 T_thresh / half T_thresh short of opaque.

Bound per element: |kernel - float64| <= C * 2^-24 * (T + K) * mag, C = 2, K = 16 (T: the ray's sample count, the burst's slot count; + half
an fp16 ulp on the fp16 gradients, + (T + K) 2^-126 on fp32 values), mag from ragged_ref: no allowance of bad rows or rays anywhere. The
stop is a discontinuous decision: all of a ray's outputs, forward and backward, must lie within the bound of the reference at ONE of the
stops float64 cannot exclude (ragged_ref.stop_candidates); a decided ray has exactly one, and at most 2 % of a case's rays, none of a
constructed one, are undecided (asserted here again on the reference alone). The tail's grad_c has a second fp16 rounding point — torch's
half sigmoid backward receives g w as a half — which adds half an fp16 ulp of g w times y (1 - y) to that output's allowance.

Measured on MI355X over every case of this file, worst ratio |kernel - float64| / (2^-24 (T + K) mag) per output (asserted C = 2):
training composite 0.031 (weights_sum, depth, image, grad_rgb), 0.013 (grad_sigma); tail 0.031 (weights_sum, image_raw), 0.020 (sumsq),
0.018 (image), 0.0026 (grad_h0), 0.0022 (grad_c), 0.0005 (depth); burst 0.16 (rays_t), 0.076 (image), 0.061 (depth), 0.050 (weights_sum); every
kill decision float64's. A margin of 12 x at the least. Wall time of the file: 5.5 s for its 50 tests.
"""
import numpy as np
import pytest
import torch

import ragged_ref as R
from ragged_ref import C
from util import to_np

pytestmark = pytest.mark.gpu

CASES = R.train_cases()
BURSTS = R.burst_cases()
IDS = [d["name"] for d in CASES]
BURST_IDS = [b["name"] + "-" + form for form, b in BURSTS]
SENTINEL = 0x7FC0BEEF                     # a quiet NaN no kernel computes: rows a kernel must leave alone keep it bit for bit
WORST = {}                                # name -> worst measured ratio (read by whoever runs this module to record it)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _record(tag, per):
    for k, v in per.items():
        WORST[f"{tag}.{k}"] = max(WORST.get(f"{tag}.{k}", 0.0), v)


_REF = {}                                 # the float64 values are computed once and shared (the tail tests run every case at two widths)


def _candidates(d, form, bg_ray=True):
    key = (d["name"], form, bg_ray)
    if key not in _REF:
        vals, mags, fwd = R.evaluate(d, form, None, bg_ray=bg_ray, mags=True)
        _REF[key] = R.stop_candidates(fwd, mags, d["T_thresh"]), fwd["L"]
    return _REF[key]


def _want(d, form, on, bg_ray=True):
    """stops -> (values, magnitudes) of the reference, kept per stop."""
    def fn(stops):
        key = (d["name"], form, bg_ray, on, tuple(int(x) for x in stops))
        if key not in _REF:
            _REF[key] = R.evaluate(d, form, stops, on=on, bg_ray=bg_ray, mags=True)[:2]
        return _REF[key]
    return fn


def test_undecided_cap_on_the_reference():
    for d in CASES:
        for form in ("composite", "tail"):
            cands, _ = _candidates(d, form)
            n = sum(len(c) > 1 for c in cands)
            assert n <= 0.02 * d["N"] and ("stops" not in d or n == 0), (d["name"], form, n)
    for form, b in BURSTS:
        ref = R.burst(*R.burst_args(b))
        m = R.burst_magnitudes(b["n_step"], *R.burst_args(b)[2:])
        cands = R.burst_candidates(b["n_step"], b["T_thresh"], b["deltas"], ref["T"], m["T"])
        assert sum(len(c) > 1 for c, l in zip(cands, ref["listed"]) if l) <= 0.02 * ref["listed"].sum(), b["name"]


def _inside(L, M, upto=None):
    """[M] bool: the rows of rays that fit (upto [N]: only the samples <= upto of each)."""
    keep = L["valid"] if upto is None else L["valid"] & (L["col"] <= np.asarray(upto)[:, None])
    m = np.zeros(M, bool)
    m[L["rows"][keep]] = True
    return m


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_composite_train_kernels_against_float64(d):
    """foc_composite_rays_train_forward / _backward: weights_sum, depth, image; grad_sigmas and grad_rgbs on the active rows for grad_image
    alone (grad_weights_sum = NULL), grad_weights_sum alone, and both; the rows behind a stop, of rays that do not fit and of the pad keep
    the sentinel they were filled with bit for bit."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    N, M, thr = d["N"], d["M"], d["T_thresh"]
    sig, rgb = R.composite_inputs(d)
    st, rt, dt, yt = _cuda(sig), _cuda(rgb), _cuda(d["deltas"]), _cuda(d["rays"])
    ws, dp, im = _nan(N), _nan(N), _nan(N, 3)
    check(lib.foc_composite_rays_train_forward(ptr(st), ptr(rt), ptr(dt), ptr(yt), M, N, thr, ptr(ws), ptr(dp), ptr(im), stream_of(st)), "train_forward")
    cands, L = _candidates(d, "composite")
    fwd_got = dict(weights_sum=R.by_list(L, to_np(ws)), depth=R.by_list(L, to_np(dp)), image=R.by_list(L, to_np(im)))
    for on in R.combos("composite"):
        g = R.grads_of(d, on, "composite")
        gi = _cuda(g["grad_image"])
        gw = _cuda(g["grad_ws"]) if g["grad_ws"] is not None else None
        gs = torch.full((M,), SENTINEL, dtype=torch.int32, device="cuda")
        gc = torch.full((M, 3), SENTINEL, dtype=torch.int32, device="cuda")
        check(lib.foc_composite_rays_train_backward(ptr(gw), ptr(gi), ptr(st), ptr(rt), ptr(dt), ptr(yt), ptr(ws), ptr(im), M, N, thr, ptr(gs), ptr(gc),
                                                    stream_of(st)), "train_backward")
        gs_b, gc_b = to_np(gs), to_np(gc)
        wrote_s, wrote_c = gs_b != SENTINEL, (gc_b != SENTINEL).all(1)
        assert np.array_equal(wrote_s, wrote_c) and np.array_equal(wrote_c, (gc_b != SENTINEL).any(1))
        got = dict(fwd_got, grad_sigma=R.gather(L, np.where(wrote_s, gs_b.view(np.float32), 0)),
                   grad_rgb=R.gather(L, np.where(wrote_c[:, None], gc_b.view(np.float32), 0)))
        best, chosen, per = R.match(cands, _want(d, "composite", on), got, L, half=())
        _record("train", per)
        assert best.max() <= C, (on, per, np.argmax(best))
        assert np.array_equal(wrote_s, _inside(L, M, chosen)), "rows written: exactly the samples up to the stop of the rays that fit"


@pytest.mark.parametrize("c_width", [4, 16])
@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_tail_kernels_against_float64(d, c_width):
    """foc_occ_tail_forward / _backward and the _sumsq twins at the case's density_scale (1 or 2), with a per-ray and a scalar background:
    weights_sum, image_raw, image, depth (both forwards), ray_sumsq; grad_h0 and grad_c for each incoming term alone (grad_ws = NULL where
    it is absent; the criterion term through the _sumsq backward) and all together. Every row of grad_c / grad_h0 is written from a NaN
    prefill: zeros outside the rays that fit and in the pad columns, behind a stop the criterion term alone."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    N, M, thr, ds = d["N"], d["M"], d["T_thresh"], d["density_scale"]
    rng = np.random.default_rng(5)
    h = rng.normal(0, 1, (M, 16)).astype(np.float16)                     # columns 1..15 are not the tail's to read
    h[:, 0] = d["h0"]
    c = (rng.normal(0, 1, (M, c_width)) * 30).astype(np.float16)        # pad columns: whatever the colour network left there
    c[:, :3] = d["c"]
    ht, ct, dt, yt = _cuda(h), _cuda(c), _cuda(d["deltas"]), _cuda(d["rays"])
    nt, ft = _cuda(d["nears"]), _cuda(d["fars"])
    counter = torch.tensor([d["total"], N], dtype=torch.int32, device="cuda")
    for bg_ray in (True, False):
        bt = _cuda(d["bg"]) if bg_ray else None
        cands, L = _candidates(d, "tail", bg_ray)
        outs = []
        for crit in (False, True):
            o = dict(weights_sum=_nan(N), image_raw=_nan(N, 3), image=_nan(N, 3), depth=_nan(N))
            args = (ptr(ht), ptr(ct), c_width, ptr(dt), ptr(yt), M, N, thr, ds, ptr(bt), R.BG_SCALAR, ptr(nt), ptr(ft), ptr(o["weights_sum"]),
                    ptr(o["image_raw"]), ptr(o["image"]), ptr(o["depth"]))
            if crit:
                o["sumsq"] = _nan(N)
                check(lib.foc_occ_tail_forward_sumsq(*args, ptr(o["sumsq"]), stream_of(ht)), "tail_forward_sumsq")
            else:
                check(lib.foc_occ_tail_forward(*args, stream_of(ht)), "tail_forward")
            outs.append(o)
        for k in ("weights_sum", "image_raw", "image", "depth"):
            assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), f"the twins' {k}"
        o = outs[1]
        fwd_got = {k: R.by_list(L, to_np(v)) for k, v in o.items()}
        for on in R.combos("tail"):
            g = R.grads_of(d, on, "tail")
            gi = _cuda(g["grad_image"])
            gw = _cuda(g["grad_ws"]) if g["grad_ws"] is not None else None
            gq = _cuda(g["grad_sumsq"]) if g["grad_sumsq"] is not None else None
            grad_c, grad_h0 = _nan(M, c_width, dtype=torch.float16), _nan(M, dtype=torch.float16)
            args = (ptr(gi), ptr(gw), ptr(ht), ptr(ct), c_width, ptr(dt), ptr(yt), ptr(counter), ptr(o["weights_sum"]), ptr(o["image_raw"]), M, N, thr, ds,
                    ptr(bt), R.BG_SCALAR, ptr(grad_c), ptr(grad_h0))
            if gq is not None:
                check(lib.foc_occ_tail_backward_sumsq(*args, ptr(gq), stream_of(ht)), "tail_backward_sumsq")
            else:
                check(lib.foc_occ_tail_backward(*args, stream_of(ht)), "tail_backward")
            gc, gh = to_np(grad_c).astype(np.float64), to_np(grad_h0).astype(np.float64)
            assert not np.isnan(gc).any() and not np.isnan(gh).any(), "every row is written"
            assert not gc[:, 3:].any(), "pad columns of grad_c"
            out = ~_inside(L, M)
            assert not gc[out].any() and not gh[out].any(), "rows of rays that do not fit and of the pad"
            got = dict(fwd_got, grad_h0=R.gather(L, gh), grad_c=R.gather(L, gc[:, :3]))
            best, chosen, per = R.match(cands, _want(d, "tail", on, bg_ray), got, L)
            _record("tail", per)
            assert best.max() <= C, (bg_ray, on, per, np.argmax(best))
            behind = _inside(L, M) & ~_inside(L, M, chosen)
            assert not gc[behind].any(), "behind a stop no colour gradient"
            if g["grad_sumsq"] is None:
                assert not gh[behind].any(), "behind a stop only the criterion term remains"


@pytest.mark.parametrize("fb", BURSTS, ids=BURST_IDS)
def test_inference_burst_against_float64(fb):
    """foc_composite_rays on 16-byte aligned arrays (the register-resident kernels at 4, 8, 16 slots) and on arrays 4 bytes off (the
    pointer-walking kernel), foc_composite_compact on sample-major arrays: weights_sum, depth, image and a survivor's rays_t within the
    bound, the kill decision float64's on every decided row, a dead ray's rays_t and every accumulator outside the list bit for bit
    untouched; the compacted list is the survivors in order."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    form, b = fb
    n, s, thr = b["n_alive"], b["n_step"], b["T_thresh"]
    sig, rgb, dl = b["sigmas"], b["rgbs"].reshape(-1), b["deltas"].reshape(-1)
    if form == "compact":                                                 # [n_step][n_alive]
        sig = sig.reshape(n, s).T.reshape(-1)
        rgb = rgb.reshape(n, s, 3).transpose(1, 0, 2).reshape(-1)
        dl = dl.reshape(n, s, 2).transpose(1, 0, 2).reshape(-1)
    off = 1 if form == "offset" else 0

    def place(a):
        buf = torch.zeros(a.size + off, device="cuda")
        buf[off:] = _cuda(a)
        return buf, buf[off:]

    (sb, st), (rb, rt), (db, dt) = place(sig), place(rgb), place(dl)
    assert all((x.data_ptr() % 16 == 0) == (off == 0) for x in (st, rt, dt))
    alive, t = _cuda(b["rays_alive"]), _cuda(b["rays_t"])
    ws, dp, im = _cuda(b["weights_sum"]), _cuda(b["depth"]), _cuda(b["image"])
    if form == "compact":
        out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
        blocks = torch.zeros(n // 1024 + 2, dtype=torch.int32, device="cuda")
        check(lib.foc_composite_compact(n, s, thr, ptr(alive), ptr(t), ptr(st), ptr(rt), ptr(dt), ptr(ws), ptr(dp), ptr(im), ptr(out), ptr(n_out), ptr(blocks),
                                        None, 0, 1, 1, stream_of(st)), "composite_compact")
    else:
        check(lib.foc_composite_rays(n, s, thr, ptr(alive), ptr(t), ptr(st), ptr(rt), ptr(dt), ptr(ws), ptr(dp), ptr(im), stream_of(st)), "composite_rays")
    got = dict(rays_alive=to_np(alive), rays_t=to_np(t), weights_sum=to_np(ws), depth=to_np(dp), image=to_np(im))
    best, per, _ = R.burst_match(b, got)
    _record("burst", per)
    assert best.max() <= C, (per, np.argmax(best))
    untouched = np.ones(b["n_rays"], bool)
    untouched[b["rays_alive"][b["rays_alive"] >= 0]] = False
    for k in ("rays_t", "weights_sum", "depth", "image"):
        assert np.array_equal(got[k][untouched].view(np.uint32), b[k][untouched].view(np.uint32)), f"{k} of rays outside the list"
    assert (got["rays_alive"][b["rays_alive"] < 0] == -1).all()
    if form == "compact":
        kept = got["rays_alive"][got["rays_alive"] >= 0]
        assert int(n_out) == kept.size and np.array_equal(to_np(out)[:kept.size], kept)
