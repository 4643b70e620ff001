"""CPU: tests/attribution_ref.py (the float64 statement of per-object attribution, include/focnerf.h foc_combine_select_composite_attr)
pinned against what exists — the oracle's select and composite — and the host-side refusals of the two new entry points.
The tolerance is 1e-4 absolute, the project's own for composited quantities (tests/test_gpu_combine.py)."""
import ctypes

import numpy as np
import pytest

import oracle
import attribution_ref as ar

ATOL = 1e-4


def _oracle_select(dens, rgb):
    m, b = dens[0].copy(), rgb[0].copy()
    for k in range(1, dens.shape[0]):
        m, b = oracle.combine_select(dens[k], rgb[k], m, b)
    return m.reshape(dens.shape[1:]), b.reshape(rgb.shape[1:])


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("K,N,T", [(1, 5, 2), (2, 37, 64), (4, 33, 65), (16, 9, 40)])
def test_rgb_of_the_winner_is_the_oracles_best_rgb(K, N, T):
    dens, rgb, nears, fars = ar.fields(K, N, T, 7 + K)
    win, src, merged = ar.winner(dens)
    m, best = _oracle_select(dens, rgb)
    assert np.array_equal(win, src.astype(np.uint8))                      # field k is object k
    assert _same_bits(np.take_along_axis(rgb, src[None, ..., None], 0)[0], best) and _same_bits(merged, m)
    if K > 1:
        assert (win[:, :8] != 1).all() and (dens[1, :, :8] == dens[0, :, :8]).all()      # exact ties: the later object never takes one
    assert (win[ar.empty_rays(N)] == 0).all()                             # an empty ray is all ties at 0: object 0's


def test_winner_on_ties_signed_zeros_infinities_and_nan():
    """One sample per column, three objects. Column by column: tie at 0; non-zero tie; -0.0 against +0.0 (equal: no take) and the reverse;
    inf beats finite, a second inf ties; NaN in the incoming field never takes; NaN in the running max blocks every later object."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    d0 = np.array([0.0, 2.5, -0.0, 0.0, 1.0, inf, 1.0, nan, 3.0, -inf], np.float32)
    d1 = np.array([0.0, 2.5, 0.0, -0.0, inf, inf, nan, 9.0, nan, 0.0], np.float32)
    d2 = np.array([0.0, 2.5, 1e-30, 0.0, inf, 1.0, 2.0, 9.0, 4.0, nan], np.float32)
    dens = np.stack([d0, d1, d2])[:, None, :]                             # [3, 1, 10]
    rng = np.random.default_rng(0)
    rgb = rng.random((3, 1, 10, 3)).astype(np.float32)
    win, src, merged = ar.winner(dens)
    assert win[0].tolist() == [0, 0, 2, 0, 1, 0, 0, 0, 0, 1]
    m, best = _oracle_select(dens, rgb)
    assert _same_bits(np.take_along_axis(rgb, src[None, ..., None], 0)[0], best)
    assert np.array_equal(np.isnan(merged), np.isnan(m)) and _same_bits(merged[~np.isnan(m)], m[~np.isnan(m)])
    # ids: constants other than the position, and a plane
    plane = np.full((1, 10), 7, np.uint8)
    plane[0, 4] = 5
    win2, _, _ = ar.winner(dens, ids=[3, plane, 1])
    assert win2[0].tolist() == [3, 3, 1, 3, 5, 3, 3, 3, 3, 7]


@pytest.mark.parametrize("K,N,T", [(1, 5, 2), (3, 40, 65), (4, 64, 130), (8, 33, 512)])
def test_column_sums_are_the_oracles_composite(K, N, T):
    dens, rgb, nears, fars = ar.fields(K, N, T, 20 + K)
    ref = ar.attribution(dens, nears, fars, K)
    m, best = _oracle_select(dens, rgb)
    _, depth, w = oracle.composite_fixed_steps(m, best, nears, fars, 1.0, clamp01=True, want_weights=True)
    np.testing.assert_allclose(ref.weights, w, atol=ATOL, rtol=0)
    np.testing.assert_allclose(ref.obj_depth.sum(axis=1), depth, atol=ATOL, rtol=0)
    # zero rgb over a white background: what is not background is the sum of the mattes
    img, _ = oracle.composite_fixed_steps(m, np.zeros_like(best), nears, fars, 1.0, clamp01=True)
    np.testing.assert_allclose(ref.obj_weights.sum(axis=1), 1.0 - img[:, 0], atol=ATOL, rtol=0)
    # columns are disjoint: every sample's weight sits in its winner's column and nowhere else
    for k in range(K):
        assert np.array_equal(ref.obj_weights[:, k], np.where(ref.winner == k, ref.weights, 0.0).sum(axis=1))
    empty = ar.empty_rays(N)
    assert (ref.obj_weights[empty] == 0).all() and (ref.instance[empty] == -1).all() and (ref.instance[~empty] >= 0).any()
    assert np.array_equal(ref.instance, np.where(ref.obj_weights.max(axis=1) > 0, np.argmax(ref.obj_weights, axis=1), -1))


def test_instance_rules():
    nan = np.nan
    w = np.array([[0.0, 0.0, 0.0], [0.2, 0.5, 0.5], [nan, 0.1, 0.0], [nan, nan, nan], [0.0, -0.0, 1e-30], [nan, 0.0, 0.0]])
    assert ar.instance_of(w).tolist() == [-1, 1, 1, -1, 2, -1]
    assert ar.top_two_gap(np.array([[0.2, 0.5, 0.45], [0.0, 0.0, 0.3]])).round(6).tolist() == [0.05, 0.3]


def test_out_of_range_plane_ids_count_nowhere():
    dens, rgb, nears, fars = ar.fields(2, 12, 16, 3)
    plane = np.ones((12, 16), np.uint8)
    plane[:, ::3] = 9
    ref = ar.attribution(dens, nears, fars, 2, ids=[0, plane])
    base = ar.attribution(dens, nears, fars, 2)
    lost = np.where((base.winner == 1) & (plane == 9), base.weights, 0.0).sum(axis=1)
    assert np.array_equal(ref.obj_weights[:, 0], base.obj_weights[:, 0])
    np.testing.assert_allclose(ref.obj_weights[:, 1], base.obj_weights[:, 1] - lost, atol=1e-12, rtol=0)
    assert lost.max() > 0 and ref.instance.max() <= 1


# ------------------------------------------------------------------------------------------------ the library's refusals, no device
def test_attribution_entry_points_refuse_bad_arguments_on_the_host():
    """foc_combine_select_composite_attr / foc_combine_select4_ids through ctypes: every refusal is rc 1 (FOC_E_INVALID) with a message
    naming the argument, before anything touches a device. Pointers that validation never dereferences are small fake addresses."""
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)
    bgs = (ctypes.c_float * 2)(1.0, 0.0)

    def call(K=2, n_obj=4, ids=(0, 1), T=8, N=4, fields=None, outs=(one, one, one), planes=None):
        n = max(K, 1)
        f = (ctypes.c_void_p * n)(*(fields or [16 * (k + 1) for k in range(n)]))
        cid = (ctypes.c_uint32 * n)(*(list(ids) + [0] * n)[:n])
        return lib.foc_combine_select_composite_attr(f, K, planes, cid, n_obj, one, one, N, T, bgs, 2, one, one, None, outs[0], outs[1], outs[2], None, None)

    for kw, word in ((dict(n_obj=17), b"n_obj"), (dict(n_obj=0), b"n_obj"), (dict(K=0), b"K"), (dict(K=17), b"K"), (dict(ids=(0, 4)), b"ids[1]"),
                     (dict(n_obj=2, ids=(2, 0)), b"ids[0]"), (dict(T=1), b"T must be >= 2"), (dict(outs=(None, one, one)), b"obj_weights"),
                     (dict(outs=(one, None, one)), b"obj_depth"), (dict(outs=(one, one, None)), b"instance"), (dict(fields=[16, 40]), b"field 1")):
        assert call(**kw) == 1, kw
        assert word in lib.foc_last_error(), (kw, lib.foc_last_error())
    assert call(N=0) == 0 and call(N=0, outs=(None, None, None)) == 0            # an empty chunk: nothing to do, nothing to refuse
    # a field with an id plane needs no constant id; one without either is refused
    planes = (ctypes.c_void_p * 2)(64, None)
    assert lib.foc_combine_select_composite_attr((ctypes.c_void_p * 2)(16, 32), 2, planes, None, 4, one, one, 0, 8, bgs, 2, one, one, None, one, one, one,
                                                 None, None) == 1
    assert b"neither an id plane nor a constant id" in lib.foc_last_error()
    assert lib.foc_combine_select4_ids(one, 16, one, one, 8, None) == 1 and b"id 16" in lib.foc_last_error()
    assert lib.foc_combine_select4_ids(one, 3, one, None, 8, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_combine_select4_ids(one, 3, ctypes.c_void_p(20), one, 8, None) == 1 and b"16-byte aligned" in lib.foc_last_error()
    assert lib.foc_combine_select4_ids(None, 3, None, None, 0, None) == 0


def test_python_layer_refuses_before_any_launch():
    import torch
    from focnerf_amd import Attribution
    from focnerf_amd.combine import ObjectCombiner, combine_packed
    assert Attribution._fields == ("weights", "depth", "instance")

    class NoOps:                                        # any call into the ops would be an AttributeError
        pass
    f = [torch.zeros(2, 4, 4) for _ in range(17)]
    with pytest.raises(ValueError, match="at most 16"):
        combine_packed(f, torch.ones(2), torch.full((2,), 2.0), attribution=True, ops=NoOps)
    comb = ObjectCombiner(rank=0, world_size=1, ops=NoOps)
    fns = [lambda lo, hi, out: torch.zeros(hi - lo, 4, 4)] * 2
    for att in ((0, 17), (3, 4), (0, 1), (-1, 4)):
        with pytest.raises(ValueError, match="attribution"):
            comb.render_view(fns, 2, torch.ones(2), torch.full((2,), 2.0), 4, attribution=att)
