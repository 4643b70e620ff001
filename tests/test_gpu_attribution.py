"""GPU: per-object attribution of the combined render (csrc/combine.hip k_combine_select_composite_attr / k_combine_select4_ids,
include/focnerf.h) against the float64 statement in tests/attribution_ref.py and against the kernel it extends.

Shapes (K, N, T): (1, 5, 2) the minimum T and N not a multiple of the 4 rays per workgroup; (2, 37, 64) / (3, 4, 65) either side of the
64-sample pass; (4, 257, 130) general; (16, 64, 65) the object limit and the widest instantiation; (8, 130, 512) the workload's T and the
middle instantiation. Fields: tests/test_gpu_combine.py's generator (half the densities exactly 0, exact non-zero ties) with a third
of the rays thinned by 0.01 and every eleventh ray empty. Tolerance 1e-4 absolute: the project's for this kernel's composited outputs."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import attribution_ref as ar
from util import to_np

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 5, 2), (2, 37, 64), (3, 4, 65), (4, 257, 130), (16, 64, 65), (8, 130, 512)]
SEED = 100          # with it the rays left out of the instance comparison are 0 - 0.4 % per shape (float64 reference alone, checked on the CPU)
ATOL = 1e-4


@functools.lru_cache(maxsize=None)
def _case(K, N, T):
    """(dens, rgb, nears, fars, reference) of a shape: computed once, shared by every test, never written to."""
    dens, rgb, nears, fars = ar.fields(K, N, T, SEED)
    return dens, rgb, nears, fars, ar.attribution(dens, nears, fars, K)


def _pack(dens, rgb):
    return torch.from_numpy(np.concatenate([dens[..., None], rgb], -1).astype(np.float32)).cuda().contiguous()


def _device(K, N, T):
    dens, rgb, nears, fars, _ = _case(K, N, T)
    return [_pack(dens[k], rgb[k]) for k in range(K)], torch.from_numpy(nears).cuda(), torch.from_numpy(fars).cuda()


def _bits(a, b):
    """Bit for bit, NaN payloads and signed zeros included."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _attr(fields, nr, fr, n_obj, bgs=(1.0, 0.0), **kw):
    from focnerf_amd.combine import HipCombineOps
    return HipCombineOps.select_composite_attr(fields, nr, fr, bgs, n_obj, **kw)


@pytest.mark.parametrize("K,N,T", SHAPES)
def test_image_depth_and_merged_are_those_of_select_composite(K, N, T):
    from focnerf_amd.combine import HipCombineOps
    fields, nr, fr = _device(K, N, T)
    for bgs in ((1.0, 0.0), (0.25,)):
        i0, d0, m0 = HipCombineOps.select_composite(fields, nr, fr, bgs, want_merged=True)
        i1, d1, att, m1, _ = _attr(fields, nr, fr, K, bgs, want_merged=True)
        assert _bits(i1, i0) and _bits(d1, d0) and _bits(m1, m0), bgs
        i2, d2, att2, m2, w2 = _attr(fields, nr, fr, K, bgs)                   # the optional outputs left out: same bits
        assert m2 is None and w2 is None and _bits(i2, i0) and _bits(d2, d0)
        assert all(_bits(a, b) for a, b in zip(att, att2))
        assert att.weights.shape == (N, K) and att.depth.shape == (N, K) and att.instance.shape == (N,) and att.instance.dtype == torch.int32


@pytest.mark.parametrize("K,N,T", SHAPES)
def test_winner_is_the_references_and_carries_the_merged_rgb(K, N, T):
    dens, rgb, _, _, ref = _case(K, N, T)
    fields, nr, fr = _device(K, N, T)
    _, _, _, merged, winner = _attr(fields, nr, fr, K, want_merged=True, want_winner=True)
    assert winner.dtype == torch.uint8 and np.array_equal(to_np(winner), ref.winner)
    own = torch.stack(fields)[..., 1:].gather(0, winner.long()[None, ..., None].expand(1, N, T, 3))[0]
    assert _bits(merged[..., 1:].contiguous(), own.contiguous())


def test_winner_on_signed_zeros_infinities_and_nan():
    """Three objects, ten samples of one ray (tests/test_attribution_ref.py walks the same columns): tie at 0, non-zero tie, -0.0 / +0.0,
    inf against finite and inf, NaN in the incoming field (never takes), NaN in the running max (nothing takes it afterwards)."""
    nan, inf = float("nan"), float("inf")
    d = np.array([[0.0, 2.5, -0.0, 0.0, 1.0, inf, 1.0, nan, 3.0, -inf],
                  [0.0, 2.5, 0.0, -0.0, inf, inf, nan, 9.0, nan, 0.0],
                  [0.0, 2.5, 1e-30, 0.0, inf, 1.0, 2.0, 9.0, 4.0, nan]], np.float32)[:, None, :]
    rgb = np.random.default_rng(0).random((3, 1, 10, 3)).astype(np.float32)
    fields = [_pack(d[k], rgb[k]) for k in range(3)]
    nr, fr = torch.full((1,), 0.2, device="cuda"), torch.full((1,), 2.0, device="cuda")
    _, _, att, merged, winner = _attr(fields, nr, fr, 3, want_merged=True, want_winner=True)
    want, src, _ = ar.winner(d)
    assert to_np(winner)[0].tolist() == want[0].tolist() == [0, 0, 2, 0, 1, 0, 0, 0, 0, 1]
    assert _bits(merged[0, :, 1:].contiguous(), torch.from_numpy(np.take_along_axis(rgb, src[None, ..., None], 0)[0, 0]).cuda())
    assert int(att.instance[0]) in (-1, 0, 1, 2)                              # NaN weights downstream of the NaN sample: any column, never out of range
    plane = torch.full((1, 10), 7, dtype=torch.uint8, device="cuda")
    plane[0, 4] = 5
    _, _, _, _, w2 = _attr(fields, nr, fr, 8, ids=[3, plane, 1], want_winner=True)
    assert to_np(w2)[0].tolist() == [3, 3, 1, 3, 5, 3, 3, 3, 3, 7]


@pytest.mark.parametrize("K,N,T", SHAPES)
def test_mattes_and_depths_against_the_float64_reference(K, N, T):
    _, _, _, _, ref = _case(K, N, T)
    fields, nr, fr = _device(K, N, T)
    _, depth, att, _, _ = _attr(fields, nr, fr, K)
    w, z = to_np(att.weights).astype(np.float64), to_np(att.depth).astype(np.float64)
    print(f"({K},{N},{T}) max |obj_weights - ref| {np.abs(w - ref.obj_weights).max():.3e}  max |obj_depth - ref| {np.abs(z - ref.obj_depth).max():.3e}")
    np.testing.assert_allclose(w, ref.obj_weights, atol=ATOL, rtol=0)
    np.testing.assert_allclose(z, ref.obj_depth, atol=ATOL, rtol=0)
    never = ~(ref.winner[..., None] == np.arange(K)).any(axis=1)                # [N,K]: the object wins no sample of the ray
    assert (w[never] == 0).all() and (z[never] == 0).all() and never.any() == (K > 1)
    np.testing.assert_allclose(z.sum(axis=1), to_np(depth), atol=ATOL, rtol=0)  # rows sum to the composite's depth
    assert w.max() > 0.3 and (w.sum(axis=1) < 0.3).any()                        # dense and thin rays both present


@pytest.mark.parametrize("K,N,T", [s for s in SHAPES if s[0] > 1])
@pytest.mark.parametrize("last", [False, True])
def test_an_object_above_all_others_gets_the_one_object_columns_bit_for_bit(K, N, T, last):
    dens, rgb, _, _, _ = _case(K, N, T)
    _, nr, fr = _device(K, N, T)
    j = K - 1 if last else 0
    lifted = dens.copy()
    lifted[j] = dens.max(axis=0) + np.float32(1.0)                             # strictly above every object at every sample
    fields = [_pack(lifted[k], rgb[k]) for k in range(K)]
    i_all, d_all, att, _, winner = _attr(fields, nr, fr, K, want_winner=True)
    i_one, d_one, one, _, _ = _attr([fields[j]], nr, fr, 1)
    assert (winner == j).all() and _bits(i_all, i_one) and _bits(d_all, d_one)
    assert _bits(att.weights[:, j].contiguous(), one.weights[:, 0].contiguous()) and _bits(att.depth[:, j].contiguous(), one.depth[:, 0].contiguous())
    others = [k for k in range(K) if k != j]
    assert (att.weights[:, others] == 0).all() and (att.depth[:, others] == 0).all() and (att.instance == j).all()
    assert _bits(one.depth[:, 0].contiguous(), d_one)                          # one object: its column IS the composite's depth


@pytest.mark.parametrize("K,N,T", SHAPES)
def test_instance_is_the_first_argmax_of_the_kernels_own_mattes(K, N, T):
    dens, _, _, _, ref = _case(K, N, T)
    fields, nr, fr = _device(K, N, T)
    _, _, att, _, _ = _attr(fields, nr, fr, K)
    w, inst = to_np(att.weights), to_np(att.instance)
    positive = w.max(axis=1) > 0
    assert np.array_equal(inst, np.where(positive, np.argmax(w, axis=1), -1))
    empty = ~(dens > 0).any(axis=(0, 2))
    assert empty.any() and (w[empty] == 0).all() and (to_np(att.depth)[empty] == 0).all() and (inst[empty] == -1).all()
    # against the reference wherever its own decision is clear of the tolerance: top-two gap > 2 x 1e-4 (empty rays are exact: compared too)
    compared = (ar.top_two_gap(ref.obj_weights) > 2 * ATOL) | empty
    print(f"({K},{N},{T}) rays left out of the instance comparison: {int((~compared).sum())} of {N}")
    assert (~compared).mean() <= 0.02
    assert np.array_equal(inst[compared], ref.instance[compared])


def test_premerged_pairs_with_id_planes_equal_the_four_field_call():
    from focnerf_amd.combine import HipCombineOps
    K, N, T = 4, 257, 130
    fields, nr, fr = _device(K, N, T)
    want = _attr(fields, nr, fr, 4, want_merged=True, want_winner=True)
    accs, planes = [], []
    for a, b in ((0, 1), (2, 3)):
        acc, acc_plain = fields[a].clone(), fields[a].clone()
        plane = torch.full((N, T), a, dtype=torch.uint8, device="cuda")
        HipCombineOps.select4_ids(fields[b], b, acc, plane)
        HipCombineOps.select4(fields[b], acc_plain)
        assert _bits(acc, acc_plain) and set(torch.unique(plane).tolist()) == {a, b}
        accs.append(acc)
        planes.append(plane)
    got = _attr(accs, nr, fr, 4, ids=planes, want_merged=True, want_winner=True)
    assert _bits(got[0], want[0]) and _bits(got[1], want[1]) and _bits(got[3], want[3]) and _bits(got[4], want[4])
    assert all(_bits(a, b) for a, b in zip(got[2], want[2]))
    mixed = _attr([accs[0], fields[2], fields[3]], nr, fr, 4, ids=[planes[0], 2, 3], want_winner=True)      # planes and constants in one call
    assert _bits(mixed[0], want[0]) and _bits(mixed[4], want[4]) and all(_bits(a, b) for a, b in zip(mixed[2], want[2]))


def test_a_plane_id_beyond_n_obj_counts_in_no_column():
    """n_obj = 2 runs the four-column instantiation: id 3 lies past n_obj but inside the instantiation, 255 past both."""
    K, N, T = 2, 37, 64
    _, _, _, _, ref = _case(K, N, T)
    fields, nr, fr = _device(K, N, T)
    base = _attr(fields, nr, fr, 2, want_merged=True)
    bad = np.zeros((N, T), bool)
    bad[:, 1::5] = True
    plane = np.ones((N, T), np.uint8)
    plane[:, 1::5] = 3
    plane[:, 6::10] = 255
    got = _attr(fields, nr, fr, 2, ids=[0, torch.from_numpy(plane).cuda()], want_merged=True, want_winner=True)
    assert _bits(got[0], base[0]) and _bits(got[1], base[1]) and _bits(got[3], base[3])          # the render itself does not look at ids
    lost_w = np.where(bad & (ref.winner == 1), ref.weights, 0.0).sum(axis=1)
    assert lost_w.max() > 0.01
    assert _bits(got[2].weights[:, 0].contiguous(), base[2].weights[:, 0].contiguous()) and _bits(got[2].depth[:, 0].contiguous(), base[2].depth[:, 0].contiguous())
    np.testing.assert_allclose(to_np(got[2].weights[:, 1]), to_np(base[2].weights[:, 1]) - lost_w, atol=ATOL, rtol=0)
    w, inst = to_np(got[2].weights), to_np(got[2].instance)
    assert inst.max() <= 1 and np.array_equal(inst, np.where(w.max(axis=1) > 0, np.argmax(w, axis=1), -1))
    assert np.array_equal(to_np(got[4])[ref.winner == 1], plane[ref.winner == 1])                # `winner` reports the plane's byte as it is


def test_two_runs_give_the_same_bits_and_an_empty_chunk_gives_empty_tensors():
    K, N, T = 8, 130, 512
    fields, nr, fr = _device(K, N, T)
    a = _attr(fields, nr, fr, K, want_merged=True, want_winner=True)
    b = _attr(fields, nr, fr, K, want_merged=True, want_winner=True)
    assert _bits(a[0], b[0]) and _bits(a[1], b[1]) and _bits(a[3], b[3]) and _bits(a[4], b[4]) and all(_bits(x, y) for x, y in zip(a[2], b[2]))
    i4, d, att, _, _ = _attr([f[:0] for f in fields], nr[:0], fr[:0], K)
    assert i4.shape == (2, 0, 4) and d.shape == (0,) and att.weights.shape == (0, K) and att.depth.shape == (0, K) and att.instance.shape == (0,)
    with pytest.raises(RuntimeError, match="n_obj"):
        _attr(fields, nr, fr, 17)
    with pytest.raises(RuntimeError, match=r"ids\[7\]"):
        _attr(fields, nr, fr, 7)
    with pytest.raises(RuntimeError, match="uint8"):
        _attr(fields, nr, fr, K, ids=[torch.zeros(N, T, device="cuda")] + list(range(1, K)))


def test_object_combiner_on_one_rank_equals_combine_packed():
    from focnerf_amd.combine import Attribution, ObjectCombiner, combine_packed
    K, N, T = 3, 100, 48
    dens, rgb, nears, fars = ar.fields(K, N, T, SEED + 1)
    fields = [_pack(dens[k], rgb[k]) for k in range(K)]
    nr, fr = torch.from_numpy(nears).cuda(), torch.from_numpy(fars).cuda()

    def make(f4, into_out):
        def fn(lo, hi, out):
            if into_out and out is not None:
                out.copy_(f4[lo:hi])
                return out
            return f4[lo:hi].clone()
        return fn
    fns = [make(fields[k], k == 0) for k in range(K)]
    i_ref, d_ref, att_ref = combine_packed(fields, nr, fr, (1.0, 0.0), attribution=True)
    i_old, d_old = combine_packed(fields, nr, fr, (1.0, 0.0))
    assert isinstance(att_ref, Attribution) and _bits(i_ref, i_old) and _bits(d_ref, d_old)
    i_m, d_m, m_m, att_m = combine_packed(fields, nr, fr, (1.0, 0.0), want_merged=True, attribution=True)
    assert m_m.shape == (N, T, 4) and all(_bits(a, b) for a, b in zip(att_m, att_ref))
    comb = ObjectCombiner(rank=0, world_size=1)
    for overlap in (True, False):
        img, dep, att = comb.render_view(fns, N, nr, fr, T, bgs=(1.0, 0.0), max_ray_batch=48, overlap=overlap, attribution=(0, 3))   # pieces of 48, 48, 4
        assert _bits(img, i_ref) and _bits(dep, d_ref) and all(_bits(a, b) for a, b in zip(att, att_ref))
    pair = comb.render_view(fns, N, nr, fr, T, bgs=(1.0, 0.0), max_ray_batch=48)
    assert len(pair) == 2 and _bits(pair[0], i_old) and _bits(pair[1], d_old)
    assert len(set(att_ref.instance.tolist())) >= 3 and comb.bytes_sent == 0
    with pytest.raises(ValueError, match="at most 16"):
        combine_packed([fields[0]] * 17, nr, fr, attribution=True)


def test_one_rank_attribution_through_rccl():
    """tests/rccl_attr_worker.py as a fresh process: `render_view(attribution=...)` with `collectives_at_world_1=True`, so that both
    all-to-alls — the uint8 one included — and the extended gather go through RCCL on one GPU; bit for bit the exchange-free result."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "rccl_attr_worker.py")], env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    tail = (r.stdout + r.stderr)[-3000:]
    if r.returncode == 77:
        pytest.skip("the nccl (RCCL) process group could not be created on this box: " + tail[-400:])
    assert r.returncode == 0 and "RCCL_ATTR_OK backend nccl" in r.stdout, tail
