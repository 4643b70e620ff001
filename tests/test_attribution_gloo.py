"""CPU, world_size 2 and 4 over gloo: `ObjectCombiner.render_view(attribution=(first_object, n_objects))` (focnerf_amd/combine.py) — the id
plane built per piece, its uint8 all-to-all beside the field's, one plane per received field on the owner of a ray slice, the extended
gather — against the single-process statement on the same fields, bit for bit (the same CPU functions see the same rows). The device
kernels are replaced by CPU ops DEFINED HERE: tests/test_combine_gloo.py's oracle-backed ops plus the two new methods on
tests/attribution_ref.py. Without the keyword the combiner must reach none of the new methods and send not one byte more."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import attribution_ref as ar
from test_combine_gloo import CpuOps, _free_port, _init, _packed

K, N, T, CHUNK, BGS = 4, 37, 16, 16, (1.0, 0.0)          # pieces of 16, 16 and 5 rays: the last is ragged, and at world 4 one rank owns none of it


class CpuAttrOps(CpuOps):
    @staticmethod
    def select4_ids(field4, obj_id, acc4, acc_ids):
        with np.errstate(invalid="ignore"):
            take = field4.numpy()[..., 0] > acc4.numpy()[..., 0]
        CpuOps.select4(field4, acc4)
        acc_ids.numpy()[take] = obj_id

    @staticmethod
    def select_composite_attr(fields4, nears, fars, bgs, n_obj, ids=None, want_merged=False, want_winner=False):
        from focnerf_amd.combine import Attribution
        image4, depth, merged = CpuOps.select_composite(fields4, nears, fars, bgs, want_merged=True)
        ids = list(range(len(fields4))) if ids is None else [i.numpy() if torch.is_tensor(i) else i for i in ids]
        ref = ar.attribution(np.stack([f.numpy()[..., 0] for f in fields4]), nears.numpy(), fars.numpy(), n_obj, ids)
        att = Attribution(torch.from_numpy(ref.obj_weights.astype(np.float32)), torch.from_numpy(ref.obj_depth.astype(np.float32)),
                          torch.from_numpy(ref.instance.astype(np.int32)))
        return image4, depth, att, merged if want_merged else None, torch.from_numpy(ref.winner) if want_winner else None


def _view():
    dens, rgb, nears, fars = ar.fields(K, N, T, 3)
    return [_packed(dens[k], rgb[k]) for k in range(K)], torch.from_numpy(nears), torch.from_numpy(fars)


def _worker(rank, world, port, overlap, out_dir):
    _init(rank, world, port)
    from focnerf_amd.combine import Attribution, ObjectCombiner
    fields, nears, fars = _view()
    per_rank = K // world
    mine = list(range(rank * per_rank, (rank + 1) * per_rank))
    fns = [lambda lo, hi, out, f4=fields[k]: f4[lo:hi].clone() for k in mine]
    comb = ObjectCombiner(ops=CpuAttrOps)
    img, dep, att = comb.render_view(fns, N, nears, fars, T, bgs=BGS, max_ray_batch=CHUNK, overlap=overlap, attribution=(mine[0], K))
    assert isinstance(att, Attribution) and att.instance.dtype == torch.int32
    sent_attr = comb.bytes_sent
    plain = ObjectCombiner(ops=CpuOps)                                   # today's ops only: the default path may call nothing else
    pair = plain.render_view(fns, N, nears, fars, T, bgs=BGS, max_ray_batch=CHUNK, overlap=overlap)
    assert isinstance(pair, tuple) and len(pair) == 2
    np.savez(os.path.join(out_dir, f"a{rank}.npz"), img=img.numpy(), dep=dep.numpy(), w=att.weights.numpy(), z=att.depth.numpy(), inst=att.instance.numpy(),
             img_plain=pair[0].numpy(), dep_plain=pair[1].numpy(), sent_attr=np.int64(sent_attr), sent_plain=np.int64(plain.bytes_sent))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("overlap", [True, False])
def test_render_view_attribution_equals_the_single_process_reference(tmp_path, world, overlap):
    mp.spawn(_worker, args=(world, _free_port(), overlap, str(tmp_path)), nprocs=world, join=True)
    fields, nears, fars = _view()
    img_s, dep_s, att_s, _, win_s = CpuAttrOps.select_composite_attr(fields, nears, fars, BGS, K, want_winner=True)
    assert set(np.unique(win_s.numpy())) == {0, 1, 2, 3} and (att_s.instance == -1).any() and len(np.unique(att_s.instance.numpy())) >= 4
    # what leaves a rank: per piece (p-1) slices of 16 B per sample, per view (p-1) copies of its flat buffer (exchange_start, _render_view)
    pieces = [min(CHUNK, N - lo) for lo in range(0, N, CHUNK)]
    pers = [-(-n // world) for n in pieces]
    per = pers[0]
    fields_bytes = sum((world - 1) * p * T * 16 for p in pers)
    gather_plain = (world - 1) * 4 * len(pieces) * per * (len(BGS) * 4 + 1)
    ids_bytes = sum((world - 1) * p * T for p in pers)
    gather_attr = (world - 1) * 4 * len(pieces) * per * (2 * K + 1)
    for r in range(world):
        g = np.load(os.path.join(tmp_path, f"a{r}.npz"))
        assert g["w"].shape == (N, K) and g["z"].shape == (N, K) and g["inst"].shape == (N,) and g["inst"].dtype == np.int32
        for name, want in (("img", img_s), ("dep", dep_s), ("w", att_s.weights), ("z", att_s.depth), ("inst", att_s.instance),
                           ("img_plain", img_s), ("dep_plain", dep_s)):
            assert np.array_equal(g[name].view(np.uint32), want.numpy().view(np.uint32)), f"rank {r}: {name} differs from the single-process reference"
        assert int(g["sent_plain"]) == fields_bytes + gather_plain
        assert int(g["sent_attr"]) == fields_bytes + gather_plain + ids_bytes + gather_attr


def test_one_rank_with_and_without_its_collectives(tmp_path):
    """World 1: no exchange and the plane used directly; with `collectives_at_world_1` both all-to-alls and the extended gather run (the
    switch tests/test_gpu_attribution.py uses to rehearse the RCCL path on one GPU). Same bits either way, nothing on the wire."""
    mp.spawn(_one_rank_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    g = np.load(os.path.join(tmp_path, "one.npz"))
    fields, nears, fars = _view()
    img_s, dep_s, att_s, _, _ = CpuAttrOps.select_composite_attr(fields[:3], nears, fars, BGS, 3)
    for name in ("plain", "forced"):
        for key, want in (("img", img_s), ("dep", dep_s), ("w", att_s.weights), ("z", att_s.depth), ("inst", att_s.instance)):
            assert np.array_equal(g[f"{name}_{key}"].view(np.uint32), want.numpy().view(np.uint32)), (name, key)


def _one_rank_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    from focnerf_amd.combine import ObjectCombiner
    fields, nears, fars = _view()
    fns = [lambda lo, hi, out, f4=fields[k]: f4[lo:hi].clone() for k in range(3)]
    res = {}
    for name, comb in (("plain", ObjectCombiner(ops=CpuAttrOps)), ("forced", ObjectCombiner(ops=CpuAttrOps, collectives_at_world_1=True))):
        img, dep, att = comb.render_view(fns, N, nears, fars, T, bgs=BGS, max_ray_batch=CHUNK, attribution=(0, 3))
        assert comb.bytes_sent == 0
        res.update({f"{name}_img": img.numpy(), f"{name}_dep": dep.numpy(), f"{name}_w": att.weights.numpy(), f"{name}_z": att.depth.numpy(),
                    f"{name}_inst": att.instance.numpy()})
    np.savez(os.path.join(out_dir, "one.npz"), **res)
    dist.destroy_process_group()
