"""Worker of tests/test_gpu_attribution.py (NOT a test module), modelled on tests/rccl_one_rank_worker.py: ONE rank on cuda:0 with the `nccl`
backend (= RCCL on ROCm) and `ObjectCombiner(collectives_at_world_1=True)`, so that everything `render_view(attribution=...)` adds for
N > 1 goes through RCCL — the second `all_to_all_single` with the double-buffered uint8 [world*per, T] id planes beside the field's, and
the view's one `all_gather_into_tensor` extended by the mattes, their depths and the instance map (int32 bits carried as float32) —
and must leave the results of the exchange-free single-rank path, bit for bit. With one rank RCCL moves the data on the device itself:
this covers the binding (buffers, dtypes, split sizes), the ordering of RCCL's stream against this library's launches on both sides
and the buffer reuse of the overlapped loop; it says nothing about links.  Exit code 77: the process group could not be created on
this box (nothing of this repo was reached)."""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ.setdefault("MASTER_PORT", "29733")   # the test passes a free one
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import numpy as np
import torch
import torch.distributed as dist

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
try:
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=60))
    probe = torch.ones(8, device=dev)
    dist.all_reduce(probe)
    torch.cuda.synchronize()
    assert float(probe.sum()) == 8.0
except Exception as e:                                       # noqa: BLE001 — whatever keeps RCCL from starting is the box's, not the product's
    print("RCCL_UNAVAILABLE", repr(e), flush=True)
    sys.exit(77)

import attribution_ref as ar
from focnerf_amd.combine import ObjectCombiner

K, N, T, chunk = 3, 1000, 64, 256                            # pieces of 256, 256, 256 and a ragged one of 232
dens, rgb, nears, fars = ar.fields(K, N, T, 41)
fields = [torch.from_numpy(np.concatenate([dens[k][..., None], rgb[k]], -1).astype(np.float32)).cuda().contiguous() for k in range(K)]
nears, fars = torch.from_numpy(nears).cuda(), torch.from_numpy(fars).cuda()


def make(f4, into_out):
    def fn(lo, hi, out):
        if into_out and out is not None:                     # the first object writes straight into the send buffer
            out.copy_(f4[lo:hi])
            return out
        return f4[lo:hi].clone()
    return fn


fns = [make(fields[k], k == 0) for k in range(K)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


plain = ObjectCombiner(rank=0, world_size=1)
img0, dep0, att0 = plain.render_view(fns, N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=chunk, attribution=(0, K))
assert plain.bytes_sent == 0 and len(set(att0.instance.tolist())) >= 3 and float(att0.weights.max()) > 0.5
rccl = ObjectCombiner(collectives_at_world_1=True)           # rank and world size from the process group
assert (rccl.rank, rccl.world, rccl.xch) == (0, 1, True)
views = 0
for overlap in (True, False):
    for rep in range(2):                                     # repeated: the double buffers, the id planes' included, are reused across views
        img1, dep1, att1 = rccl.render_view(fns, N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=chunk, overlap=overlap, attribution=(0, K))
        assert same(img1, img0) and same(dep1, dep0), f"image / depth differ (overlap={overlap}, view {rep})"
        assert same(att1.weights, att0.weights) and same(att1.depth, att0.depth) and same(att1.instance, att0.instance), f"attribution differs (overlap={overlap}, view {rep})"
        assert rccl.bytes_sent == 0
        views += 1
# this rank's objects as 1 and 2 of a four-object scene: ids offset by first_object, a column nobody fills
img1, dep1, att1 = rccl.render_view(fns[:2], N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=chunk, attribution=(1, 4))
img2, dep2, att2 = plain.render_view(fns[:2], N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=chunk, attribution=(1, 4))
assert same(img1, img2) and same(dep1, dep2) and all(same(a, b) for a, b in zip(att1, att2))
assert (att1.weights[:, [0, 3]] == 0).all() and set(att1.instance.tolist()) == {-1, 1, 2}
# without the keyword: the pair, today's bits
pair = rccl.render_view(fns, N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=chunk)
assert len(pair) == 2 and same(pair[0], img0) and same(pair[1], dep0)

torch.cuda.synchronize()
print("RCCL_ATTR_OK backend", dist.get_backend(), "views", views + 2, flush=True)
dist.destroy_process_group()
