"""The two ends of a training step at the headline shape (800 x 800, V = 100 views, N = 4096 rays, C = 4), two legs alternating in one
process: (a) the reference trainer's torch lines for the batch (nerf/provider.py:398-447 collate, nerf/utils.py:57-157 get_rays, with
its fp32 preload on the device) and for the loss (nerf/utils.py:840-899: rand_like, blend, MSELoss(reduction='none').mean(-1), .mean()),
restated here; (b) RaySampler.next() + photo_loss on a uint8 dataset. Per leg: the batch alone, the loss with its backward alone, both
as one replayed graph, and both as the front and back end of the headline render (bench's model, its render call and step count) with
FusedAdam under LossScaler, eager and as one replayed graph. Medians over the rounds of the time per call (device events around a
window of calls). (b) is always compared with (a) of the same run. One JSON line.

The YOLO mask lines of get_rays (cv2 on the host) and the error map are left out of both legs. In a graph, leg (a) needs its view index
from the host before every replay (a static index tensor, copied in); leg (b) needs nothing.

usage: python tools/time_batch.py [--rounds 7] [--window 30] [--step-rounds 5] [--step-window 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from focnerf_amd import DeviceDataset, FusedAdam, LossScaler, RaySampler, photo_loss, synthetic  # noqa: E402

H = W = bench.VIEW
V, N, C = 100, bench.NUM_RAYS, 4
LEGS = ("torch_lines", "device_batch")


# ---------------------------------------------------------------- leg (a): the reference's lines
def torch_get_rays(poses, intrinsics, N):
    """nerf/utils.py:57-157 for N > 0, patch_size 1, no error map, without the mask lines."""
    device = poses.device
    B = poses.shape[0]
    fx, fy, cx, cy = intrinsics
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=device), torch.linspace(0, H - 1, H, device=device), indexing="ij")
    i = i.t().reshape([1, H * W]).expand([B, H * W]) + 0.5
    j = j.t().reshape([1, H * W]).expand([B, H * W]) + 0.5
    N = min(N, H * W)
    inds = torch.randint(0, H * W, size=[N], device=device)
    inds = inds.expand([B, N])
    i = torch.gather(i, -1, inds)
    j = torch.gather(j, -1, inds)
    zs = torch.ones_like(i)
    xs = (i - cx) / fx * zs
    ys = (j - cy) / fy * zs
    directions = torch.stack((xs, ys, zs), dim=-1)
    directions = directions / torch.norm(directions, dim=-1, keepdim=True)
    rays_d = directions @ poses[:, :3, :3].transpose(-1, -2)
    rays_o = poses[..., :3, 3]
    rays_o = rays_o[..., None, :].expand_as(rays_d)
    return rays_o, rays_d, inds


def torch_collate(images, poses, intrinsics, index):
    """nerf/provider.py:420-438; `index` a list of one view (eager) or a [1] int64 tensor on the device (inside a graph)."""
    p = poses[index]
    rays_o, rays_d, inds = torch_get_rays(p, intrinsics, N)
    im = images[index]
    im = torch.gather(im.view(1, -1, C), 1, torch.stack(C * [inds], -1))
    return rays_o, rays_d, im


def torch_targets(images):
    """nerf/utils.py:840-858, color_space 'srgb', C = 4, no background model."""
    bg_color = torch.rand_like(images[..., :3])
    gt_rgb = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
    return bg_color, gt_rgb


_criterion = torch.nn.MSELoss(reduction="none")


def torch_loss(pred_rgb, gt_rgb):
    """nerf/utils.py:867-899 without the error map."""
    return _criterion(pred_rgb, gt_rgb).mean(-1).mean()


# ---------------------------------------------------------------- timing
def window_us(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1000.0 * s.elapsed_time(e) / n


def capture(fn, warmup=3):
    """`fn` as one graph (warm-up and capture on a side stream, as focnerf_amd.graph.GraphedStep does) -> the replay callable."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    return graph.replay


def measure(fns, rounds, window, warmup=10):
    for _ in range(warmup):
        for leg in LEGS:
            fns[leg]()
    torch.cuda.synchronize()
    samples = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            samples[leg].append(window_us(fns[leg], window))
    out = {leg: {"us": round(statistics.median(samples[leg]), 2), "us_min": round(min(samples[leg]), 2), "us_max": round(max(samples[leg]), 2)} for leg in LEGS}
    out["device_over_torch"] = round(out[LEGS[1]]["us"] / out[LEGS[0]]["us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-window", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_batch.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)

    gen = torch.Generator().manual_seed(0)
    poses = synthetic.rand_poses(V, dev, radius=2.0, generator=gen)
    intr = synthetic.intrinsics(H, W)
    u8 = torch.empty(V, H, W, C, dtype=torch.uint8, device=dev)
    for v in range(V):                                           # a view at a time: 2.5 MB each from the host
        u8[v] = torch.randint(0, 256, (H, W, C), generator=gen, dtype=torch.uint8).to(dev)
    f32 = u8.float() / 255                                       # the reference's preload: fp32 on the device
    sampler = RaySampler(DeviceDataset(u8, poses, intr), num_rays=N, seed=0)
    counter = [0]

    def next_index():
        counter[0] += 1
        return [counter[0] % V]

    idx_host = torch.zeros(1, dtype=torch.int64).pin_memory()
    idx_dev = torch.zeros(1, dtype=torch.int64, device=dev)

    def next_index_static():
        idx_host[0] = next_index()[0]
        idx_dev.copy_(idx_host, non_blocking=True)

    result = {"tool": "time_batch", "device": torch.cuda.get_device_name(0), "shape": {"H": H, "W": W, "V": V, "N": N, "C": C},
              "rounds": args.rounds, "window": args.window, "baseline": LEGS[0],
              "dataset_bytes": {LEGS[0]: f32.numel() * 4, LEGS[1]: u8.numel()}}

    # ---- the batch alone
    result["batch"] = measure({LEGS[0]: lambda: torch_targets(torch_collate(f32, poses, intr, next_index())[2]),
                               LEGS[1]: sampler.next}, args.rounds, args.window)

    # ---- the loss with its backward alone, on a fixed prediction
    pred_a = torch.rand(1, N, 3, device=dev).requires_grad_(True)
    pred_b = pred_a.detach().clone().requires_grad_(True)
    gt = torch.rand(1, N, 3, device=dev)

    def loss_a():
        pred_a.grad = None
        torch_loss(pred_a, gt).backward()

    def loss_b():
        pred_b.grad = None
        photo_loss(pred_b, gt)[0].backward()
    result["loss_backward"] = measure({LEGS[0]: loss_a, LEGS[1]: loss_b}, args.rounds, args.window)

    # ---- both ends without a render between them (a stand-in prediction computed from the rays), eager and as one replayed graph
    def ends_a(index):
        rays_o, rays_d, im = torch_collate(f32, poses, intr, index)
        _, gt_rgb = torch_targets(im)
        pred = (rays_d * 0.5 + 0.5).requires_grad_(True)
        torch_loss(pred, gt_rgb).backward()

    def ends_b():
        b = sampler.next()
        pred = (b.rays_d * 0.5 + 0.5).requires_grad_(True)
        photo_loss(pred, b.gt_rgb)[0].backward()
    result["ends_eager"] = measure({LEGS[0]: lambda: ends_a(next_index()), LEGS[1]: ends_b}, args.rounds, args.window)
    replay_a, replay_b = capture(lambda: ends_a(idx_dev)), capture(ends_b)

    def graph_a():
        next_index_static()
        replay_a()
    result["ends_graph"] = measure({LEGS[0]: graph_a, LEGS[1]: replay_b}, args.rounds, args.window)

    # ---- as the front and back end of the headline render, FusedAdam under LossScaler
    def make_step(leg):
        model = bench.build_model(1, dev, seed=0).train()
        opt, scaler = FusedAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15), LossScaler()
        smp = RaySampler(DeviceDataset(u8, poses, intr), num_rays=N, seed=1)

        def render(rays_o, rays_d, bg):
            return model.render(rays_o, rays_d, staged=False, num_steps=bench.NUM_STEPS, upsample_steps=0, perturb=True, bg_color=bg, fused=True)["image"]

        def step_a(index):
            rays_o, rays_d, im = torch_collate(f32, poses, intr, index)
            with torch.autocast("cuda", dtype=torch.float16):
                bg, gt_rgb = torch_targets(im)
                loss = torch_loss(render(rays_o, rays_d, bg), gt_rgb)
            scaler.scale(loss).backward()
            opt.step(scaler=scaler, zero_grads=True)

        def step_b():
            b = smp.next()
            with torch.autocast("cuda", dtype=torch.float16):
                image = render(b.rays_o, b.rays_d, b.bg_color)
            loss, _ = photo_loss(image, b.gt_rgb)
            scaler.scale(loss).backward()
            opt.step(scaler=scaler, zero_grads=True)
        return step_a if leg == LEGS[0] else step_b

    step_a, step_b = make_step(LEGS[0]), make_step(LEGS[1])
    result["train_step_eager"] = measure({LEGS[0]: lambda: step_a(next_index()), LEGS[1]: step_b}, args.step_rounds, args.step_window, warmup=5)
    gstep_a, gstep_b = make_step(LEGS[0]), make_step(LEGS[1])
    greplay_a, greplay_b = capture(lambda: gstep_a(idx_dev)), capture(gstep_b)

    def gstep_a_call():
        next_index_static()
        greplay_a()
    result["train_step_graph"] = measure({LEGS[0]: gstep_a_call, LEGS[1]: greplay_b}, args.step_rounds, args.step_window, warmup=5)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
