"""Training batches and the photometric loss on the device (csrc/batch.hip): one launch draws a batch, one more gives the loss, its
gradient and the error map.

The reference trainer builds a batch with about fifteen torch ops (nerf/provider.py:398-447 NeRFDataset.collate, nerf/utils.py:57-157
get_rays) and its loss with about ten more and their backward nodes (nerf/utils.py:840-899 Trainer.train_step). Here the dataset stays
resident on the device and the step counter advances inside the sampler's launch, so a whole step replays as a graph that produces a
new batch each time by itself:

    data = DeviceDataset(images, poses, (fx, fy, cx, cy))            # images [V,H,W,C] uint8 / fp16 / fp32 on the device
    sampler = RaySampler(data, num_rays=4096, seed=0)
    b = sampler.next()                                               # one launch: rays_o, rays_d, inds, gt_rgb, bg_color, view, inds_coarse
    out = model.run(b.rays_o, b.rays_d, None, fused=True, bg_color=b.bg_color, ...)
    loss, ray_loss = photo_loss(out["image"], b.gt_rgb)              # one launch; backward is one multiply
    scaler.scale(loss).backward(); opt.step(scaler=scaler, zero_grads=True)

Random numbers are Philox4x32-10 with counter (ray, step, stream) and key seed (include/focnerf.h): a batch is a pure function of
(seed, step), whatever the launch size. Torch's random stream is NOT reproduced: a seeded run here draws other pixels than a seeded
reference run. Out of scope: patch_size > 1 (it exists for the LPIPS term), batches of more than one view (the
reference's loader always has batch_size=1) and the 64 x 64 YOLO ray mask (passed through `yolo_details` as today). The parameter EMA
is not a batch matter: focnerf_amd/ema.py `ParameterEMA` takes it inside `FusedAdam.step(ema=...)`.
There is no fallback: without the library the import fails.
"""
from typing import NamedTuple, Optional, Union

import torch

from ._lib import FOC_F16, FOC_F32, FOC_U8, check, lib, ptr, stream_of

CELLS = 128 * 128               # the error map's cells per view (nerf/provider.py:320)
MAX_PIXELS = 1 << 30
_IMAGE_DTYPES = {torch.uint8: FOC_U8, torch.float16: FOC_F16, torch.float32: FOC_F32}
_KINDS = {"mse": 0, "huber": 1}


class Batch(NamedTuple):
    rays_o: torch.Tensor                        # [1,N,3]
    rays_d: torch.Tensor                        # [1,N,3]
    inds: torch.Tensor                          # [1,N] int64
    gt_rgb: torch.Tensor                        # [1,N,3]
    bg_color: Union[torch.Tensor, float]        # [1,N,3], or the float 1 where the reference passes 1
    view: torch.Tensor                          # [1] int32
    inds_coarse: Optional[torch.Tensor]         # [1,N] int64 with an error map, else None


class DeviceDataset:
    """The training views resident on the device: `images [V,H,W,C]` (uint8, float16 or float32; C = 3 or 4 — uint8 takes a quarter of
    the memory of the reference's fp32 preload), `poses [V,4,4]` float32, `intrinsics = (fx, fy, cx, cy)`, `color_space` 'srgb' (the
    reference's default: pixels as they are) or 'linear' (srgb_to_linear on r, g, b)."""

    def __init__(self, images, poses, intrinsics, color_space="srgb"):
        for name, t in (("images", images), ("poses", poses)):
            if not torch.is_tensor(t):
                raise ValueError(f"DeviceDataset: {name} must be a tensor")
        if images.dtype not in _IMAGE_DTYPES:
            raise ValueError(f"DeviceDataset: images must be uint8, float16 or float32 (got {images.dtype})")
        if images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError(f"DeviceDataset: images [V,H,W,3] or [V,H,W,4] expected (got {tuple(images.shape)})")
        V, H, W, C = images.shape
        if V < 1 or H < 1 or W < 1 or H * W > MAX_PIXELS:
            raise ValueError(f"DeviceDataset: V >= 1 and H * W in 1 .. 2^30 pixels expected (got {V} views of {H} x {W})")
        if poses.dtype != torch.float32:
            raise ValueError(f"DeviceDataset: poses must be float32 (got {poses.dtype})")
        if tuple(poses.shape) != (V, 4, 4):
            raise ValueError(f"DeviceDataset: poses [{V},4,4] expected (got {tuple(poses.shape)})")
        try:
            fx, fy, cx, cy = (float(v) for v in intrinsics)
        except (TypeError, ValueError):
            raise ValueError("DeviceDataset: intrinsics must be the four numbers (fx, fy, cx, cy)") from None
        if fx == 0 or fy == 0 or not all(v == v and abs(v) != float("inf") for v in (fx, fy, cx, cy)):
            raise ValueError(f"DeviceDataset: intrinsics must be finite, fx and fy not zero (got {(fx, fy, cx, cy)})")
        if color_space not in ("srgb", "linear"):
            raise ValueError(f"DeviceDataset: color_space must be 'srgb' or 'linear' (got {color_space!r})")
        for name, t in (("images", images), ("poses", poses)):         # shapes first, devices last: a wrong shape reads the same on any host
            if not t.is_cuda:
                raise ValueError(f"DeviceDataset: {name} is on {t.device}; these ops have no CPU implementation")
        if poses.device != images.device:
            raise ValueError(f"DeviceDataset: poses is on {poses.device}, images on {images.device}")
        self.images, self.poses = images.contiguous(), poses.contiguous()
        self.intrinsics = (fx, fy, cx, cy)
        self.color_space = color_space
        self.V, self.H, self.W, self.C = int(V), int(H), int(W), int(C)

    @property
    def device(self):
        return self.images.device


class RaySampler:
    """Draws the training batches of a `DeviceDataset`, one launch each. `next()` RETURNS THE SAME TENSORS EVERY TIME: the outputs, the
    step counter, the order and the ticket word are allocated once and their addresses never change, so a graph capture sees the same
    buffers and each replay overwrites them with the next batch (clone what must outlive the next call).

    The view of a step is `order[step mod V]`; `shuffle()` writes a new permutation for the next epoch, outside any graph. With
    `error_map=True` the sampler keeps `error_map [V,16384]` of ones on the device, draws `inds_coarse` with torch.multinomial from the
    view's row (that one draw stays a torch op, and torch's generator decides it) and the kernel jitters the pixel inside its cell;
    pass `(sampler.error_map, b.view, b.inds_coarse)` to `photo_loss` to have the map updated. `num_rays` is clamped to H * W as the
    reference does; `clamp=False` keeps it (the uniform draw is with replacement either way: pixels of a small image then repeat more)."""

    def __init__(self, dataset, num_rays=4096, seed=0, random_bg=True, error_map=False, clamp=True):
        if not isinstance(dataset, DeviceDataset):
            raise ValueError("RaySampler: dataset must be a DeviceDataset")
        if int(num_rays) < 1:
            raise ValueError(f"RaySampler: num_rays must be >= 1 (got {num_rays})")
        self.dataset = dataset
        dev = dataset.device
        self.num_rays = N = min(int(num_rays), dataset.H * dataset.W) if clamp else int(num_rays)      # nerf/utils.py:73
        if error_map and N > CELLS:
            raise ValueError(f"RaySampler: the error-map route draws at most {CELLS} distinct cells (got num_rays {N})")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.random_bg = bool(random_bg)
        self.order = torch.arange(dataset.V, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ws = torch.zeros(lib.foc_batch_workspace_bytes() // 4, dtype=torch.int32, device=dev)    # the ticket word: zeroed once
        self.error_map = torch.ones(dataset.V, CELLS, dtype=torch.float32, device=dev) if error_map else None
        self._inds = torch.empty(1, N, dtype=torch.int64, device=dev)
        self._rays_o = torch.empty(1, N, 3, dtype=torch.float32, device=dev)
        self._rays_d = torch.empty(1, N, 3, dtype=torch.float32, device=dev)
        self._bg = torch.empty(1, N, 3, dtype=torch.float32, device=dev)
        self._gt = torch.empty(1, N, 3, dtype=torch.float32, device=dev)
        self._view = torch.zeros(1, dtype=torch.int32, device=dev)
        self._inds_coarse = torch.empty(1, N, dtype=torch.int64, device=dev) if error_map else None

    def _draw_coarse(self):
        """inds_coarse of the step about to be drawn (nerf/utils.py:101), selected by device indices: no synchronisation."""
        view = self.order.index_select(0, torch.remainder(self.step, self.dataset.V))
        self._inds_coarse.copy_(torch.multinomial(self.error_map.index_select(0, view), self.num_rays, replacement=False))
        return self._inds_coarse

    def next(self, workgroups=0):
        """The batch of the current step, and the step advances by one — all inside one launch. `workgroups`: 0 for the library's
        choice; any other launch size gives the same bits."""
        d = self.dataset
        coarse = self._draw_coarse() if self.error_map is not None else None
        fx, fy, cx, cy = d.intrinsics
        check(lib.foc_batch_sample(ptr(d.images), _IMAGE_DTYPES[d.images.dtype], d.V, d.H, d.W, d.C, ptr(d.poses), fx, fy, cx, cy, ptr(self.order), ptr(self.step),
                                   self.seed, self.num_rays, ptr(coarse), int(self.random_bg), int(d.color_space == "linear"), ptr(self._inds), ptr(self._rays_o),
                                   ptr(self._rays_d), ptr(self._bg), ptr(self._gt), ptr(self._view), ptr(self._ws), self._ws.numel() * 4, int(workgroups),
                                   stream_of(d.images)), "batch_sample")
        bg = self._bg if (d.C == 4 and self.random_bg) else 1.0             # nerf/utils.py:847-853
        return Batch(self._rays_o, self._rays_d, self._inds, self._gt, bg, self._view, coarse)

    def shuffle(self, generator=None):
        """A new permutation of the views into `order` (in place), for the next epoch. `generator`: a CPU torch.Generator, or torch's own."""
        self.order.copy_(torch.randperm(self.dataset.V, generator=generator).to(torch.int32))

    def view_rays(self, v):
        """All the rays of view `v`, row-major: rays_o, rays_d [1,H*W,3] (the evaluation route; takes the place of the host meshgrid)."""
        d = self.dataset
        v = int(v)
        if not 0 <= v < d.V:
            raise ValueError(f"RaySampler: view {v} of {d.V}")
        rays_o = torch.empty(1, d.H * d.W, 3, dtype=torch.float32, device=d.device)
        rays_d = torch.empty_like(rays_o)
        fx, fy, cx, cy = d.intrinsics
        check(lib.foc_view_rays(ptr(d.poses[v]), fx, fy, cx, cy, d.H, d.W, ptr(rays_o), ptr(rays_d), stream_of(d.poses)), "view_rays")
        return rays_o, rays_d

    def state_dict(self):
        """seed, step, order and the error map (on the host): a resumed run continues its sequence. Reads the device: a synchronisation."""
        return {"seed": self.seed, "step": int(self.step.item()), "order": self.order.cpu(),
                "error_map": self.error_map.cpu() if self.error_map is not None else None}

    def load_state_dict(self, state_dict):
        order = torch.as_tensor(state_dict["order"], dtype=torch.int32)
        if tuple(order.shape) != (self.dataset.V,) or sorted(order.tolist()) != list(range(self.dataset.V)):
            raise ValueError(f"RaySampler: order must be a permutation of {self.dataset.V} views")
        em = state_dict.get("error_map")
        if (em is None) != (self.error_map is None):
            raise ValueError("RaySampler: the state dict and this sampler disagree about the error map")
        if em is not None and tuple(em.shape) != tuple(self.error_map.shape):
            raise ValueError(f"RaySampler: error_map {tuple(self.error_map.shape)} expected (got {tuple(em.shape)})")
        self.seed = int(state_dict["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.step.fill_(int(state_dict["step"]))
        self.order.copy_(order)
        if em is not None:
            self.error_map.copy_(em)


# ---------------------------------------------------------------- the loss
_loss_workspaces = {}


def _loss_workspace(device):
    """Ticket and slots of the loss, one per device, as FusedAdam's workspace: it serves one stream at a time."""
    ws = _loss_workspaces.get(device)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("photo_loss: the workspace must exist before a graph capture (one eager call first)")
        ws = torch.zeros(lib.foc_photo_loss_workspace_bytes() // 8, dtype=torch.int64, device=device)      # zeroed once
        _loss_workspaces[device] = ws
    return ws


class _PhotoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt_rgb, kind, delta, error_map):
        N = pred.numel() // 3
        dev = pred.device
        p, g = pred.contiguous(), gt_rgb.contiguous()
        ray_loss = torch.empty(pred.shape[:-1], dtype=torch.float32, device=dev)
        grad = torch.empty(pred.shape, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _loss_workspace(dev)
        emap, view, coarse, V = None, None, None, 0
        if error_map is not None:
            emap, view, coarse = error_map
            V = emap.shape[0]
        check(lib.foc_photo_loss(ptr(p), FOC_F16 if p.dtype == torch.float16 else FOC_F32, ptr(g), N, kind, delta, ptr(emap), V, ptr(view), ptr(coarse),
                                 ptr(ray_loss), ptr(grad), ptr(loss), ptr(ws), ws.numel() * 8, stream_of(p)), "photo_loss")
        ctx.save_for_backward(grad)
        ctx.pred_dtype = pred.dtype
        ctx.mark_non_differentiable(ray_loss)
        return loss.view(()), ray_loss

    @staticmethod
    def backward(ctx, grad_loss, _grad_ray_loss):
        (grad,) = ctx.saved_tensors
        g = grad * grad_loss                    # the upstream scalar is read on the device: no synchronisation
        return (g if g.dtype == ctx.pred_dtype else g.to(ctx.pred_dtype)), None, None, None, None


def photo_loss(pred, gt_rgb, kind="mse", delta=0.1, error_map=None):
    """The trainer's criterion and its mean in one launch (nerf/utils.py:867-899): -> (loss, ray_loss). `pred [...,3]` float32 or float16
    (widened exactly), `gt_rgb` float32 of the same shape; `kind` 'mse', or 'huber' with `delta` (torch.nn.HuberLoss's definition).
    `ray_loss [...]` is the criterion's mean over the three channels, `loss` its mean over the rays, a 0-dim float32 whose backward is
    one multiply of the stored d(loss)/d(pred) by the upstream scalar. `error_map=(map [V,16384], view [1] int32, inds_coarse [.,N]
    int64)`: the launch also writes map[view, c] = 0.1 * old + 0.9 * ray_loss, in place. The same bits on every run. The ticket and
    the slots of the mean live in one workspace per device: run the loss on one stream at a time."""
    if kind not in _KINDS:
        raise ValueError(f"photo_loss: kind must be 'mse' or 'huber' (got {kind!r})")
    for name, t in (("pred", pred), ("gt_rgb", gt_rgb)):
        if not torch.is_tensor(t):
            raise ValueError(f"photo_loss: {name} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"photo_loss: {name} is on {t.device}; these ops have no CPU implementation")
    if pred.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"photo_loss: pred must be float32 or float16 (got {pred.dtype})")
    if gt_rgb.dtype != torch.float32:
        raise ValueError(f"photo_loss: gt_rgb must be float32 (got {gt_rgb.dtype})")
    if pred.dim() < 1 or pred.shape[-1] != 3 or pred.numel() < 3 or pred.shape != gt_rgb.shape or pred.device != gt_rgb.device:
        raise ValueError(f"photo_loss: pred and gt_rgb [...,3] of one shape on one device expected (got {tuple(pred.shape)} and {tuple(gt_rgb.shape)})")
    delta = float(delta)
    if kind == "huber" and not (0.0 < delta < float("inf")):
        raise ValueError(f"photo_loss: delta must be finite and > 0 (got {delta})")
    if error_map is not None:
        emap, view, coarse = error_map
        N = pred.numel() // 3
        if (emap.dtype != torch.float32 or emap.dim() != 2 or emap.shape[1] != CELLS or not emap.is_contiguous() or view.dtype != torch.int32
                or view.numel() != 1 or coarse.dtype != torch.int64 or coarse.numel() != N or not coarse.is_contiguous()
                or any(t.device != pred.device for t in (emap, view, coarse))):
            raise ValueError(f"photo_loss: error_map = (map [V,{CELLS}] float32 contiguous, view [1] int32, inds_coarse [{N}] int64) on pred's device expected")
    return _PhotoLoss.apply(pred, gt_rgb, _KINDS[kind], delta, error_map)
