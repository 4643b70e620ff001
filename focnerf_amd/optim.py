"""The trainer's optimizer step on the library's own kernels (csrc/optim.hip): overflow check, unscale and Adam in two launches.

The reference trainer's optimizer is always `torch.optim.Adam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)` under torch's
GradScaler (main_nerf.py:211,472, nerf/utils.py:1225-1235): about twenty small launches per step. Two ways in:

    opt = FusedAdam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)

    scaler = torch.amp.GradScaler("cuda")          # the drop-in route: the trainer's lines stay as they are; torch does the inf
    scaler.scale(loss).backward()                  # check and the scale update, FusedAdam the update (a one-workgroup launch + one launch per 16 tensors)
    scaler.step(opt); scaler.update()

    scaler = LossScaler()                          # the fast route: check + decision + scale update in one launch, the update in
    scaler.scale(loss).backward()                  # a second one, nothing else; no host synchronisation, so it captures in a graph
    opt.step(scaler=scaler, zero_grads=True)       # (there is no scaler.update(): the step has done it)

    ema = ParameterEMA(model.parameters(), 0.95)   # the trainer's parameter EMA (focnerf_amd/ema.py) rides in the update launch of either
    opt.step(scaler=scaler, ema=ema)               # route — `scaler.step(opt, ema=ema)` under torch's GradScaler — instead of ema.update()

The state is the one `torch.optim.Adam(fused=True, capturable=True)` keeps — per parameter `step` (0-dim fp32 on the device), `exp_avg`,
`exp_avg_sq`, the same keys in `param_groups` — so state dicts go both ways between the two classes and the reference trainer's full
checkpoints keep loading; `LossScaler`'s state dict is `torch.amp.GradScaler`'s. There is no fallback: without the library the import fails.
"""
import ctypes

import torch

from ._lib import DEFINES, FocOptimStep, FocOptimTensor, check, lib, stream_of

CHUNK = DEFINES["FOC_OPTIM_CHUNK"]                    # elements per workgroup of the kernels (include/focnerf.h)
MAX_TENSORS = DEFINES["FOC_OPTIM_MAX_TENSORS"]        # tensors per call
_PHASE_STEP, _PHASE_CHECK, _PHASE_DECIDE = 0, 1, 2
_WS_FOUND, _WS_SCALE_USED = 5, 6    # words of the workspace where the decide phase leaves found_inf and the scale of this step's grads


def _adam_defaults(lr, betas, eps, weight_decay):
    """The `defaults` of `torch.optim.Adam(fused=True, capturable=True)` of THIS torch: whatever keys its constructor has, at its values."""
    d = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
    d.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=True, capturable=True)
    return d


class LossScaler:
    """Dynamic loss scale whose update runs inside `FusedAdam.step(scaler=...)`. `scale` (fp32) and the growth tracker (int32) are 0-dim
    device tensors that the step's first launch updates by torch._amp_update_scale_'s rule; `state_dict()` / `load_state_dict()` speak
    `torch.amp.GradScaler`'s five keys. No `update()`: the step has already done it."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not growth_factor > 1.0:
            raise ValueError("LossScaler: growth_factor must be > 1")
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError("LossScaler: backoff_factor must lie in (0, 1)")
        if int(growth_interval) < 1:
            raise ValueError("LossScaler: growth_interval must be >= 1")
        self._init_scale = float(init_scale)
        self._init_growth_tracker = 0
        self._growth_factor = float(growth_factor)
        self._backoff_factor = float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._scale = None                  # created on the device of the first loss (or the first step), as torch's GradScaler does
        self._growth_tracker = None

    def _on(self, device):
        if self._scale is None or self._scale.device != device:
            capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
            if capturing:
                raise RuntimeError("LossScaler: scale(loss) or FusedAdam.init_state(scaler) must run once before a graph capture")
            scale = self._init_scale if self._scale is None else float(self._scale)
            tracker = self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker)
            self._scale = torch.full((), scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((), tracker, dtype=torch.int32, device=device)
        return self

    def scale(self, loss):
        self._on(loss.device)
        return loss * self._scale

    def get_scale(self):
        """The current scale as a float (reads the device: a synchronisation, as `GradScaler.get_scale()`)."""
        return self._init_scale if self._scale is None else float(self._scale.item())

    def _get_growth_tracker(self):
        return self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker.item())

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        if len(state_dict) == 0:
            raise RuntimeError("LossScaler: the source state dict is empty (it came from a disabled GradScaler)")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)


class FusedAdam(torch.optim.Optimizer):
    """Adam with L2 weight decay for fp32 parameters on the device, state and `param_groups` laid out as
    `torch.optim.Adam(fused=True, capturable=True)`. `lr` may be a 0-dim fp32 device tensor (a schedule that runs under graph replay)."""

    _step_supports_amp_scaling = True       # torch's GradScaler then hands over `grad_scale` / `found_inf` instead of unscaling itself

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad=True is not supported")
        if maximize:
            raise ValueError("FusedAdam: maximize=True is not supported")
        if not torch.is_tensor(lr) and not 0.0 <= lr:
            raise ValueError(f"FusedAdam: invalid lr {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"FusedAdam: invalid eps {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: invalid betas {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"FusedAdam: invalid weight_decay {weight_decay}")
        self._workspaces = {}
        super().__init__(params, _adam_defaults(lr, betas, eps, weight_decay))

    def add_param_group(self, param_group):
        params = param_group["params"]
        params = [params] if torch.is_tensor(params) else list(params)
        param_group = dict(param_group, params=params)
        for p in params:
            if p.dtype != torch.float32:
                raise ValueError(f"FusedAdam: params must be float32 (got {p.dtype})")
            if p.layout != torch.strided or not p.is_contiguous():
                raise ValueError("FusedAdam: params must be dense and contiguous")
        super().add_param_group(param_group)

    # ---------------------------------------------------------------- state
    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam: the state must exist before a graph capture (one eager step, or init_state())")
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not (torch.is_tensor(st["step"]) and st["step"].device == p.device and st["step"].dtype == torch.float32):
            st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device)      # a state loaded from a non-capturable Adam
        return st

    def _workspace(self, device):
        ws = self._workspaces.get(device)
        if ws is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam: the workspace must exist before a graph capture (one eager step, or init_state())")
            ws = torch.zeros(lib.foc_optim_workspace_bytes(MAX_TENSORS) // 4, dtype=torch.int32, device=device)
            self._workspaces[device] = ws
        return ws

    def init_state(self, scaler=None, ema=None):
        """Allocate moments, step counters and the workspace now (before a graph capture that has no eager warm-up step); with `ema`, its
        device counter and its own workspace too."""
        for group in self.param_groups:
            for p in group["params"]:
                self._state_of(p)
                self._workspace(p.device)
                if scaler is not None:
                    scaler._on(p.device)
                if ema is not None and p.is_cuda:
                    ema._on(p.device)
                    ema._workspace(p.device)

    # ---------------------------------------------------------------- step
    def _collect(self):
        items = []
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise RuntimeError("FusedAdam: a param group asks for amsgrad / maximize, which this optimizer does not offer")
            lr = group["lr"]
            lr_t = None
            if torch.is_tensor(lr):
                if lr.is_cuda:
                    if lr.dtype != torch.float32 or lr.numel() != 1:
                        raise RuntimeError("FusedAdam: a device lr must be one float32 element")
                    lr_t, lr = lr, 0.0
                else:
                    lr = float(lr)
            b1, b2 = (float(b) for b in group["betas"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.layout != torch.strided:
                    raise RuntimeError("FusedAdam: sparse grads are not supported")
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise RuntimeError("FusedAdam: grads must be float32 and contiguous")
                if not p.is_cuda or g.device != p.device:
                    raise RuntimeError("FusedAdam: params and grads live on the device; this optimizer has no CPU implementation")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdam: params must be float32 and contiguous")
                items.append((p, g, self._state_of(p), lr, lr_t, b1, b2, float(group["eps"]), float(group["weight_decay"])))
        return items

    @staticmethod
    def _descriptors(chunk):
        arr = (FocOptimTensor * len(chunk))()
        for d, (p, g, st, lr, lr_t, b1, b2, eps, wd) in zip(arr, chunk):
            d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.step = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()
            d.lr_tensor = lr_t.data_ptr() if lr_t is not None else None
            d.n = p.numel()
            d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = lr, b1, b2, eps, wd
        return arr

    @torch.no_grad()
    def step(self, closure=None, *, scaler=None, zero_grads=False, ema=None):
        """One step. `scaler`: a `LossScaler` whose scale the grads carry — check, decision, scale update and update, two launches per 16
        tensors, no host synchronisation. Without it: under `torch.amp.GradScaler.step(opt)` the `grad_scale` / `found_inf` torch has set
        on this object decide; otherwise plain Adam. `zero_grads=True` writes zeros to the grads in the same pass — also when the step is
        skipped for an overflow (torch would leave them; they are of no use after a skipped step). Params whose grad is None are left out
        and their step counters do not advance.
        `ema`: a `ParameterEMA` that takes its update with this step, instead of an `ema.update()` after it — also when the step is skipped
        for an overflow, as the reference's unconditional call does. The shadows of the step's params are updated inside the update launch;
        params the EMA tracks and the step leaves out (no grad, not in this optimizer) follow in one more launch per 16 on the same
        stream; its counter advances once. The launches of the step itself are the same with and without it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if scaler is not None and (grad_scale is not None or found_inf is not None):
            raise RuntimeError("FusedAdam: step(scaler=LossScaler) inside torch's GradScaler.step: one scaler at a time")
        if scaler is not None and not isinstance(scaler, LossScaler):
            raise TypeError("FusedAdam: scaler must be a focnerf_amd.optim.LossScaler (torch's GradScaler calls scaler.step(optimizer) itself)")
        if ema is not None and not hasattr(ema, "_for_step"):
            raise TypeError("FusedAdam: ema must be a focnerf_amd.ParameterEMA")
        items = self._collect()
        if not items:
            if ema is not None:
                ema.update()                    # nothing to step: the EMA's update alone
            return loss
        device = items[0][0].device
        if any(it[0].device != device for it in items):
            raise RuntimeError("FusedAdam: all params of one optimizer must live on one device")
        ws = self._workspace(device)
        stream = stream_of(items[0][0])
        chunks = [items[i:i + MAX_TENSORS] for i in range(0, len(items), MAX_TENSORS)]

        call = FocOptimStep()
        call.struct_bytes, call.tensor_bytes = ctypes.sizeof(FocOptimStep), ctypes.sizeof(FocOptimTensor)
        call.zero_grads = 1 if zero_grads else 0
        call.workspace, call.workspace_bytes = ws.data_ptr(), ws.numel() * 4

        riding, behind, by_torch = ema._for_step([it[0] for it in items], device) if ema is not None else ({}, [], [])
        ema_count = ema._count if ema is not None else None     # on `device` now; None: a constant decay
        opened = [ema is None]                  # the EMA of this step is opened (counter + 1, 1 - decay_t into the record) exactly once

        def run(chunk, phase):
            arr = self._descriptors(chunk) if chunk is not None else None
            call.n_tensors, call.tensors, call.phase = (len(chunk), arr, phase) if chunk is not None else (0, None, phase)
            if ema is None or phase == _PHASE_CHECK:
                check(lib.foc_optim_step(ctypes.byref(call), stream), "optim_step")
                return
            shadows = None
            if chunk is not None:
                shadows = (ctypes.c_uint64 * len(chunk))(*[riding[id(it[0])].data_ptr() if id(it[0]) in riding else 0 for it in chunk])
            advance, opened[0] = (0 if opened[0] else 1), True
            check(lib.foc_optim_step_ema(ctypes.byref(call), shadows, float(ema.decay), ema_count.data_ptr() if ema_count is not None else None,
                                         advance, stream), "optim_step_ema")

        def finish():
            if behind:
                ema._launch(behind, device, ws, advance=False)
            if by_torch:
                ema._torch_rule(by_torch, advanced=True)
            return loss

        if scaler is not None:
            scaler._on(device)
            call.scale, call.growth_tracker = scaler._scale.data_ptr(), scaler._growth_tracker.data_ptr()
            call.growth_factor, call.backoff_factor, call.growth_interval = scaler._growth_factor, scaler._backoff_factor, scaler._growth_interval
            if len(chunks) == 1:
                run(chunks[0], _PHASE_STEP)
                return finish()
            for chunk in chunks:            # one decision for all groups: every check, the decision, then every update
                run(chunk, _PHASE_CHECK)
            run(None, _PHASE_DECIDE)
            call.scale = call.growth_tracker = None
            call.found_inf, call.grad_scale = ws.data_ptr() + 4 * _WS_FOUND, ws.data_ptr() + 4 * _WS_SCALE_USED
        else:
            for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
                if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != device):
                    raise RuntimeError(f"FusedAdam: {name} must be one float32 element on the params' device")
            call.grad_scale = grad_scale.data_ptr() if grad_scale is not None else None
            call.found_inf = found_inf.data_ptr() if found_inf is not None else None
        for chunk in chunks:
            run(chunk, _PHASE_STEP)
        return finish()
