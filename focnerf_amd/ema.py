"""The trainer's parameter EMA on the library's kernels (csrc/optim.hip), with `torch_ema.ExponentialMovingAverage`'s interface.

The reference trainer keeps an exponential moving average of its parameters (nerf/utils.py:739 `ExponentialMovingAverage(model.parameters(),
decay=0.95)`), updates it after every optimizer step (:1125, :1256), evaluates and saves under store() / copy_to() / restore()
(:1164-1174, :1293-1295) and carries its state dict in every full checkpoint (:1454, :1521). torch_ema's update is three torch ops and a
temporary per tensor. Two ways in:

    ema = ParameterEMA(model.parameters(), decay=0.95)      # the trainer's line, with another class name (or `import torch_ema` with
    ...                                                     # focnerf_amd/dropin on the path: the trainer's lines stay as they are)
    opt.step(scaler=scaler, ema=ema)                        # the EMA inside the Adam launch: the shadow's read and write, no launch more
    scaler.step(opt, ema=ema); scaler.update()              # the same under torch's GradScaler, which forwards keyword arguments
    ema.update()                                            # alone: one launch per 16 tensors (the reference's call, unchanged)

The rule (include/focnerf.h), for a parameter p and its shadow s: n <- n + 1 (with use_num_updates; n starts at 0); decay_t = min(decay,
(1 + n) / (10 + n)) in double, `decay` without use_num_updates; omd = float32(1 - decay_t); s <- s - (s - p) * omd in three fp32
roundings. It runs after every step, also one the loss scaler skipped: the shadow then moves toward the unchanged parameters.

`num_updates` lives as a 0-dim int64 tensor on the device once a device parameter is updated (the step and the update read and advance it
there: no host synchronisation, so a step with its EMA captures in a graph); `state_dict()` and the `num_updates` attribute read it back,
which synchronises. fp32 dense contiguous device parameters go through the kernels; any other tensor (CPU, fp16, non-contiguous) goes
through the three torch ops of the rule with the decay derived on the host, so the class also works on CPU tensors. An instance that
holds BOTH kinds reads the device counter back on every update(): that update synchronises. copy_to / store / restore are torch copies:
they run once per evaluation, not per step.
"""
import contextlib
import copy
import ctypes
import weakref

import torch

from ._lib import DEFINES, check, lib, stream_of

MAX_TENSORS = DEFINES["FOC_OPTIM_MAX_TENSORS"]


def _omd(decay, num_updates):
    """float(1 - decay_t) as a Python double (the kernels and torch's `mul_` round it to fp32 once); num_updates: the count AFTER this update, or None"""
    if num_updates is not None:
        decay = min(decay, (1 + num_updates) / (10 + num_updates))
    return 1.0 - decay


def _drop_weight_caches():
    """The fused paths' derived weights (fp16 casts, packed MLP blobs, object features) live only inside an open `field.half_cache_scope`,
    keyed on the parameter's identity, which an in-place copy does not change: after copy_to() / restore() an open scope starts over."""
    import sys
    field = sys.modules.get(__package__ + ".field")
    if field is not None:
        field.drop_half_cache()


class ParameterEMA:
    """`torch_ema.ExponentialMovingAverage(parameters, decay, use_num_updates=True)`: the same methods, attributes and state dict."""

    def __init__(self, parameters, decay, use_num_updates=True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        parameters = list(parameters)
        if any(p.is_cuda for p in parameters) and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ParameterEMA: the shadows must exist before a graph capture")
        self.decay = decay
        self._host_updates = 0 if use_num_updates else None      # the count while there is no device counter (and what a new one starts from)
        self._count = None                                        # 0-dim int64 on the device of the first parameter the kernels serve
        self.shadow_params = [p.clone().detach() for p in parameters]
        self.collected_params = None
        self._params_refs = [weakref.ref(p) for p in parameters]
        self._workspaces = {}

    # ---------------------------------------------------------------- the counter
    @property
    def num_updates(self):
        """torch_ema's attribute: an int, or None without use_num_updates. Reads the device counter (a synchronisation) where there is one."""
        if self._host_updates is None:
            return None
        return int(self._count.item()) if self._count is not None else self._host_updates

    @num_updates.setter
    def num_updates(self, value):
        self._host_updates = None if value is None else int(value)
        if value is None:
            self._count = None
        elif self._count is not None:
            self._count.fill_(int(value))

    def _on(self, device):
        """The device counter (created on first use; during a graph capture that is too late) -> its tensor, or None for a constant decay."""
        if self._host_updates is None:
            return None
        if self._count is None or self._count.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ParameterEMA: the counter must exist before a graph capture (one eager update, or FusedAdam.init_state(ema=...))")
            self._count = torch.full((), self.num_updates, dtype=torch.int64, device=device)
        return self._count

    def _workspace(self, device):
        ws = self._workspaces.get(device)
        if ws is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ParameterEMA: the workspace must exist before a graph capture (one eager update, or FusedAdam.init_state(ema=...))")
            ws = torch.zeros(lib.foc_optim_workspace_bytes(MAX_TENSORS) // 4, dtype=torch.int32, device=device)
            self._workspaces[device] = ws
        return ws

    # ---------------------------------------------------------------- update
    def _get_parameters(self, parameters):
        if parameters is None:
            parameters = [p() for p in self._params_refs]
            if any(p is None for p in parameters):
                raise ValueError("(One of) the parameters with which this ExponentialMovingAverage was initialized no longer exists (was "
                                 "garbage collected); please either provide `parameters` explicitly or keep the model to which they belong "
                                 "from being garbage collected.")
            return parameters
        parameters = list(parameters)
        if len(parameters) != len(self.shadow_params):
            raise ValueError("Number of parameters passed as argument is different from number of shadow parameters maintained by this "
                             "ExponentialMovingAverage")
        return parameters

    def _device(self):
        """The device the kernels serve: the counter's, else that of the first shadow on a GPU."""
        if self._count is not None:
            return self._count.device
        for s in self.shadow_params:
            if s.is_cuda:
                return s.device
        return None

    @staticmethod
    def _fused_pair(p, s, device):
        return (device is not None and p.device == device and s.device == device and p.dtype == torch.float32 and s.dtype == torch.float32
                and p.layout == torch.strided and s.layout == torch.strided and p.is_contiguous() and s.is_contiguous() and p.shape == s.shape)

    def _split(self, parameters):
        """(device, [(p, s)] the kernels serve, [(p, s)] for the torch ops)"""
        device = self._device()
        fused, slow = [], []
        for p, s in zip(parameters, self.shadow_params):
            if s.numel() == 0:
                continue
            (fused if self._fused_pair(p, s, device) else slow).append((p, s))
        return device, fused, slow

    def _launch(self, pairs, device, workspace, advance):
        """foc_ema_update over `pairs`, 16 per launch; `advance`: the first launch opens the step (counter + 1, omd into `workspace`)."""
        count = self._on(device)
        stream = stream_of(pairs[0][1])
        for i in range(0, len(pairs), MAX_TENSORS):
            chunk = pairs[i:i + MAX_TENSORS]
            k = len(chunk)
            pa = (ctypes.c_uint64 * k)(*[p.data_ptr() for p, _ in chunk])
            sa = (ctypes.c_uint64 * k)(*[s.data_ptr() for _, s in chunk])
            na = (ctypes.c_int64 * k)(*[s.numel() for _, s in chunk])
            check(lib.foc_ema_update(pa, sa, na, k, float(self.decay), count.data_ptr() if count is not None else None,
                                     1 if (advance and i == 0) else 0, workspace.data_ptr(), workspace.numel() * 4, stream), "ema_update")

    def _torch_rule(self, pairs, advanced):
        """The three torch ops of the rule with the decay derived on the host. Where the counter lives on the device it is read back (a
        synchronisation); `advanced`: a launch of this update has advanced it already."""
        if self._host_updates is None:
            n = None
        elif self._count is not None:
            if not advanced:
                self._count.add_(1)
            n = int(self._count.item())
        else:
            self._host_updates += 1
            n = self._host_updates
        one_minus_decay = _omd(self.decay, n)
        with torch.no_grad():
            for p, s in pairs:
                tmp = s - p
                tmp.mul_(one_minus_decay)
                s.sub_(tmp)

    def update(self, parameters=None):
        """One update of every shadow from its parameter. Device fp32 dense tensors: one launch per 16, no host synchronisation."""
        device, fused, slow = self._split(self._get_parameters(parameters))
        if fused:
            self._launch(fused, device, self._workspace(device), advance=True)
        if slow or not fused:
            self._torch_rule(slow, advanced=bool(fused))

    def _for_step(self, step_params, device):
        """FusedAdam.step(ema=self): -> ({id(p): shadow} of the step's params whose EMA rides in the update launch,
        [(p, s)] for foc_ema_update behind it, [(p, s)] for the torch ops). The counter is on `device` afterwards."""
        if self._device() not in (None, device):
            raise RuntimeError(f"ParameterEMA: the shadows live on {self._device()}, the optimizer's params on {device}")
        self._on(device)
        _, fused, slow = self._split(self._get_parameters(None))
        in_step = {id(p) for p in step_params}
        riding = {id(p): s for p, s in fused if id(p) in in_step}
        return riding, [(p, s) for p, s in fused if id(p) not in in_step], slow

    # ---------------------------------------------------------------- evaluation: torch copies
    def copy_to(self, parameters=None):
        """Copy the averages into the parameters (in place)."""
        for s, p in zip(self.shadow_params, self._get_parameters(parameters)):
            p.data.copy_(s.data)
        _drop_weight_caches()

    def store(self, parameters=None):
        """Save the current parameters for restore()."""
        self.collected_params = [p.detach().clone() for p in self._get_parameters(parameters)]

    def restore(self, parameters=None):
        """Put the parameters of the last store() back (in place)."""
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        for c, p in zip(self.collected_params, self._get_parameters(parameters)):
            p.data.copy_(c.data)
        _drop_weight_caches()

    @contextlib.contextmanager
    def average_parameters(self, parameters=None):
        """`with ema.average_parameters(): evaluate()` — store(), copy_to(), and restore() on the way out."""
        parameters = self._get_parameters(parameters)
        self.store(parameters)
        self.copy_to(parameters)
        try:
            yield
        finally:
            self.restore(parameters)

    def to(self, device=None, dtype=None):
        """Move the shadows and the stored parameters; `dtype` applies to floating-point tensors only. The counter follows `device`."""
        def move(t):
            return t.to(device=device, dtype=dtype) if t.is_floating_point() else t.to(device=device)
        count = self.num_updates
        self.shadow_params = [move(s) for s in self.shadow_params]
        if self.collected_params is not None:
            self.collected_params = [move(c) for c in self.collected_params]
        if self._count is not None and device is not None:
            self._host_updates, self._count = count, None          # made again, where the shadows now are, by the next update
        return

    # ---------------------------------------------------------------- state dict: torch_ema's four keys
    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params,
                "collected_params": self.collected_params}

    def load_state_dict(self, state_dict):
        state_dict = copy.deepcopy(state_dict)
        decay = state_dict["decay"]
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        num_updates = state_dict["num_updates"]
        assert num_updates is None or isinstance(num_updates, int), "Invalid num_updates"
        shadow = state_dict["shadow_params"]
        assert isinstance(shadow, list), "shadow_params must be a list"
        assert all(isinstance(s, torch.Tensor) for s in shadow), "shadow_params must all be Tensors"
        collected = state_dict["collected_params"]
        if collected is not None:
            assert isinstance(collected, list), "collected_params must be a list"
            assert all(isinstance(c, torch.Tensor) for c in collected), "collected_params must all be Tensors"
            assert len(collected) == len(shadow), "collected_params and shadow_params had different lengths"
        if len(shadow) != len(self._params_refs):
            raise ValueError("Tried to `load_state_dict()` with the wrong number of parameters in the saved state.")
        self.decay = decay
        self.num_updates = num_updates
        params = [p() for p in self._params_refs]
        if not any(p is None for p in params):                     # torch_ema: the loaded tensors take the parameters' device and dtype
            shadow = [s.to(device=p.device, dtype=p.dtype) for p, s in zip(params, shadow)]
            if collected is not None:
                collected = [c.to(device=p.device, dtype=p.dtype) for p, c in zip(params, collected)]
        self.shadow_params, self.collected_params = shadow, collected
