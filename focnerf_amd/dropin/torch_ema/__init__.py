"""`from torch_ema import ExponentialMovingAverage` for the reference trainer (nerf/utils.py:30, :739) when focnerf_amd/dropin is on the
path: the class is focnerf_amd.ParameterEMA — torch_ema 0.3's constructor, methods (update, copy_to, store, restore, average_parameters,
to, state_dict, load_state_dict) and state-dict layout, so the trainer's lines and its checkpoints stay as they are. `ema.update()` runs
on the library's kernel for fp32 device parameters; `optimizer.step(ema=ema)` with focnerf_amd.FusedAdam takes it inside the Adam launch."""
from focnerf_amd.ema import ParameterEMA as ExponentialMovingAverage

__all__ = ["ExponentialMovingAverage"]
