"""Deterministic mode: bit-reproducible training steps (the library switch FOC_DETERMINISTIC, include/focnerf.h "Deterministic mode").

Off by default. With it on, the kernels that otherwise sum in arrival order (the binned grid backward's chunks, the background
model's table gradient, the density grid's mean, the split-K MLP weight gradient) take a form whose result does not depend on timing,
and the entry points that have no such form refuse with a RuntimeError that names FOC_DETERMINISTIC. Same GPU model, same build, same
inputs, same seeds and same option values then give the same bits on every run (INTEGRATION.md section 4 lists the covered paths).

    import focnerf_amd
    focnerf_amd.use_deterministic(True)
    with focnerf_amd.deterministic():          # or for a block; the previous value comes back on exit
        ...

The mode is NOT tied to torch's own flag (that would change behaviour for whoever has the flag on today); to link the two:

    focnerf_amd.use_deterministic(torch.are_deterministic_algorithms_enabled())

The environment variable FOC_DETERMINISTIC=1 sets the initial value, like every library switch. Workspace sizes grow with the mode:
set it before the first step (and before capturing a graph), not between a forward pass and its backward."""
from . import _lib

OPTION = "FOC_DETERMINISTIC"


def use_deterministic(flag=True):
    """Switch deterministic mode on or off for the rest of the process."""
    _lib.set_option(OPTION, 1 if flag else 0)


def is_deterministic():
    """True when deterministic mode is on."""
    return _lib.get_option(OPTION) != 0


class deterministic:
    """`with deterministic(): ...` — the mode set for the block; the value it had before comes back on exit, also after an exception."""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.old = _lib.get_option(OPTION)
        _lib.set_option(OPTION, 1 if self.flag else 0)
        return self

    def __exit__(self, *exc):
        _lib.set_option(OPTION, self.old)
        return False
