"""Drop-in for tiny-cuda-nn's PyTorch bindings (`import tinycudann as tcnn`)."""
from focnerf_amd.tcnn import Encoding, Network, NetworkWithInputEncoding  # noqa: F401
