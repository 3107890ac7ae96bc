"""`from inference.consistency import DataConsistency, SliceProfile`: re-exports the HIP-engine module
(video-to-video-diffusion_amd/consistency.py)."""
import importlib as _il

_mod = _il.import_module("video-to-video-diffusion_amd.consistency")
globals().update({k: v for k, v in vars(_mod).items() if not k.startswith("__")})
