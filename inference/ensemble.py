"""`from inference.ensemble import EnsembleAccumulator, EnsembleResult`: re-exports the HIP-engine module
(video-to-video-diffusion_amd/ensemble.py)."""
import importlib as _il

_mod = _il.import_module("video-to-video-diffusion_amd.ensemble")
globals().update({k: v for k, v in vars(_mod).items() if not k.startswith("__")})
