"""`from inference.measurement_guidance import MeasurementGuidance`: re-exports the HIP-engine module
(video-to-video-diffusion_amd/measurement_guidance.py)."""
import importlib as _il

_mod = _il.import_module("video-to-video-diffusion_amd.measurement_guidance")
globals().update({k: v for k, v in vars(_mod).items() if not k.startswith("__")})
