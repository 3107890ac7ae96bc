"""Drop-in for the reference's `inference` package (reference inference/__init__.py:1-3)."""
import importlib as _il

_pkg = _il.import_module("video-to-video-diffusion_amd")
DDIMSampler = _pkg.DDIMSampler
DDPMSampler = _pkg.DDPMSampler
DPMSolverSampler = _pkg.DPMSolverSampler   # additive: DPM-Solver++(2M), not in the reference
HeunSampler = _pkg.HeunSampler             # additive: EDM Heun / Euler on Karras sigmas, not in the reference

__all__ = ['DDIMSampler', 'DDPMSampler', 'DPMSolverSampler', 'HeunSampler']
