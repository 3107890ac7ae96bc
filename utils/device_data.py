"""`from utils.device_data import DevicePatchLoader`: training patches sampled on the device from volumes kept in HBM (see
video-to-video-diffusion_amd/device_data.py).  The reference has no such module; its own `data/` package stays importable."""
import importlib

_m = importlib.import_module("video-to-video-diffusion_amd.device_data")
DeviceVolumeStore = _m.DeviceVolumeStore
DevicePatchSampler = _m.DevicePatchSampler
DevicePatchLoader = _m.DevicePatchLoader
