"""zdr_amd — MI355X-native differentiable path tracer behind the reference's Python API
(``from zdr import Scene, Camera, float3``; /root/reference/__init__.py:1)."""
from .denoiser import denoise
from .pushpull import push_pull
from .mathtypes import Camera, float3, float4x4
from .render import Aovs, Scene, TexelAovs, TexelLighting

__all__ = ["Scene", "Aovs", "TexelAovs", "TexelLighting", "Camera", "float3", "float4x4", "denoise", "push_pull"]
