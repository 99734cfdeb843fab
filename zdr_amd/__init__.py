"""zdr_amd — MI355X-native differentiable path tracer behind the reference's Python API
(``from zdr import Scene, Camera, float3``; /root/reference/__init__.py:1)."""
from .denoiser import denoise
from .mip import ImagePyramid, image_pyramid, image_pyramid_backward, image_pyramid_forward, pyramid_layout
from .project import (texel_footprint_forward, texel_gather, texel_gather_aniso_backward, texel_gather_aniso_forward, texel_gather_backward,
                      texel_gather_dview, texel_gather_forward, texel_gather_mip_backward, texel_gather_mip_forward)
from .plan import GatherPlan, gather_plan
from .pushpull import push_pull
from .mathtypes import Camera, float3, float4x4
from .render import Aovs, Scene, TexelAovs, TexelBounce, TexelFootprint, TexelLighting, TexelProjection, TexelTangents, TexelView

__all__ = ["Scene", "Aovs", "TexelAovs", "TexelLighting", "Camera", "float3", "float4x4", "denoise", "push_pull",
           "TexelView", "TexelProjection", "texel_gather", "texel_gather_forward", "texel_gather_backward",
           "GatherPlan", "gather_plan", "texel_gather_dview", "TexelTangents", "TexelBounce"]
