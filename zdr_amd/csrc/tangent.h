// tangent.h — what the host side (zdr_api.cpp) asks of the UV-tangent kernels (zdr_tangent.hip): the per-texel tangent buffer of
// zdr_scene_texel_tangents and the footprint ellipse of a texel's TRUE patch, the parallelogram its tangents span
// (zdr_texel_footprint_tangents; include/zdr.h).  Like the other texture-space kernels these live in a translation unit and a library of
// their own (libzdr_tangent.so, a dependency of libzdr_hip.so): libzdr_texel.so and libzdr_aniso.so keep exactly the kernels they had.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "texel.h"
#include "aniso.h"

// ZDR_TANGENT_LAUNCHER_REF: as ZDR_TEXEL_LAUNCHER_REF of texel.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_tangent.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_TANGENT_LAUNCHER_REF
#define ZDR_TANGENT_LAUNCHER_REF
#endif
// one launch on `stream` each.  No allocation, no synchronisation.
// The resolve reads A.keys and A.aovs as zdr_launch_texel_aovs(A, stream) left them (the same stream, before this call) and writes
// tangents, (tex_h, tex_w, 8) floats.
ZDR_TANGENT_LAUNCHER_REF int zdr_launch_texel_tangents(const TexelArgs &A, float4 *tangents, hipStream_t stream);
// A as for zdr_launch_texel_footprint; tangents (tex_h, tex_w, 8) floats.
ZDR_TANGENT_LAUNCHER_REF int zdr_launch_texel_footprint_tangents(const AnisoFootprintArgs &A, const float4 *tangents, hipStream_t stream);
