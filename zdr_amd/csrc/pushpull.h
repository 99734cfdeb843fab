// pushpull.h — what the host side (zdr_api.cpp) asks of the push-pull kernels (zdr_pushpull.hip): the hole filling of zdr_push_pull and
// its adjoint (include/zdr.h).  Like the texture-space kernels these live in a translation unit and a library of their own
// (libzdr_pushpull.so, a dependency of libzdr_hip.so): nothing here is seen by any other kernel's object file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZDR_PUSHPULL_MAX_TEXELS (1u << 26)   // the cap of zdr_scene_texel_aovs
#define ZDR_PUSHPULL_MAX_LEVELS 32           // 2^26 texels in one row still end after 26 halvings
#define ZDR_PUSHPULL_TAIL_DIM 32             // a level of at most 32 x 32 and everything above it is one workgroup's work, in LDS
#define ZDR_PUSHPULL_TAIL_TEXELS 1368        // 32^2 + 16^2 + ... + 1 = 1365, rounded up to a multiple of 8

// The pyramid of one call: sizes of the levels 0 .. L and where the levels >= 1 sit in the workspace.  A level holds one float4 per texel
// (p, then y in place; G, then q in place for the adjoint) and two floats (a and r), each array rounded up to 16 bytes.
struct PushPullPlan {
    int32_t L;                                       // the top level
    int32_t tail;                                    // the first level <= L that fits the fused tail, L + 1 if none does
    int32_t w[ZDR_PUSHPULL_MAX_LEVELS], h[ZDR_PUSHPULL_MAX_LEVELS];
    size_t v_off[ZDR_PUSHPULL_MAX_LEVELS], a_off[ZDR_PUSHPULL_MAX_LEVELS], r_off[ZDR_PUSHPULL_MAX_LEVELS];   // bytes; [0] unused
    size_t bytes;                                    // of the workspace, never 0
};

static inline PushPullPlan zdr_push_pull_plan(int32_t width, int32_t height, int32_t levels) {
    PushPullPlan P;
    P.L = 0; P.w[0] = width; P.h[0] = height;
    P.v_off[0] = P.a_off[0] = P.r_off[0] = 0;
    size_t off = 16;                                 // (a 1 x 1 texture has no level >= 1: the size is still not 0)
    while ((P.w[P.L] > 1 || P.h[P.L] > 1) && (levels <= 0 || P.L < levels) && P.L + 1 < ZDR_PUSHPULL_MAX_LEVELS) {
        const int l = ++P.L;
        P.w[l] = (P.w[l - 1] + 1) / 2; P.h[l] = (P.h[l - 1] + 1) / 2;
        const size_t n = (size_t)P.w[l] * (size_t)P.h[l], scalar = (n * sizeof(float) + 15) & ~(size_t)15;
        P.v_off[l] = off; off += n * sizeof(float4);
        P.a_off[l] = off; off += scalar;
        P.r_off[l] = off; off += scalar;
    }
    P.tail = P.L + 1;
    for (int l = 0; l <= P.L; l++)
        if (P.w[l] <= ZDR_PUSHPULL_TAIL_DIM && P.h[l] <= ZDR_PUSHPULL_TAIL_DIM) { P.tail = l; break; }
    P.bytes = off;
    return P;
}

struct PushPullArgs {
    int32_t width, height, levels;
    const float *weight;             // (H, W)
    const float4 *in;                // (H, W, 4): x, or d_out for the adjoint
    float4 *out;                     // (H, W, 4): y, or d_x
    void *workspace;
};

// ZDR_PUSHPULL_LAUNCHER_REF: as ZDR_TEXEL_LAUNCHER_REF of texel.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_pushpull.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_PUSHPULL_LAUNCHER_REF
#define ZDR_PUSHPULL_LAUNCHER_REF
#endif
// every launch of one pass on `stream`: the up-sweep level by level, the fused tail, the down-sweep.  No allocation, no synchronisation.
ZDR_PUSHPULL_LAUNCHER_REF int zdr_launch_push_pull(const PushPullArgs &A, int backward, hipStream_t stream);
