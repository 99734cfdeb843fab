// plan.h — what the host side (zdr_api.cpp) asks of the gather-plan kernels (zdr_plan.hip): the transpose of a texel gather — bilinear,
// mip or anisotropic — laid out once as CSR rows per destination pixel (zdr_gather_plan_count, zdr_gather_plan_build) and applied as a
// gather, without a float atomic and in a defined summation order (zdr_gather_plan_apply; include/zdr.h).  Like the mip and the aniso
// kernels these live in a translation unit and a library of their own (libzdr_plan.so, a dependency of libzdr_hip.so): nothing here is
// seen by any other kernel's object file.  The pyramid's layout is zdr_image_pyramid's (csrc/mip.h, zdr_mip_plan), unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "texel_filter.h"                 // the filters' numbers; ZDR_FILTER_MAX_TEXELS and ZDR_FILTER_MAX_PIXELS bound a plan: a row index fits 32 bits

#define ZDR_PLAN_MAX_NNZ 0x7fffffffull    // entry ids fit an int32
#define ZDR_PLAN_BLOCK 256                // texels of one workgroup of the enumeration
#define ZDR_PLAN_HEADER_BYTES 256         // the workspace begins with nnz as a uint64
#define ZDR_PLAN_LONG_ROW 64              // a row of at least this many entries is summed by a whole wave

enum { ZDR_PLAN_BILINEAR = TF_BILINEAR, ZDR_PLAN_MIP = TF_MIP, ZDR_PLAN_ANISO = TF_ANISO };   // zdr_gather_plan_params.filter

// Wave-uniform arguments of the enumeration (the count and the fill).
struct PlanEnumArgs {
    const float4 *view;               // (tex_h, tex_w, 8) floats: floats 0 (visible), 2, 3 (X, Y) and, for mip, 6 (scale) are read
    const float4 *foot;               // aniso: (tex_h, tex_w, 4) floats, the footprint buffer
    uint32_t ntexels, nblocks;        // nblocks = ceil(ntexels / ZDR_PLAN_BLOCK)
    int32_t filter, width, height, L, max_aniso;
    float footprint;
    uint32_t p0;                      // width * height: where the rows of the levels >= 1 begin
};

// The build's workspace, as zdr_plan_workspace lays it out (every part begins at a multiple of 256 bytes).
struct PlanWorkspace {
    uint64_t *nnz;                    // header: the number of entries
    uint32_t *block_off;              // nblocks: the first entry id of each workgroup of the enumeration
    uint32_t *keys, *keys_sorted;     // nnz each: the destination row of each entry, in entry-id order and sorted
    uint64_t *vals;                   // nnz: (texel, weight) in entry-id order
    void *sort_temp;                  // what the radix sort asks for
    size_t sort_temp_bytes, bytes;
};

// Wave-uniform arguments of the apply.
struct PlanApplyArgs {
    const uint32_t *row_start;        // rows + 1
    const uint2 *entries;             // (texel, weight bits)
    const float *d_color;             // (tex_h, tex_w, 4)
    float *d_image;                   // rows 0 .. p0 - 1, added into
    float *d_pyramid;                 // rows p0 .. rows - 1, written
    uint32_t p0, rows;
};

// ZDR_PLAN_LAUNCHER_REF: as ZDR_MIP_LAUNCHER_REF of mip.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library linked
// without libzdr_plan.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_PLAN_LAUNCHER_REF
#define ZDR_PLAN_LAUNCHER_REF
#endif
// bytes the stable sort of n (key, value) pairs with keys below `rows` needs; 0 with *ok = 0 if the query fails (no device).  Host only.
ZDR_PLAN_LAUNCHER_REF size_t zdr_plan_sort_temp_bytes(uint64_t n, uint32_t rows, int *ok);
// two launches on `stream`: the entries of every workgroup of 256 texels, then their running sum; leaves nnz in W.nnz.
ZDR_PLAN_LAUNCHER_REF int zdr_launch_plan_count(const PlanEnumArgs &E, const PlanWorkspace &W, hipStream_t stream);
// the count again, the fill, the stable sort by row and the row starts, on `stream`.  No allocation, no synchronisation.
ZDR_PLAN_LAUNCHER_REF int zdr_launch_plan_build(const PlanEnumArgs &E, const PlanWorkspace &W, uint32_t nnz, uint32_t rows, uint32_t *row_start, uint64_t *entries,
                                                hipStream_t stream);
// two launches on `stream`: the rows below ZDR_PLAN_LONG_ROW entries, sixteen lanes a row, and the others, a wave a row.
ZDR_PLAN_LAUNCHER_REF int zdr_launch_plan_apply(const PlanApplyArgs &A, hipStream_t stream);
