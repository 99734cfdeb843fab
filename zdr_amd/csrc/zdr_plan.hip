// zdr_plan.hip — the gather plan for gfx950 (include/zdr.h: zdr_gather_plan_count, zdr_gather_plan_build, zdr_gather_plan_apply): the
// transpose of a texel gather with the view held fixed, laid out once as CSR rows per destination pixel and then applied as a gather —
// no float atomic, a defined summation order, the same bits from run to run.  Linked into libzdr_plan.so (zdr_amd/build.py), compiled
// without contraction: the weights are the scatter kernels' own products and the sums are defined by the operation order of
// include/zdr.h.
//
// The build, once per (view, image size, filter):
//   k_plan_count       thread = texel: how many taps its scatter kernel touches; a workgroup of 256 texels adds them up (integer atomics
//                      in LDS: the sum does not depend on their order)
//   k_plan_scan        ONE workgroup: the running sum of the workgroups' counts, and nnz into the workspace's header
//   k_plan_fill        thread = texel: its entries, in the scatter kernel's order, at the texel's place in that running sum — the entry
//                      id — as (row, (texel, weight))
//   (the stable radix sort of rocPRIM by row: within a row the entries stay in entry-id order)
//   k_plan_rows        thread = row: where the row begins, a binary search in the sorted rows
// The apply, every step (k_plan_apply, two instantiations, one launch each):
//   short rows         (fewer than 64 entries: minification gives millions of them)  sixteen lanes a row, lane = 4 q + c: channel c, the
//                      sub-sums q, q + 4, q + 8, q + 12 of the header's sixteen; the tree's first two steps are in the lane, the last two
//                      are shuffles over lane xor 8 and 4
//   long rows          (magnification gives thousands of rows of hundreds to thousands of entries)  a wave a row, lane = 4 j + c, one
//                      sub-sum a lane, four entries in flight per lane; the tree is shuffles over lane xor 32, 16, 8, 4
// A row is owned by the lanes that sum it, every store is a plain store of its owner: no atomics, no scratch, the same bits whatever the
// grid and the launch order.  The four channel lanes of a sub-sum read the same entry (8 bytes, one request) and 16 contiguous bytes of
// d_color.
//
// The enumeration is tf_enumerate (texel_filter.h), the very walk the scatter kernels of zdr_project.hip, zdr_mip.hip and zdr_aniso.hip run
// with an atomic add as its emit: the fill's emit stores (row, (texel, weight)) instead.  Why one weight formula has the bits of all
// three kernels is argued there.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include "plan.h"

#define ZD __device__ __forceinline__

// ---------------------------------------------------------------------------------------------------------------- what a texel enumerates
// the state the scatter kernel of E.filter forms for texel t (texel_filter.h); an invisible texel reads nothing else and has no entry
ZD tf_texel_t pl_texel(const PlanEnumArgs &E, uint32_t t) {
    const float4 vw = E.view[2 * (size_t)t];                 // {visible, cosine, X, Y}
    tf_texel_t x = tf_texel(vw.x, vw.z, vw.w);
    if (!tf_on(vw.x)) return x;
    if (E.filter == ZDR_PLAN_MIP) {
        const float scale = ((const float *)E.view)[8 * (size_t)t + 6];
        x.lv = tf_level(scale * E.footprint, E.L);
    } else if (E.filter == ZDR_PLAN_ANISO) {
        const float4 fp = E.foot[t];                         // {major axis x, y, minor, major}
        const tf_probes_t pr = tf_probes(fp.z, fp.w, E.footprint, E.max_aniso);
        x.N = pr.N; x.ax = fp.x; x.ay = fp.y;
        x.lv = tf_level(pr.s, E.L);
    }
    return x;
}

ZD uint32_t pl_count(const tf_texel_t &x) { return tf_on(x.visible) ? (uint32_t)x.N * (x.lv.f != 0.0f ? 8u : 4u) : 0u; }

// ------------------------------------------------------------------------------------------------------------------------- the build
__global__ __launch_bounds__(ZDR_PLAN_BLOCK) void k_plan_count(PlanEnumArgs E, uint32_t *block_off) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0u) total = 0u;
    __syncthreads();
    const uint32_t t = blockIdx.x * ZDR_PLAN_BLOCK + threadIdx.x;
    const uint32_t n = t < E.ntexels ? pl_count(pl_texel(E, t)) : 0u;
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0u) block_off[blockIdx.x] = total;            // (blockIdx.x < nblocks: the grid is nblocks)
}

// in place: the counts of the n workgroups become their running sum (exclusive, modulo 2^32: the host refuses a plan beyond
// ZDR_PLAN_MAX_NNZ before anything is written through it); the total, in 64 bits, goes to *nnz
__global__ __launch_bounds__(256) void k_plan_scan(uint32_t *block_off, uint32_t n, uint64_t *nnz) {
    __shared__ uint64_t part[256];
    const uint32_t seg = (n + 255u) / 256u, b = threadIdx.x * seg, e = b + seg < n ? b + seg : n;
    uint64_t sum = 0;
    for (uint32_t i = b; i < e; i++) sum += block_off[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    uint64_t base = 0;
    for (uint32_t k = 0; k < threadIdx.x; k++) base += part[k];
    if (threadIdx.x == 255u) *nnz = base + sum;
    for (uint32_t i = b; i < e; i++) { const uint32_t c = block_off[i]; block_off[i] = (uint32_t)base; base += c; }
}

__global__ __launch_bounds__(ZDR_PLAN_BLOCK) void k_plan_fill(PlanEnumArgs E, const uint32_t *__restrict__ block_off, uint32_t nnz, uint32_t *__restrict__ keys,
                                                              uint64_t *__restrict__ vals) {
    __shared__ uint32_t cnt[ZDR_PLAN_BLOCK];
    const uint32_t t = blockIdx.x * ZDR_PLAN_BLOCK + threadIdx.x;
    tf_texel_t x = tf_texel(0.0f, 0.0f, 0.0f);                       // (a thread beyond the last texel: invisible)
    if (t < E.ntexels) x = pl_texel(E, t);
    cnt[threadIdx.x] = pl_count(x);
    __syncthreads();
    if (!tf_on(x.visible)) return;
    uint32_t at = block_off[blockIdx.x];
    for (uint32_t k = 0; k < threadIdx.x; k++) at += cnt[k];
    // a destination's row: the pixels of the image first, then, from p0 on, the pixels of the packed levels >= 1
    tf_enumerate(x, E.filter, E.footprint, E.width, E.height, [&](bool pyramid, uint32_t pixel, float weight) {
        if (at < nnz) {                                              // (a caller's nnz below the true one: the entries beyond it are dropped, not written)
            keys[at] = (pyramid ? E.p0 : 0u) + pixel;
            vals[at] = (uint64_t)t | ((uint64_t)__float_as_uint(weight) << 32);
        }
        at++;
    });
}

// row_start[r] = the first sorted entry whose row is not below r; r = rows gives nnz
__global__ __launch_bounds__(256) void k_plan_rows(const uint32_t *__restrict__ keys_sorted, uint32_t nnz, uint32_t rows, uint32_t *__restrict__ row_start) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > rows) return;
    uint32_t lo = 0u, hi = nnz;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys_sorted[mid] < r) lo = mid + 1u; else hi = mid;
    }
    row_start[r] = lo;
}

// ------------------------------------------------------------------------------------------------------------------------- the apply
template <bool LONG>
__global__ __launch_bounds__(256) void k_plan_apply(PlanApplyArgs A) {
    if (LONG) {
        const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u, j = lane >> 2, c = lane & 3u;
        if (r >= A.rows) return;                                     // (wave-uniform, like the next one)
        const uint32_t b = A.row_start[r], e = A.row_start[r + 1u];
        if (e - b < ZDR_PLAN_LONG_ROW) return;
        float s = 0.0f;
        for (uint32_t k0 = b; k0 < e; k0 += 64u) {
            float p[4];
            bool has[4];
            uint2 en[4];                                             // the four entries first, then the four colours: eight loads in flight
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t k = k0 + 16u * (uint32_t)u + j;
                has[u] = k < e;
                en[u] = A.entries[has[u] ? k : e - 1u];              // (no branch around the loads: a lane past the end reads the row's last entry and drops it)
            }
#pragma unroll
            for (int u = 0; u < 4; u++) p[u] = __uint_as_float(en[u].y) * A.d_color[4 * (size_t)en[u].x + c];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (has[u]) s = s + p[u];
        }
        s = s + __shfl_xor(s, 32);
        s = s + __shfl_xor(s, 16);
        s = s + __shfl_xor(s, 8);
        s = s + __shfl_xor(s, 4);
        if (j == 0u) {
            if (r < A.p0) { float *d = A.d_image + 4 * (size_t)r + c; *d = *d + s; }
            else A.d_pyramid[4 * (size_t)(r - A.p0) + c] = s;
        }
    } else {
        const uint32_t r = blockIdx.x * 16u + (threadIdx.x >> 4), q = (threadIdx.x >> 2) & 3u, c = threadIdx.x & 3u;
        const bool live = r < A.rows;                                // (the sixteen lanes of a row agree on everything below)
        uint32_t b = 0u, e = 0u;
        if (live) { b = A.row_start[r]; e = A.row_start[r + 1u]; }
        const uint32_t R = e - b;
        const bool mine = live && R < ZDR_PLAN_LONG_ROW;
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (mine) {
            for (uint32_t k0 = b; k0 < e; k0 += 16u) {
                float p[4];
                bool has[4];
                uint2 en[4];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const uint32_t k = k0 + 4u * (uint32_t)m + q;
                    has[m] = k < e;
                    en[m] = A.entries[has[m] ? k : e - 1u];          // (as in the long rows; e > b here)
                }
#pragma unroll
                for (int m = 0; m < 4; m++) p[m] = __uint_as_float(en[m].y) * A.d_color[4 * (size_t)en[m].x + c];
#pragma unroll
                for (int m = 0; m < 4; m++)
                    if (has[m]) s[m] = s[m] + p[m];
            }
        }
        float v = (s[0] + s[2]) + (s[1] + s[3]);                     // s_j + s_{j+8}, then + s_{j+4}
        v = v + __shfl_xor(v, 8);
        v = v + __shfl_xor(v, 4);
        if (mine && q == 0u) {
            if (r < A.p0) { if (R) { float *d = A.d_image + 4 * (size_t)r + c; *d = *d + v; } }
            else A.d_pyramid[4 * (size_t)(r - A.p0) + c] = v;        // (an empty row: the tree of sixteen zeros, 0)
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ launchers
// the bits of the largest key: the rows 0 .. rows - 1, and `rows` itself, which marks a place beyond the last entry
static int plan_key_bits(uint32_t rows) {
    int bits = 1;
    while (bits < 32 && rows >> bits) bits++;
    return bits;
}

size_t zdr_plan_sort_temp_bytes(uint64_t n, uint32_t rows, int *ok) {
    size_t bytes = 0;
    *ok = 1;
    if (n == 0) return 0;
    const hipError_t rc = rocprim::radix_sort_pairs((void *)nullptr, bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr,
                                                    (size_t)n, 0u, (unsigned)plan_key_bits(rows), (hipStream_t)0);
    if (rc != hipSuccess) { (void)hipGetLastError(); *ok = 0; return 0; }
    return bytes ? bytes : 16;
}

int zdr_launch_plan_count(const PlanEnumArgs &E, const PlanWorkspace &W, hipStream_t st) {
    hipLaunchKernelGGL(k_plan_count, dim3(E.nblocks), dim3(ZDR_PLAN_BLOCK), 0, st, E, W.block_off);
    if (hipGetLastError() != hipSuccess) return -1;                  // the next launch would read what this one did not write
    hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(256), 0, st, W.block_off, E.nblocks, W.nnz);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_plan_build(const PlanEnumArgs &E, const PlanWorkspace &W, uint32_t nnz, uint32_t rows, uint32_t *row_start, uint64_t *entries, hipStream_t st) {
    if (zdr_launch_plan_count(E, W, st)) return -1;
    if (nnz) {
        // every key is `rows` first: with a caller's nnz above the true one the places the fill does not reach sort behind every row,
        // so that row_start ends at the true count and no row holds an entry that was never written
        if (hipMemsetD32Async((hipDeviceptr_t)W.keys, (int)rows, nnz, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(k_plan_fill, dim3(E.nblocks), dim3(ZDR_PLAN_BLOCK), 0, st, E, (const uint32_t *)W.block_off, nnz, W.keys, W.vals);
        if (hipGetLastError() != hipSuccess) return -1;
        size_t temp = W.sort_temp_bytes;
        if (rocprim::radix_sort_pairs(W.sort_temp, temp, (uint32_t *)W.keys, W.keys_sorted, (uint64_t *)W.vals, entries, (size_t)nnz, 0u, (unsigned)plan_key_bits(rows),
                                      st) != hipSuccess)
            return -1;
    }
    hipLaunchKernelGGL(k_plan_rows, dim3(rows / 256u + 1u), dim3(256), 0, st, (const uint32_t *)W.keys_sorted, nnz, rows, row_start);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_plan_apply(const PlanApplyArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_plan_apply<false>, dim3((A.rows + 15u) / 16u), dim3(256), 0, st, A);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_plan_apply<true>, dim3((A.rows + 3u) / 4u), dim3(256), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
