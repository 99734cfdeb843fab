// zdr_envmap.hip — rebuilds the environment map's importance-sampling tables on the device (include/zdr.h,
// zdr_scene_update_envmap_sampling) for gfx950: the device form of zdr_amd/envmap.py, build_tables.
//
// Four kernels, launched one after the other on the caller's stream (each needs all of the one before):
//   k_env_weight    one lane per texel of the 512 x 256 sample map: 17 x 17 Gaussian taps of luminance x sin(theta), each a bilinear
//                   clamp-to-edge lookup of the scene's texture (scene.h, env_lookup), in float32 and in the host's order of operations;
//                   every workgroup also leaves the sum of its 256 weights, in double;
//   k_env_rows      one wave per row: the map's mean from the 512 partial sums (the same fixed order in every workgroup and every run, no
//                   float atomics), MIS compensation, then the row's Vose alias table with the weights, the probabilities, the aliases
//                   and the two work lists in LDS (12 KiB);
//   k_env_marginal  one wave: the same table over the 256 row averages;
//   k_env_pdf       one lane per texel: pdf = p(x|y) p(y) W H.
// Tables are built in float64 like the host's Python floats and stored as float32.  The work lists are filled in index order (ballot +
// prefix count) and paired from their ends by one lane, which is what create_alias_table does: the 257 tables are independent, the
// parallelism is across rows.  Every loop of the pairing is bounded by the table's size.  No scratch memory
// (tests/test_envmap_sampling_resources.py).
#include "envsample.h"

#define EW ZDR_ENVS_W
#define EH ZDR_ENVS_H
#define ENV_PI 3.14159265358979323846f

__device__ __forceinline__ int env_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the same value in every lane: a + b is commutative, so both partners of a butterfly step compute the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(ZDR_ENVS_BLOCK) void k_env_weight(EnvSamplingArgs A) {
    __shared__ double wave_part[ZDR_ENVS_BLOCK / 64];
    const int idx = (int)blockIdx.x * ZDR_ENVS_BLOCK + (int)threadIdx.x;         // the grid covers the map exactly
    const int x = idx & (EW - 1), y = idx / EW;
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const float *__restrict__ taps = A.scratch->taps;
    const float4 *__restrict__ tex = A.tex;
    const int eh = A.env_h, ew = A.env_w;
    float sum = 0.f;
#pragma unroll 1
    for (int dy = 0; dy < ZDR_ENVS_TAPS; dy++) {
        const float v = (cy + (float)(dy - ZDR_ENVS_TAPS / 2) * 0.125f) * (1.0f / EH);    // exact: v may leave [0, 1] by one texel
        const float sv = sinf(v * ENV_PI);
        const float ty = v * (float)eh - 0.5f, y0f = floorf(ty), fy = ty - y0f;
        const int y0 = env_clampi((int)y0f, 0, eh - 1), y1 = env_clampi((int)y0f + 1, 0, eh - 1);
        const float4 *r0 = tex + (size_t)y0 * (size_t)ew, *r1 = tex + (size_t)y1 * (size_t)ew;
#pragma unroll
        for (int dx = 0; dx < ZDR_ENVS_TAPS; dx++) {
            const float u = (cx + (float)(dx - ZDR_ENVS_TAPS / 2) * 0.125f) * (1.0f / EW);
            const float tx = u * (float)ew - 0.5f, x0f = floorf(tx), fx = tx - x0f;
            const int x0 = env_clampi((int)x0f, 0, ew - 1), x1 = env_clampi((int)x0f + 1, 0, ew - 1);
            const float4 c00 = r0[x0], c10 = r0[x1], c01 = r1[x0], c11 = r1[x1];
            const float tr = c00.x + (c10.x - c00.x) * fx, tg = c00.y + (c10.y - c00.y) * fx, tb = c00.z + (c10.z - c00.z) * fx;
            const float br = c01.x + (c11.x - c01.x) * fx, bg = c01.y + (c11.y - c01.y) * fx, bb = c01.z + (c11.z - c01.z) * fx;
            const float r = tr + (br - tr) * fy, g = tg + (bg - tg) * fy, b = tb + (bb - tb) * fy;
            const float lum = 0.212671f * r + 0.715160f * g + 0.072169f * b;
            sum += taps[dy * ZDR_ENVS_TAPS + dx] * fminf(lum * sv, 1e8f);
        }
    }
    const float s = sum / taps[ZDR_ENVS_TAPS * ZDR_ENVS_TAPS];
    A.scratch->scale[idx] = s;
    const double ws = wave_sum((double)s);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < ZDR_ENVS_BLOCK / 64; k++) t += wave_part[k];
        A.scratch->partial[blockIdx.x] = t;
    }
}

// Vose's alias table of the N values w[] (LDS), by ONE wave, as zdr_amd/envmap.py:create_alias_table builds it: prob = w N / total,
// entries above and below 1 listed in index order, paired from the ends of the two lists.  A table whose total is 0 is uniform.
// What is left in a list when the other runs out gets prob 1 — except an entry whose weight is exactly 0 in a table with a positive
// total: it keeps prob 0 and takes the heaviest entry as its alias, so a texel whose pdf is 0 is never drawn.  (In exact arithmetic a
// zero weight is never left over: the deficits of the entries below 1 add up to the excess of those above.)
// Returns sum |w| (total) and sum w (sum); writes prob (clamped to [0, 1]) and alias.
template <int N>
__device__ __forceinline__ void alias_table(const float *w, double *prob, int *alias, int *over, int *under, float *__restrict__ out_prob,
                                            int32_t *__restrict__ out_alias, double &total, double &sum) {
    static_assert(N % 64 == 0, "one wave, N / 64 entries per lane");
    const int lane = (int)threadIdx.x;
    double t = 0.0, sg = 0.0;
    float best = w[lane]; int best_i = lane;
    for (int i = lane; i < N; i += 64) {
        const float v = w[i];
        t += fabs((double)v); sg += (double)v;
        if (v > best) { best = v; best_i = i; }
    }
    t = wave_sum(t); sg = wave_sum(sg);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {                              // heaviest entry, the lowest index among equals
        const float ob = __shfl_xor(best, m, 64); const int oi = __shfl_xor(best_i, m, 64);
        if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
    }
    const double ratio = t > 0.0 ? (double)N / t : 1.0;
    const unsigned long long below = (1ull << lane) - 1ull;
    int no = 0, nu = 0;
    for (int c = 0; c < N; c += 64) {
        const int i = c + lane;
        const double p = (double)w[i] * ratio;
        prob[i] = p; alias[i] = i;
        const unsigned long long mo = __ballot(p > 1.0), mu = __ballot(p < 1.0);
        if (p > 1.0) over[no + __popcll(mo & below)] = i;            // (no + count <= N: an entry is in one list at most)
        if (p < 1.0) under[nu + __popcll(mu & below)] = i;
        no += __popcll(mo); nu += __popcll(mu);
    }
    __syncthreads();
    if (lane == 0) {
        // a trip pops one entry of each list and pushes one at most, onto the list it popped from or the other: neither list outgrows its
        // first length, and the loop ends within 2 N trips
        for (int trip = 0; trip < 2 * N && no > 0 && nu > 0; trip++) {
            const int o = over[--no], u = under[--nu];
            const double po = prob[o] - (1.0 - prob[u]);
            prob[o] = po; alias[u] = o;
            if (po > 1.0) over[no++] = o;
            else if (po < 1.0) under[nu++] = o;
        }
        for (int k = 0; k < no; k++) { const int i = over[k]; prob[i] = 1.0; alias[i] = i; }
        for (int k = 0; k < nu; k++) {
            const int i = under[k];
            if (t > 0.0 && w[i] == 0.0f) { prob[i] = 0.0; alias[i] = best_i; }
            else { prob[i] = 1.0; alias[i] = i; }
        }
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        out_prob[i] = fminf(fmaxf((float)prob[i], 0.0f), 1.0f);
        out_alias[i] = alias[i];
    }
    total = t; sum = sg;
}

__global__ __launch_bounds__(64) void k_env_rows(EnvSamplingArgs A) {
    __shared__ float w[EW];
    __shared__ double prob[EW];
    __shared__ int alias[EW], over[EW], under[EW];
    const int y = (int)blockIdx.x, lane = (int)threadIdx.x;          // the grid has EH workgroups
    EnvSamplingScratch *S = A.scratch;
    float sub = 0.f;
    if (A.compensate_mis) {                                          // (wave-uniform) envmap.py:167-175
        double s = 0.0;
        for (int i = lane; i < ZDR_ENVS_PARTIALS; i += 64) s += S->partial[i];
        const float mean = (float)(wave_sum(s) / (double)(EW * EH));
        sub = (float)((double)mean * S->row_factor[y]);
    }
    float *row = S->scale + (size_t)y * EW;
    for (int i = lane; i < EW; i += 64) {
        float v = row[i];
        if (A.compensate_mis) { v = fmaxf(v - sub, 0.0f); row[i] = v; }   // k_env_pdf reads the weights the table was built from
        w[i] = v;
    }
    __syncthreads();
    double total, sum;
    alias_table<EW>(w, prob, alias, over, under, A.alias_prob + EH + (size_t)y * EW, A.alias_idx + EH + (size_t)y * EW, total, sum);
    if (lane == 0) { S->row_total[y] = total; S->row_avg[y] = (float)(sum / (double)EW); }
}

__global__ __launch_bounds__(64) void k_env_marginal(EnvSamplingArgs A) {
    __shared__ float w[EH];
    __shared__ double prob[EH];
    __shared__ int alias[EH], over[EH], under[EH];
    const int lane = (int)threadIdx.x;
    for (int i = lane; i < EH; i += 64) w[i] = A.scratch->row_avg[i];
    __syncthreads();
    double total, sum;
    alias_table<EH>(w, prob, alias, over, under, A.alias_prob, A.alias_idx, total, sum);
    if (lane == 0) A.scratch->marginal_total[0] = total;
}

__global__ __launch_bounds__(ZDR_ENVS_BLOCK) void k_env_pdf(EnvSamplingArgs A) {
    const int idx = (int)blockIdx.x * ZDR_ENVS_BLOCK + (int)threadIdx.x, y = idx / EW;
    const EnvSamplingScratch *S = A.scratch;
    const double rt = S->row_total[y], mt = S->marginal_total[0];
    const double c = rt > 0.0 ? fabs((double)S->scale[idx]) / rt : 1.0 / (double)EW;        // p(x|y)
    const double m = mt > 0.0 ? fabs((double)S->row_avg[y]) / mt : 1.0 / (double)EH;        // p(y)
    A.pdf[idx] = (float)(c * (m * (double)(EW * EH)));
}

int zdr_launch_envmap_sampling(const EnvSamplingArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_env_weight, dim3(ZDR_ENVS_PARTIALS), dim3(ZDR_ENVS_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_env_rows, dim3(EH), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_env_pdf, dim3(ZDR_ENVS_PARTIALS), dim3(ZDR_ENVS_BLOCK), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
