// gat_wide_lanes.h -- the lane view, pair deal and head-dot scheme of the wide-row GAT kernels
// (rows of 257 .. 1024 floats), shared by gat_wide.hip and gat_exact_wide.hip.
//
// One wave walks one row.  Lane l owns CH = ceil(F / 256) float4 slices, slice ch holding
// floats 256 ch + 4 l .. + 3; D = F / heads is a multiple of 4, so a slice lies in one head,
// whose index the lane keeps per slice.  The U * H (edge, head) pairs of a batch of U edges
// are dealt over the 64 lanes (pair i = lane + 64 t: edge i / H, head i % H).
//
// The LDS of a wave is private to it: DS operations of one wave execute in issue order, so
// a tile written by some lanes is read by others after a compiler-level fence (lds_sync); no
// workgroup barrier (the four waves of a block walk rows of different lengths).
#pragma once

#include "gat_common.h"

namespace gala {

typedef GVec<4>::T V4;

__host__ __device__ constexpr int wide_u(int CH) { return CH == 2 ? 8 : 4; }  // x[U][CH]: 64 VGPRs

// Per-wave LDS (floats): tile[2][U*H] (the terms, double-buffered for the deferred store),
// aux[U*H] (FIXED: exp terms; statistics: m * p), hv[64] (per head: q or the rescale factor
// at h, the running max at 32 + h), red[U][GW] (per-head dot partials).
// Dot products per head: a butterfly inside aligned groups of g0 = 2^lg0 lanes (the largest
// power of two dividing D / 4, at most 64), then the head's NG = D / 4 / g0 group sums added
// in order from red (GW = CH * 64 / g0 groups per vector).
struct WideCfg {
    int32_t per_wave, lg0, GW, NG;
};

__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The lane's slices of a row.
template <int CH>
struct WideLane {
    int64_t off[CH];
    int hd[CH];
    bool valid[CH];
    __device__ __forceinline__ WideLane(int lane, int F, int D) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const int f = 256 * ch + 4 * lane;
            valid[ch] = f < F;
            off[ch] = valid[ch] ? f : 0;  // lanes past F read a valid column, never store
            hd[ch] = (int)(off[ch] / D);
        }
    }
    __device__ __forceinline__ V4 load(const float *rowp, int ch, bool nt) const {
        const V4 *xp = reinterpret_cast<const V4 *>(rowp + off[ch]);
        const V4 v = nt ? __builtin_nontemporal_load(xp) : *xp;
        return valid[ch] ? v : V4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __device__ __forceinline__ void store(float *rowp, int ch, const float (&a)[4]) const {
        if (valid[ch]) *reinterpret_cast<V4 *>(rowp + off[ch]) = V4{a[0], a[1], a[2], a[3]};
    }
};

// The (edge, head) pairs of a batch this lane evaluates: slot t is pair lane + 64 t.
template <int U>
struct WidePairs {
    static constexpr int NT = U / 2;  // U * 32 heads / 64 lanes
    int k[NT], h[NT];
    bool v[NT];
    __device__ __forceinline__ WidePairs(int lane, int H) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int i = lane + 64 * t;
            v[t] = i < U * H;
            k[t] = v[t] ? i / H : 0;
            h[t] = v[t] ? i % H : 0;
        }
    }
};

__device__ __forceinline__ float seg_sum(float v, int lg0) {
    switch (lg0) {
        case 0: return v;
        case 1: return group_sum<2>(v);
        case 2: return group_sum<4>(v);
        case 3: return group_sum<8>(v);
        case 4: return group_sum<16>(v);
        case 5: return group_sum<32>(v);
        default: return group_sum<64>(v);
    }
}

// <a, b> of the lane's slice ch, fma chain from 0
__device__ __forceinline__ float dot4(const float (&a)[4], const V4 &b) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s = fmaf(a[i], b[i], s);
    return s;
}

// group sums of the N vectors' slice partials -> red[n][group]
template <int CH, int N>
__device__ __forceinline__ void head_dots_put(const float (&part)[N][CH], float *red, const WideCfg &w, int lane) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const float s = seg_sum(part[n][ch], w.lg0);
            if ((lane & ((1 << w.lg0) - 1)) == 0) red[n * w.GW + ((ch * 64 + lane) >> w.lg0)] = s;
        }
}

// head h's dot of vector n: its NG group sums in order
__device__ __forceinline__ float head_dots_get(const float *red, const WideCfg &w, int n, int h) {
    const float *r = red + n * w.GW + h * w.NG;
    float s = r[0];
    for (int g = 1; g < w.NG; ++g) s = __fadd_rn(s, r[g]);
    return s;
}

inline WideCfg wide_cfg(int F, int H, int CH) {
    const int U = wide_u(CH), D4 = F / H / 4;
    WideCfg w{};
    while (w.lg0 < 6 && D4 % (2 << w.lg0) == 0) ++w.lg0;
    w.GW = (CH * 64) >> w.lg0;
    w.NG = D4 >> w.lg0;
    w.per_wave = 3 * U * H + 64 + U * w.GW;
    return w;
}

// One wave per row, the wave's LDS after the kernel's own operand blocks.
template <typename K, typename... Ops>
int launch_wide(K kernel, const EdgeParams &p, int F, int CH, hipStream_t hs, const Ops &...ops) {
    const WideCfg w = wide_cfg(F, p.heads, CH);
    const size_t lds = (size_t)(kBlock / kWave) * w.per_wave * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3(blocks_for(p.n_rows, 64)), dim3(kBlock), lds, hs, p, ops..., w);
    return launch_status();
}

}  // namespace gala
