// gat_headw.hip -- the fused GAT forward (REF, FIXED; source logits recomputed), the REF
// row-statistics forward and the REF row-statistics backward for narrow rows (F <= 256) whose
// heads are D = 12, 20, 24, 28, 40 ... floats wide: D / 4 float4 vectors, no power of two, which
// the butterfly ladder of gat.hip / gat_fused.hip (HW = D / 4 lanes per head, heads * HW == G)
// cannot split.
//
// The row-group split of the narrow kernels is kept: a row group is G lanes, G the power of
// two >= F / 4, and a wave walks 64 / G rows at once.  Lane l of a group owns float4 l of the
// row and belongs to head l / (D / 4); lanes >= F / 4 own nothing (F = 120: 30 of 32 lanes)
// but still take their share of the per-edge scalar work.  That work -- the U * H (edge, head)
// pairs of a batch of U edges -- is dealt over the group's G lanes (pair i = l + G t: edge
// i / H, head i % H, so consecutive lanes read consecutive floats of aR[col] and store
// consecutive floats of alpha / p), each pair evaluated once, in as many rounds t as U * H
// takes (21 heads of 12 floats: 168 pairs over 64 lanes).  The terms go to a per-group LDS tile
// [U][H], from which every lane reads its head's term per edge and from which lane h < H
// adds head h's running sums in CSR order.  The accumulation is fmaf(p, x, acc) per edge in
// CSR order, as everywhere.
//
// Per-head dot products (the recomputed source logit, the backward's <dY, Y> and <dY, Ym>): a
// float4 fma chain per lane, a butterfly inside aligned groups of g0 lanes (the largest power
// of two dividing D / 4: the head starts at a multiple of it), and the head's D / 4 / g0 group
// sums added in lane order from the group's LDS by the lane that evaluates the pair.
//
// A group's LDS is private to its wave: DS operations of one wave execute in issue order, so
// a tile written by some lanes is read by others after a compiler-level fence (lds_sync); no
// workgroup barrier (the rows of a wave and of a block differ in length; the lanes of one
// group share their trip counts, and no cross-lane operation leaves the group).
#include "gat_headw.h"
#include "gat_wide_lanes.h"  // V4, lds_sync, seg_sum, dot4

namespace gala {

constexpr int kHeadwU = 8;                 // edges per batch: x[U] is 32 VGPRs
constexpr int kHeadwNT = (kHeadwU + 2) / 3;  // pair rounds: H * 3 <= G, so U * H <= G * U / 3

// Per-group LDS (floats): tile[2][U*H] (the terms, double-buffered for the deferred store),
// aux[U*H] (FIXED: exp terms; statistics: m * p), hv[2*H] (per head: q or the rescale factor
// at h, the running max at H + h), red[U][GW] (dot partials, GW = G / g0 lane groups per
// vector; the head's NG = D / 4 / g0 sums are adjacent).
struct HeadwCfg {
    int32_t per_group, lg0, GW, NG, D4;
};

// The lane's float4 of a row.
struct HeadwLane {
    int64_t off;
    int hd;
    bool valid;
    __device__ __forceinline__ HeadwLane(int gl, int F, int D4) {
        valid = 4 * gl < F;
        off = valid ? 4 * gl : 0;  // lanes past F read a valid column, never store
        hd = valid ? gl / D4 : 0;
    }
    __device__ __forceinline__ V4 load(const float *rowp, bool nt) const {
        const V4 *xp = reinterpret_cast<const V4 *>(rowp + off);
        const V4 v = nt ? __builtin_nontemporal_load(xp) : *xp;
        return valid ? v : V4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __device__ __forceinline__ void store(float *rowp, const float (&a)[4]) const {
        if (valid) *reinterpret_cast<V4 *>(rowp + off) = V4{a[0], a[1], a[2], a[3]};
    }
};

// The (edge, head) pairs of a batch this lane evaluates: round t is pair gl + G t.
template <int G>
struct HeadwPairs {
    int k[kHeadwNT], h[kHeadwNT];
    bool v[kHeadwNT];
    __device__ __forceinline__ HeadwPairs(int gl, int H) {
#pragma unroll
        for (int t = 0; t < kHeadwNT; ++t) {
            const int i = gl + G * t;
            v[t] = i < kHeadwU * H;
            k[t] = v[t] ? i / H : 0;
            h[t] = v[t] ? i % H : 0;
        }
    }
};

// group sums of the N vectors' lane partials -> red[n][lane group]
template <int N>
__device__ __forceinline__ void headw_dots_put(const float (&part)[N], float *red, const HeadwCfg &w, int gl) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float s = seg_sum(part[n], w.lg0);
        if ((gl & ((1 << w.lg0) - 1)) == 0) red[n * w.GW + (gl >> w.lg0)] = s;
    }
}

// head h's dot of vector n: its NG group sums in lane order
__device__ __forceinline__ float headw_dots_get(const float *red, const HeadwCfg &w, int n, int h) {
    const float *r = red + n * w.GW + h * w.NG;
    float s = r[0];
    for (int g = 1; g < w.NG; ++g) s = __fadd_rn(s, r[g]);
    return s;
}

template <int G>
__device__ __forceinline__ float *headw_lds(float *base, const HeadwCfg &w) {
    return base + (threadIdx.x / G) * w.per_group;  // threadIdx.x / G: the block's row group
}

// ---- forward ---------------------------------------------------------------------------
template <int G, int MODE, bool RC>
__global__ __launch_bounds__(kBlock) void k_gat_headw_fwd(EdgeParams p, GatDev d, HeadwCfg w) {
    constexpr int U = kHeadwU, NT = kHeadwNT;
    constexpr bool kRef = ref_mode(MODE), kStats = MODE == kRefStats;
    GALA_ROW_PROLOGUE(G);
    if (!row_ok) return;
    extern __shared__ float headw_lds_[];
    float *ws = headw_lds<G>(headw_lds_, w);
    const int H = p.heads, UH = U * H;
    float *tile = ws, *aux = ws + 2 * UH, *hv = ws + 3 * UH, *red = hv + 2 * H;
    const HeadwLane ln(gl, d.F, w.D4);
    const HeadwPairs<G> pr(gl, H);
    float pal[NT], pb[NT], wr[4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        pal[t] = d.aL[row * H + pr.h[t]];
        pb[t] = (RC && d.bR) ? d.bR[pr.h[t]] : 0.0f;
    }
    if constexpr (RC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wr[i] = ln.valid ? d.wR[ln.off + i] : 0.0f;
    }
    if constexpr (RC && kStats) {
        // the row's own source logit for the backward's alpha: X[row] through the very
        // reduction its edges take (same fma order, butterfly and group order)
        if (d.ar_out) {
            float part[1];
            part[0] = dot4(wr, ln.load(d.X + row * d.ldx, false));
            headw_dots_put<1>(part, red, w, gl);
            lds_sync();
            if (gl < H) d.ar_out[row * H + gl] = __fadd_rn(headw_dots_get(red, w, 0, gl), d.bR ? d.bR[gl] : 0.0f);
            lds_sync();
        }
    }
    float acc[4], accm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = accm[i] = 0.0f;
    float m = -INFINITY, sum = 0.0f, sma = 0.0f;  // lane h < H of the group: head h's running state
    int64_t e0, e1;
    row_range(p, 0, row, e0, e1);
    const int32_t n = (int32_t)(e1 - e0);
    const bool park = d.alpha_out != nullptr;
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V4 x[U];
        load_batch_cols<G, U>(p, e0, n, j0, c);
        float ar[NT];
        if constexpr (!RC) {
            // the pair's source logit: its edge's column read by the evaluating lane itself
            // (issued beside the batch's column loads: no second round trip)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                ar[t] = 0.0f;
                if (G * t < UH) {
                    const int32_t j = (j0 + pr.k[t] < n) ? j0 + pr.k[t] : n - 1;
                    ar[t] = d.aR[(int64_t)p.col[e0 + j] * H + pr.h[t]];
                }
            }
        }
        // given source logits: the rows are loaded nontemporal (gat.hip, gat_fwd_range_dist)
#pragma unroll
        for (int k = 0; k < U; ++k) x[k] = ln.load(d.X + c[k] * d.ldx, !RC);
        // The parked terms of a batch are stored one batch late, after this batch's loads are
        // issued (stores count in vmcnt: gat_fwd_range_dist); a previous batch is always full.
        if (park && j0 > 0) {
            const float *tp = tile + (((j0 / U) - 1) & 1) * UH;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (pr.v[t]) d.alpha_out[(e0 + j0 - U) * H + gl + G * t] = tp[gl + G * t];
        }
        if constexpr (RC) {
            float part[U];
#pragma unroll
            for (int k = 0; k < U; ++k) part[k] = dot4(wr, x[k]);
            headw_dots_put<U>(part, red, w, gl);
            lds_sync();
#pragma unroll
            for (int t = 0; t < NT; ++t)
                ar[t] = (G * t < UH) ? __fadd_rn(headw_dots_get(red, w, pr.k[t], pr.h[t]), pb[t]) : 0.0f;
            lds_sync();
        }
        float *cur = tile + ((j0 / U) & 1) * UH;
        float z[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float s = __fadd_rn(pal[t], ar[t]);
            const bool pos = s > 0.0f;
            z[t] = pos ? s : __fmul_rn(s, d.slope);
            if (!pr.v[t]) continue;
            if constexpr (kRef) {
                const float pe = ref_exp(z[t]);
                cur[gl + G * t] = pe;
                if constexpr (kStats) aux[gl + G * t] = pos ? pe : __fmul_rn(pe, d.slope);
            } else {
                cur[gl + G * t] = z[t];
            }
        }
        lds_sync();
        const int nb = (n - j0 < U) ? n - j0 : U;
        if constexpr (!kRef) {
            // the batch maximum per head from the tile; the running state rescaled once.  As in
            // the narrow kernels (gat.hip, FIXED), a head whose logits so far are all -inf keeps
            // m = -inf and its terms are exp(-inf - -inf) = NaN: finite logits are assumed.
            if (gl < H) {
                float mb = -INFINITY, r = 1.0f;
                for (int k = 0; k < nb; ++k) mb = fmaxf(mb, cur[k * H + gl]);
                if (mb > m) {
                    r = (m == -INFINITY) ? 0.0f : expf(m - mb);
                    sum = __fmul_rn(sum, r);
                    m = mb;
                }
                hv[gl] = r;
                hv[H + gl] = m;
            }
            lds_sync();
            const float r = hv[ln.hd];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __fmul_rn(acc[i], r);
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (pr.v[t]) aux[gl + G * t] = expf(z[t] - hv[H + pr.h[t]]);
            lds_sync();
        }
        const float *pt = kRef ? cur : aux;
        if (gl < H) {
            for (int k = 0; k < nb; ++k) {
                sum = __fadd_rn(sum, pt[k * H + gl]);
                if constexpr (kStats) sma = __fadd_rn(sma, aux[k * H + gl]);
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
                const float pk = pt[k * H + ln.hd];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(pk, x[k][i], acc[i]);
                if constexpr (kStats) {
                    const float mk = aux[k * H + ln.hd];
#pragma unroll
                    for (int i = 0; i < 4; ++i) accm[i] = fmaf(mk, x[k][i], accm[i]);
                }
            }
        }
        lds_sync();  // aux / hv / red are rewritten by the next batch
    }
    if (park && n > 0) {  // the last batch's terms
        const int32_t jl = (n - 1) / U * U;
        const float *tp = tile + ((jl / U) & 1) * UH;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (pr.v[t] && jl + pr.k[t] < n) d.alpha_out[(e0 + jl) * H + gl + G * t] = tp[gl + G * t];
    }
    // Y = acc * q with q = 1 / (sum [+ S * 1e-12 in REF mode]), as gat_fwd_store
    if (gl < H) {
        const float den = kRef ? sum + (float)p.seg.n * 1e-12f : sum;
        const float q = (!kRef && sum == 0.0f) ? 0.0f : 1.0f / den;
        hv[gl] = q;
        hv[H + gl] = m;
        if (d.q_out) d.q_out[row * H + gl] = q;
        if constexpr (kStats) d.sma_out[row * H + gl] = __fmul_rn(sma, q);
    }
    lds_sync();
    {
        const float q = hv[ln.hd];
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(acc[i], q);
        ln.store(d.Y + row * d.ldy, o);
        if constexpr (kStats) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(accm[i], q);
            ln.store(d.ym_out + row * d.ldym, o);
        }
    }
    if (!d.alpha_out || d.q_out) return;  // factored: the parked exp terms are the output
    // alpha from the parked terms (REF) / logits (FIXED), stored by other lanes of this group
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    float *ap = d.alpha_out + e0 * H;
    for (int32_t t = gl; t < n * H; t += G) {
        const int h = t % H;
        const float pe = kRef ? ap[t] : expf(ap[t] - hv[H + h]);
        ap[t] = __fmul_rn(pe, hv[h]);
    }
}

// ---- row-statistics backward -------------------------------------------------------------
// dX = A_alpha dY with alpha = fl(p * q) rebuilt per (edge, head) pair from aR (or the
// forward's p), gathering dY[col] only; d_aL from the row's Y, Ym, sma and dY[row].
// FP: alpha = fl(p * q) from the forward's p (d.alpha) instead of the logits.  d.attn_w (the
// source logit's per-head Linear): dX also takes fl(d_aL * attn_w) at the store.
template <int G, bool FP>
__global__ __launch_bounds__(kBlock) void k_gat_headw_bwd_stats(EdgeParams p, GatDev d, HeadwCfg w) {
    constexpr int U = kHeadwU, NT = kHeadwNT;
    GALA_ROW_PROLOGUE(G);
    if (!row_ok) return;
    extern __shared__ float headw_lds_[];
    float *ws = headw_lds<G>(headw_lds_, w);
    const int H = p.heads, UH = U * H;
    float *tile = ws, *hv = ws + 3 * UH, *red = hv + 2 * H;
    const HeadwLane ln(gl, d.F, w.D4);
    const HeadwPairs<G> pr(gl, H);
    {   // d_aL = (<dY, Ym> - (<dY, Y> + eps) sma) + eps per head (stats_d_al, gat_fused.hip)
        float part[2];
        const V4 dy = ln.load(d.dY + row * d.lddy, false);
        const float dyv[4] = {dy[0], dy[1], dy[2], dy[3]};
        part[0] = dot4(dyv, ln.load(d.ys + row * d.ldy, false));
        part[1] = dot4(dyv, ln.load(d.yms + row * d.ldym, false));
        headw_dots_put<2>(part, red, w, gl);
        lds_sync();
        if (gl < H) {
            const float eps = (float)p.seg.n * 1e-12f;
            const float acc = headw_dots_get(red, w, 0, gl) + eps;
            const float s1 = headw_dots_get(red, w, 1, gl);
            const float dal = (s1 - acc * d.smas[row * H + gl]) + eps;
            d.d_aL[row * H + gl] = dal;
            hv[gl] = dal;  // kept for the Linear's term at the store
        }
        lds_sync();
    }
    float pal[NT], pq[NT], dxa[4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        pal[t] = d.aL[row * H + pr.h[t]];
        pq[t] = d.q[row * H + pr.h[t]];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dxa[i] = 0.0f;
    int64_t e0, e1;
    row_range(p, 0, row, e0, e1);
    const int32_t n = (int32_t)(e1 - e0);
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V4 yv[U];
        load_batch_cols<G, U>(p, e0, n, j0, c);
        float sv[NT];  // the pair's source logit, or (FP) its exp term p
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sv[t] = 0.0f;
            if (G * t < UH) {
                const int32_t j = (j0 + pr.k[t] < n) ? j0 + pr.k[t] : n - 1;
                if constexpr (FP) sv[t] = d.alpha[(e0 + j) * H + pr.h[t]];
                else sv[t] = d.aR[(int64_t)p.col[e0 + j] * H + pr.h[t]];
            }
        }
        // nontemporal: the gathered dY rows would evict the aR table (gat_fused.hip)
#pragma unroll
        for (int k = 0; k < U; ++k) yv[k] = ln.load(d.dY + c[k] * d.lddy, true);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float pe = sv[t];
            if constexpr (!FP) {
                const float s = __fadd_rn(pal[t], sv[t]);
                pe = ref_exp(s > 0.0f ? s : __fmul_rn(s, d.slope));
            }
            if (pr.v[t]) tile[gl + G * t] = __fmul_rn(pe, pq[t]);
        }
        lds_sync();
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
                const float ak = tile[k * H + ln.hd];
#pragma unroll
                for (int i = 0; i < 4; ++i) dxa[i] = fmaf(ak, yv[k][i], dxa[i]);
            }
        }
        lds_sync();  // the tile is rewritten by the next batch
    }
    if (d.attn_w && ln.valid) {
        const float dal = hv[ln.hd];
#pragma unroll
        for (int i = 0; i < 4; ++i) dxa[i] = __fadd_rn(dxa[i], __fmul_rn(dal, d.attn_w[ln.off + i]));
    }
    ln.store(d.dX + row * d.lddx, dxa);
}

// ---- host side ---------------------------------------------------------------------------
static HeadwCfg headw_cfg(int F, int H, int G) {
    HeadwCfg w{};
    w.D4 = F / H / 4;
    while (w.D4 % (2 << w.lg0) == 0) ++w.lg0;
    w.GW = G >> w.lg0;
    w.NG = w.D4 >> w.lg0;
    w.per_group = 3 * kHeadwU * H + 2 * H + kHeadwU * w.GW;
    return w;
}

static int headw_group(int F) {
    int G = 8;
    while (4 * G < F) G <<= 1;
    return G;
}

// 64 / G rows per wave, each group's LDS after the previous one's.
template <typename K>
static int launch_headw(K kernel, const EdgeParams &p, const GatDev &d, int G, hipStream_t hs) {
    const HeadwCfg w = headw_cfg(d.F, p.heads, G);
    const size_t lds = (size_t)(kBlock / G) * w.per_group * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3(blocks_for(p.n_rows, G)), dim3(kBlock), lds, hs, p, d, w);
    return launch_status();
}

bool gat_headw_shape(const gala_csr_t *A, int32_t F, int32_t heads, int vec) {
    if (heads < 2 || F > 256 || F % heads != 0 || (F / heads) % 4 != 0 || vec != 4) return false;
    const int D4 = F / heads / 4;
    // square: the kernels read X[row], dY[row], Y[row] and Ym[row] of every row, so the column
    // operands must hold exactly the rows
    return (D4 & (D4 - 1)) != 0 && A->n_seg == 1 && A->n_cols == A->n_rows &&
           (!A->split || A->split->n_rows_split == 0);
}

template <int G>
static int headw_fwd_g(const EdgeParams &p, const GatDev &d, int mode, hipStream_t hs) {
    if (mode == kRefStats)
        return d.aR ? launch_headw(k_gat_headw_fwd<G, kRefStats, false>, p, d, G, hs)
                    : launch_headw(k_gat_headw_fwd<G, kRefStats, true>, p, d, G, hs);
    // outside the statistics the caller passes recomputed logits only (gat_headw.h)
    if (mode == GALA_SOFTMAX_REF) return launch_headw(k_gat_headw_fwd<G, GALA_SOFTMAX_REF, true>, p, d, G, hs);
    return launch_headw(k_gat_headw_fwd<G, GALA_SOFTMAX_FIXED, true>, p, d, G, hs);
}

int gat_headw_fwd(const EdgeParams &p, const GatDev &d, int mode, hipStream_t hs) {
    switch (headw_group(d.F)) {
        case 8: return headw_fwd_g<8>(p, d, mode, hs);
        case 16: return headw_fwd_g<16>(p, d, mode, hs);
        case 32: return headw_fwd_g<32>(p, d, mode, hs);
        default: return headw_fwd_g<64>(p, d, mode, hs);
    }
}

template <int G>
static int headw_bwd_g(const EdgeParams &p, const GatDev &d, hipStream_t hs) {
    return d.alpha ? launch_headw(k_gat_headw_bwd_stats<G, true>, p, d, G, hs)
                   : launch_headw(k_gat_headw_bwd_stats<G, false>, p, d, G, hs);
}

int gat_headw_bwd_stats(const EdgeParams &p, const GatDev &d, hipStream_t hs) {
    switch (headw_group(d.F)) {
        case 8: return headw_bwd_g<8>(p, d, hs);
        case 16: return headw_bwd_g<16>(p, d, hs);
        case 32: return headw_bwd_g<32>(p, d, hs);
        default: return headw_bwd_g<64>(p, d, hs);
    }
}

}  // namespace gala
