// SpMM neighbour aggregation from bfloat16-stored features for gfx950 (CDNA4, wave64):
// GALA_SPMM_X_BF16 / GALA_SPMM_Y2_BF16 of gala_spmm_ex_f32.
//
// The gather is the SpMM's bound, and a bf16 row is half the bytes of an fp32 row.  Every
// gathered element is widened exactly (bits << 16) and from there the arithmetic is the fp32
// kernels' (csrc/spmm.hip): w_e * (src_scale[c] * x) with the product rounded and the add
// contracted to an fma, one sequential chain per feature in CSR order, the dst factor and
// the Y2 = s2 * Y epilogue last.  Each feature is its own chain, so the result does not depend
// on which lane owns it and equals the fp32 path on the widened input bit for bit.
//
// Row kernel (k_spmm_bf16_rows): a row group of G lanes owns one CSR row; lane g owns XV
// contiguous features at column (ch*G + g)*XV for ch < CH and loads them with ONE load of
// XV*2 bytes (XV = 8: 16 B).  For the same row that is half the fp32 kernel's lanes (F = 32:
// 4 lanes, 16 rows a wave; F = 128: 16 lanes, 4 rows a wave), so a wave has twice the rows
// and twice the independent gathers in flight; the gathered rows stay packed in registers (4
// VGPRs per 8 features) until their turn in the add chain, so U edges in flight cost half the
// fp32 kernel's registers.  XV falls to 4 / 2 / 1 (8 / 4 / 2-byte loads) with the strides and
// base addresses.  The same template with XT = float serves fp32 X with a bf16 Y2.
//
// Hub kernel (k_spmm_bf16_hub): the REF-order hub rows of a split plan, k_spmm_hub_exact's
// gatherer / chain split with the neighbour rows staged in LDS AS bf16 -- twice the edges per
// tile -- and widened at the chain's LDS read.
#include <stddef.h>

#include "bf16.h"
#include "spmm_bf16.h"

namespace gala {

typedef uint16_t bf16_t;
typedef uint32_t U2 __attribute__((ext_vector_type(2)));
typedef uint32_t U4 __attribute__((ext_vector_type(4)));
typedef float F2 __attribute__((ext_vector_type(2)));
typedef float F4 __attribute__((ext_vector_type(4)));

// the XV elements one lane gathers from one X row, as loaded (bf16 stays packed)
template <class XT, int XV>
struct Raw {
    static constexpr int B = XV * (int)sizeof(XT);  // bytes per load
    static constexpr int NW = B >= 4 ? B / 4 : 1;
    uint32_t r[NW];
    __device__ __forceinline__ void load(const XT *p) {
        if constexpr (B == 2) {
            r[0] = *reinterpret_cast<const uint16_t *>(p);
        } else if constexpr (B == 4) {
            r[0] = *reinterpret_cast<const uint32_t *>(p);
        } else if constexpr (B == 8) {
            const U2 v = *reinterpret_cast<const U2 *>(p);
            r[0] = v.x, r[1] = v.y;
        } else {
            const U4 v = *reinterpret_cast<const U4 *>(p);
            r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
        }
    }
    // element i as stored, in the low 16 bits (bf16 only)
    __device__ __forceinline__ uint32_t half(int i) const {
        return XV == 1 ? r[0] : (i & 1) ? r[i / 2] >> 16 : r[i / 2] & 0xffffu;
    }
    // element i widened to fp32 (exact)
    __device__ __forceinline__ float get(int i) const {
        if constexpr (sizeof(XT) == 4) return __uint_as_float(r[i]);
        else if constexpr (XV == 1) return __uint_as_float(r[0] << 16);
        else return __uint_as_float((i & 1) ? (r[i / 2] & 0xffff0000u) : (r[i / 2] << 16));
    }
};

// GCN norm deg^-0.5 of a row count: k_degree_count's expression (csrc/spmm.hip)
__device__ __forceinline__ float deg_rsqrt_b(float d) { return 1.0f / sqrtf(d); }

__device__ __forceinline__ float dst_factor_b(const Bf16Params &p, int64_t row, bool &has) {
    has = p.dst_deg || p.dst_scale;
    if (p.dst_deg) return deg_rsqrt_b((float)(p.rowptr[row + 1] - p.rowptr[row]));
    return p.dst_scale ? p.dst_scale[row] : 1.0f;
}

// N fp32 to / from a row of Y in vectors of min(N, 4) floats; nv < N (a padded row's last
// vector) goes element by element and never touches the padding
template <int N>
__device__ __forceinline__ void ld_f(const float *p, float (&v)[N], int nv) {
    if (nv == N) {
        if constexpr (N >= 4) {
#pragma unroll
            for (int i = 0; i < N; i += 4) {
                const F4 t = *reinterpret_cast<const F4 *>(p + i);
                v[i] = t.x, v[i + 1] = t.y, v[i + 2] = t.z, v[i + 3] = t.w;
            }
        } else if constexpr (N == 2) {
            const F2 t = *reinterpret_cast<const F2 *>(p);
            v[0] = t.x, v[1] = t.y;
        } else {
            v[0] = p[0];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = i < nv ? p[i] : 0.0f;
}
template <int N>
__device__ __forceinline__ void st_f(float *p, const float (&v)[N], int nv) {
    if (nv == N) {
        if constexpr (N >= 4) {
#pragma unroll
            for (int i = 0; i < N; i += 4) {
                F4 t;
                t.x = v[i], t.y = v[i + 1], t.z = v[i + 2], t.w = v[i + 3];
                *reinterpret_cast<F4 *>(p + i) = t;
            }
        } else if constexpr (N == 2) {
            F2 t;
            t.x = v[0], t.y = v[1];
            *reinterpret_cast<F2 *>(p) = t;
        } else {
            p[0] = v[0];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i < nv) p[i] = v[i];
}
// N fp32 rounded to bf16 (nearest even) and stored as one vector of 2*N bytes
template <int N>
__device__ __forceinline__ void st_h(bf16_t *p, const float (&v)[N], int nv) {
    if (nv == N) {
        if constexpr (N == 1) {
            p[0] = bf16_rne(v[0]);
        } else {
            uint32_t w[N / 2];
#pragma unroll
            for (int i = 0; i < N / 2; ++i) w[i] = (uint32_t)bf16_rne(v[2 * i]) | (uint32_t)bf16_rne(v[2 * i + 1]) << 16;
            if constexpr (N == 2) {
                *reinterpret_cast<uint32_t *>(p) = w[0];
            } else if constexpr (N == 4) {
                U2 t;
                t.x = w[0], t.y = w[1];
                *reinterpret_cast<U2 *>(p) = t;
            } else {
                U4 t;
                t.x = w[0], t.y = w[1], t.z = w[2], t.w = w[3];
                *reinterpret_cast<U4 *>(p) = t;
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i < nv) p[i] = bf16_rne(v[i]);
}

// acc (+)= w * (s * x): the fp32 kernels' accumulate<> on one element
template <bool W, bool SRCS>
__device__ __forceinline__ void add_edge(float &acc, float x, float w, float s) {
    const float v = SRCS ? __fmul_rn(s, x) : x;
    if (W) acc = fmaf(w, v, acc);
    else acc = __fadd_rn(acc, v);
}

// ---- rows ------------------------------------------------------------------------------
template <class XT, int XV, int G, int CH, int U, bool W, bool SRCS>
__global__ __launch_bounds__(kBlock) void k_spmm_bf16_rows(Bf16Params p) {
    constexpr int RPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int gl = lane & (G - 1);
    const int64_t nb = gridDim.x;
    const int64_t blk = p.xcd_order ? logical_block_runs(blockIdx.x, nb, kXcdRun) : (int64_t)blockIdx.x;
    const int64_t rid = (blk * (kBlock / kWave) + threadIdx.x / kWave) * RPW + lane / G;
    if (rid >= p.n_rows) return;
    const int64_t row = p.row_order ? (int64_t)p.row_order[rid] : rid;
    const int64_t e0 = p.rowptr[row];
    const int32_t n = p.rowptr[row + 1] - (int32_t)e0;
    if (p.split_threshold > 0 && n > p.split_threshold) return;  // hub row: k_spmm_bf16_hub

    // per-lane columns: lanes past F gather column 0 (a valid address) and never store
    bool valid[CH];
    int off[CH], head[CH], nv[CH];
    float rs[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const int f = (ch * G + gl) * XV;
        valid[ch] = f < p.F;
        off[ch] = valid[ch] ? f : 0;
        head[ch] = W ? (p.f_base + off[ch]) / p.head_dim : 0;
        nv[ch] = valid[ch] ? (p.F - f < XV ? p.F - f : XV) : 0;
        rs[ch] = (W && p.val_rs) ? p.val_rs[row * p.val_heads + head[ch]] : 1.0f;
    }
    const XT *X = static_cast<const XT *>(p.X);
    float acc[CH][XV];
    const bool start_from_y = p.accum && p.dst_scale == nullptr && !p.dst_deg;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        if (start_from_y && valid[ch]) {
            ld_f<XV>(p.Y + row * p.ldy + off[ch], acc[ch], nv[ch]);
        } else {
#pragma unroll
            for (int i = 0; i < XV; ++i) acc[ch][i] = 0.0f;
        }
    }

    // edges in CSR order; the packed rows of U edges are loaded before the first add
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int32_t c[U];
        Raw<XT, XV> x[U][CH];
        float w[U][CH], sc[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t e = e0 + ((j0 + k < n) ? j0 + k : n - 1);  // clamped: a valid address
            c[k] = p.col[e];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) w[k][ch] = W ? p.val[e * p.val_heads + head[ch]] : 1.0f;
        }
        if (W && p.val_rs) {
#pragma unroll
            for (int k = 0; k < U; ++k)
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) w[k][ch] = __fmul_rn(w[k][ch], rs[ch]);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const XT *xr = X + (int64_t)c[k] * p.ldx;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) x[k][ch].load(xr + off[ch]);
            sc[k] = SRCS ? p.src_scale[c[k]] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch)
#pragma unroll
                    for (int i = 0; i < XV; ++i) add_edge<W, SRCS>(acc[ch][i], x[k][ch].get(i), w[k][ch], sc[k]);
            }
        }
    }

    bool has_ds;
    const float ds = dst_factor_b(p, row, has_ds);
    const float s2 = p.y2_scale ? p.y2_scale[row] : ds;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        if (!valid[ch]) continue;
        float *yp = p.Y + row * p.ldy + off[ch];
        float(&out)[XV] = acc[ch];
        if (has_ds) {
#pragma unroll
            for (int i = 0; i < XV; ++i) out[i] = __fmul_rn(ds, out[i]);
            if (p.accum) {
                float y[XV];
                ld_f<XV>(yp, y, nv[ch]);
#pragma unroll
                for (int i = 0; i < XV; ++i) out[i] = __fadd_rn(y[i], out[i]);
            }
        }
        st_f<XV>(yp, out, nv[ch]);
        if (p.Y2) {  // the next aggregation's pre-scaled input: fl(s2 * Y), then to bf16 when asked
#pragma unroll
            for (int i = 0; i < XV; ++i) out[i] = __fmul_rn(s2, out[i]);
            if (p.y2_bf16) st_h<XV>(static_cast<bf16_t *>(p.Y2) + row * p.ldy2 + off[ch], out, nv[ch]);
            else st_f<XV>(static_cast<float *>(p.Y2) + row * p.ldy2 + off[ch], out, nv[ch]);
        }
    }
}

// ---- hub rows in the reference's order, staged as bf16 ----------------------------------
// One workgroup owns (hub row, slice of FSP features).  Waves 1-7 gather the X rows of tile
// t+1 into one of two LDS buffers while wave 0, one lane per feature, adds tile t from the
// other in CSR order (k_spmm_hub_exact's pipeline, one barrier per tile).
//
// LDS layout, in dwords.  The chain lane of a feature reads 16 B = an OCTET of 8 consecutive
// edges of that feature (a dword holds the edge pair 2i | 2i+1 << 16), so a buffer of the same
// 32 KB holds twice the fp32 kernel's edges.  A bank is a dword, and two lanes storing the two
// halves of one dword would serialise, so a gatherer owns an edge PAIR: it loads the same XV
// columns of both edges' rows and stores XV whole dwords.  Octet o of feature f is at
//   o * OCT + slot(f) * 4 + pair % 4,   slot(f) = (f % XV) * (FSP / XV) + f / XV,
// so one store instruction's lanes -- FSP / XV column vectors of consecutive pairs -- write
// 4 * FSP / XV consecutive dwords per octet.  The LDS takes a wave's 4-byte stores 32 lanes
// at a time: with FSP / XV >= 8 an octet's lanes fill all 32 banks; with FSP / XV = 4
// (F <= 32 in 16-B vectors) two octets share a half-wave, and OCT is padded by 16 dwords so
// the second octet falls on the other 16 banks.  The chain's 16-B reads cover 64 consecutive
// 16-B slots of one octet.  (The 2- and 4-byte fallbacks XV <= 2 keep the addresses, not the
// guarantee: their column vectors are 4 dwords apart.)
constexpr int kHubThreads = 512;
constexpr int kHubGather = kHubThreads - kWave;
constexpr int kHubBufDw = 8192;   // dwords of X per LDS buffer before padding (32 KB; two buffers)
constexpr int kHubHeads = 4;      // edge-weight heads per slice staged in LDS (spmm.hip: kHubMaxHeads)

template <int XV, int FSP, bool W, bool SRCS>
struct HubLdsB {
    // edges per tile: 32 KB of bf16; the 4- and 2-byte fallbacks take a half and a quarter, so
    // a gatherer keeps at most 5 (pair, vector) slots -- 10 loads -- in registers
    static constexpr int T = 2 * kHubBufDw / FSP / (XV >= 4 ? 1 : XV == 2 ? 2 : 4);
    static constexpr int LPE = FSP / XV;             // column vectors (gatherer lanes) per edge pair
    static constexpr int OCT = FSP * 4 + (4 * LPE < 32 ? 4 * LPE : 0);
    static constexpr int BUF = (T / 8) * OCT;
    static constexpr int kGroup = 16;                // edges per chain group (two octets)
    static constexpr size_t buf = 0, scl = 2 * (size_t)BUF, wts = scl + (SRCS ? 2 * T : 0),
                            yinit = wts + (W ? 2 * (size_t)kHubHeads * T : 0), slack = yinit + kWave,
                            dwords = slack + 2 * (kGroup / 8) * OCT;  // the chain prefetches two groups past a buffer
};

template <int XV, int FSP, bool W, bool SRCS>
__global__ __launch_bounds__(kHubThreads) void k_spmm_bf16_hub(Bf16Params p, Bf16Hub hp) {
    typedef HubLdsB<XV, FSP, W, SRCS> L;
    constexpr int T = L::T, LPE = L::LPE, OCT = L::OCT;
    constexpr int RG = ((T / 2) * LPE + kHubGather - 1) / kHubGather;  // (pair, vector) slots per gatherer
    constexpr int RW = (T * kHubHeads + kHubGather - 1) / kHubGather;
    extern __shared__ uint32_t hub_lds_b[];
    float *const lds_f = reinterpret_cast<float *>(hub_lds_b);
    const bf16_t *X = static_cast<const bf16_t *>(p.X);
    const int64_t ri = blockIdx.x / hp.n_slices;
    const int slice = blockIdx.x % hp.n_slices;
    const int64_t row = hp.order ? hp.order[ri] : hp.rows[ri];  // the plan's order: longest chains first
    const int f0 = slice * FSP;
    const int fs = (p.F - f0) < FSP ? (p.F - f0) : FSP;
    const int lpe = (fs + XV - 1) / XV;
    const int h0 = W ? (p.f_base + f0) / p.head_dim : 0;
    const int hs = W ? (p.f_base + f0 + fs - 1) / p.head_dim - h0 + 1 : 0;  // <= kHubHeads (host)
    const int64_t e0 = p.rowptr[row], n = (int64_t)p.rowptr[row + 1] - e0;
    const int ntiles = (int)((n + T - 1) / T);
    const bool gatherer = threadIdx.x >= kWave;
    const int g = threadIdx.x - kWave;

    // ---- gatherers: slot k = (edge pair, column vector) of a tile, fixed for every tile ----
    int s_pair[RG], s_vec[RG];
    int32_t cc[RG][2];
    Raw<bf16_t, XV> xr[RG][2];
    float sr[RG][2], wr[RW];
#pragma unroll
    for (int k = 0; k < RG; ++k) {
        const int i = k * kHubGather + g;
        s_pair[k] = (gatherer && i / lpe < T / 2) ? i / lpe : -1;
        s_vec[k] = i % lpe;
    }
    auto load_cols = [&](int t) {
#pragma unroll
        for (int k = 0; k < RG; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int64_t j = (int64_t)t * T + 2 * (s_pair[k] < 0 ? 0 : s_pair[k]) + h;
                if (j >= n) j = n - 1;  // clamped: a valid address, never used
                cc[k][h] = p.col[e0 + j];
            }
    };
    auto load_x = [&](int t) {  // unconditional, so the loads issue back to back
#pragma unroll
        for (int k = 0; k < RG; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                xr[k][h].load(X + (int64_t)cc[k][h] * p.ldx + f0 + s_vec[k] * XV);
                if (SRCS) sr[k][h] = p.src_scale[cc[k][h]];
            }
        if (W) {
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                const int i = k * kHubGather + g;
                int64_t j = (int64_t)t * T + (hs > 0 ? i / hs : 0);
                if (j >= n) j = n - 1;
                wr[k] = p.val[(e0 + j) * p.val_heads + h0 + (hs > 0 ? i % hs : 0)];
            }
        }
    };
    auto store = [&](int b) {
        uint32_t *xb = hub_lds_b + L::buf + (size_t)b * L::BUF;
#pragma unroll
        for (int k = 0; k < RG; ++k) {
            const int pr = s_pair[k];
            if (pr < 0) continue;
            uint32_t *q = xb + (pr >> 2) * OCT + s_vec[k] * 4 + (pr & 3);
#pragma unroll
            for (int v = 0; v < XV; ++v) q[4 * v * LPE] = (xr[k][0].half(v) & 0xffffu) | (xr[k][1].half(v) << 16);
            if (SRCS && s_vec[k] == 0) {
                lds_f[L::scl + b * T + 2 * pr] = sr[k][0];
                lds_f[L::scl + b * T + 2 * pr + 1] = sr[k][1];
            }
        }
        if (W) {
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                const int i = k * kHubGather + g;
                if (i < T * hs) lds_f[L::wts + (size_t)b * kHubHeads * T + (i % hs) * T + i / hs] = wr[k];
            }
        }
    };

    // ---- chain: wave 0, lane f < fs owns feature f0 + f ----
    const int lane = threadIdx.x;
    const bool chain = lane < fs;
    const int cl = chain ? lane : 0;
    const int f = f0 + cl;
    const int slot = (cl % XV) * LPE + cl / XV;
    const int hl = W ? (p.f_base + f) / p.head_dim - h0 : 0;
    const float rs = (W && p.val_rs) ? p.val_rs[row * p.val_heads + h0 + hl] : 1.0f;
    const bool from_y = p.accum && p.dst_scale == nullptr && !p.dst_deg;
    if (chain && from_y) lds_f[L::yinit + lane] = p.Y[row * p.ldy + f];
    float acc = 0.0f;
    auto add = [&](uint32_t xbits, float w, float sv) {
        add_edge<W, SRCS>(acc, __uint_as_float(xbits), (W && p.val_rs) ? __fmul_rn(w, rs) : w, sv);
    };
    constexpr int GS = L::kGroup;
    struct Grp {
        U4 x[GS / 8];
        F4 w[GS / 4], s[GS / 4];
    };
    auto run_chain = [&](int t) {
        const int b = t & 1;
        const uint32_t *xb = hub_lds_b + L::buf + (size_t)b * L::BUF + slot * 4;
        const float *sb = lds_f + L::scl + b * T;
        const float *wb = lds_f + L::wts + (size_t)b * kHubHeads * T + hl * T;
        const int cnt = (int)((n - (int64_t)t * T) < T ? (n - (int64_t)t * T) : T);
        auto fetch = [&](int j, Grp &q) {  // edges j .. j+GS-1 (j % 8 == 0): 16-B reads
#pragma unroll
            for (int u = 0; u < GS / 8; ++u) q.x[u] = *reinterpret_cast<const U4 *>(xb + ((j >> 3) + u) * OCT);
#pragma unroll
            for (int u = 0; u < GS / 4; ++u) {
                if (SRCS) q.s[u] = *reinterpret_cast<const F4 *>(sb + j + 4 * u);
                if (W) q.w[u] = *reinterpret_cast<const F4 *>(wb + j + 4 * u);
            }
        };
        auto consume = [&](const Grp &q) {
#pragma unroll
            for (int u = 0; u < GS / 8; ++u)
#pragma unroll
                for (int d = 0; d < 4; ++d) {  // dword d of the octet: edges 2d (low half), 2d + 1
                    const int e = 8 * u + 2 * d;
                    add(q.x[u][d] << 16, W ? q.w[e / 4][e % 4] : 1.0f, SRCS ? q.s[e / 4][e % 4] : 1.0f);
                    add(q.x[u][d] & 0xffff0000u, W ? q.w[e / 4][e % 4 + 1] : 1.0f, SRCS ? q.s[e / 4][e % 4 + 1] : 1.0f);
                }
        };
        // three groups in rotation, each read two groups ahead of its adds (as k_spmm_hub_exact);
        // the prefetch past the last full round reads at most two groups past the buffer (the
        // other buffer or the slack) and is never consumed
        int j = 0;
        const int full = cnt / (3 * GS) * (3 * GS);
        if (full > 0) {
            Grp A, B, C;
            fetch(0, A);
            fetch(GS, B);
            for (; j < full; j += 3 * GS) {
                fetch(j + 2 * GS, C);
                __builtin_amdgcn_sched_barrier(0);
                consume(A);
                __builtin_amdgcn_sched_barrier(0);
                fetch(j + 3 * GS, A);
                __builtin_amdgcn_sched_barrier(0);
                consume(B);
                __builtin_amdgcn_sched_barrier(0);
                fetch(j + 4 * GS, B);
                __builtin_amdgcn_sched_barrier(0);
                consume(C);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        for (; j + GS <= cnt; j += GS) {
            Grp A;
            fetch(j, A);
            consume(A);
        }
        for (; j < cnt; ++j) {
            const uint32_t d = xb[(j >> 3) * OCT + ((j >> 1) & 3)];
            add((j & 1) ? d & 0xffff0000u : d << 16, W ? wb[j] : 1.0f, SRCS ? sb[j] : 1.0f);
        }
    };

    // ---- pipeline: tile t in buffer t&1 is added while tile t+1 is gathered into the other ----
    if (gatherer && ntiles > 0) {
        load_cols(0);
        load_x(0);
        if (ntiles > 1) load_cols(1);
        store(0);
        if (ntiles > 1) {
            load_x(1);
            if (ntiles > 2) load_cols(2);
        }
    }
    __syncthreads();
    if (chain && from_y) acc = lds_f[L::yinit + lane];
    for (int t = 0; t < ntiles; ++t) {
        if (gatherer) {
            if (t + 1 < ntiles) {
                store((t + 1) & 1);
                if (t + 2 < ntiles) {
                    load_x(t + 2);
                    if (t + 3 < ntiles) load_cols(t + 3);
                }
            }
        } else {
            run_chain(t);
        }
        __syncthreads();
    }
    if (!chain) return;
    float out = acc;
    bool has_ds;
    const float ds = dst_factor_b(p, row, has_ds);
    if (has_ds) {
        out = __fmul_rn(ds, out);
        if (p.accum) out = __fadd_rn(p.Y[row * p.ldy + f], out);
    }
    p.Y[row * p.ldy + f] = out;
    if (p.Y2) {
        const float o2 = __fmul_rn(p.y2_scale ? p.y2_scale[row] : ds, out);
        if (p.y2_bf16) static_cast<bf16_t *>(p.Y2)[row * p.ldy2 + f] = bf16_rne(o2);
        else static_cast<float *>(p.Y2)[row * p.ldy2 + f] = o2;
    }
}

// fp32 X with a bf16 Y2: the hub rows' Y comes from k_spmm_hub_exact; this rounds their Y2 from it
__global__ __launch_bounds__(kBlock) void k_spmm_bf16_hub_y2(Bf16Params p, Bf16Hub hp) {
    const int64_t row = hp.rows[blockIdx.x];
    bool has_ds;
    const float ds = dst_factor_b(p, row, has_ds);
    const float s2 = p.y2_scale ? p.y2_scale[row] : ds;
    for (int f = threadIdx.x; f < p.F; f += kBlock)
        static_cast<bf16_t *>(p.Y2)[row * p.ldy2 + f] = bf16_rne(__fmul_rn(s2, p.Y[row * p.ldy + f]));
}

// ---- dispatch ---------------------------------------------------------------------------
template <class XT, int XV, int G, int CH>
static void rows_flags(const Bf16Params &p, hipStream_t st) {
    // U: edges in flight per lane.  A packed row costs CH * NW VGPRs per edge; 32 VGPRs of
    // gathered rows per lane as the fp32 kernel's widest setting, i.e. twice its edges
    constexpr int NW = Raw<XT, XV>::NW;
    constexpr int U = 32 / (CH * NW) > 8 ? 8 : 32 / (CH * NW) < 2 ? 2 : 32 / (CH * NW);
    constexpr int rows_per_block = (kBlock / kWave) * (kWave / G);
    const dim3 grid((unsigned)((p.n_rows + rows_per_block - 1) / rows_per_block));
    const bool w = p.val != nullptr, s = p.src_scale != nullptr;
    if (w && s) hipLaunchKernelGGL((k_spmm_bf16_rows<XT, XV, G, CH, U, true, true>), grid, dim3(kBlock), 0, st, p);
    else if (w) hipLaunchKernelGGL((k_spmm_bf16_rows<XT, XV, G, CH, U, true, false>), grid, dim3(kBlock), 0, st, p);
    else if (s) hipLaunchKernelGGL((k_spmm_bf16_rows<XT, XV, G, CH, U, false, true>), grid, dim3(kBlock), 0, st, p);
    else hipLaunchKernelGGL((k_spmm_bf16_rows<XT, XV, G, CH, U, false, false>), grid, dim3(kBlock), 0, st, p);
}

// L vectors per row -> the smallest group that covers them; past 32 lanes a lane takes two or
// four chunks, so a wave keeps at least two rows up to 64 vectors (F = 512 in 16-B vectors)
template <class XT, int XV>
static int rows_shape(const Bf16Params &p, hipStream_t st) {
    const int L = (p.F + XV - 1) / XV;
    if (L <= 1) rows_flags<XT, XV, 1, 1>(p, st);
    else if (L <= 2) rows_flags<XT, XV, 2, 1>(p, st);
    else if (L <= 4) rows_flags<XT, XV, 4, 1>(p, st);
    else if (L <= 8) rows_flags<XT, XV, 8, 1>(p, st);
    else if (L <= 16) rows_flags<XT, XV, 16, 1>(p, st);
    else if (L <= 32) rows_flags<XT, XV, 32, 1>(p, st);
    else if (L <= 64) rows_flags<XT, XV, 32, 2>(p, st);
    else if (L <= 128) rows_flags<XT, XV, 64, 2>(p, st);
    else if (L <= kBf16MaxVecs) rows_flags<XT, XV, 64, 4>(p, st);
    else return GALA_ERR_INVALID_ARG;  // the dispatch cuts wider rows into column ranges
    return launch_status();
}

int bf16_launch_rows(const Bf16Params &p, bool x_bf16, int xv, hipStream_t st) {
    if (x_bf16) {
        if (xv == 8) return rows_shape<bf16_t, 8>(p, st);
        if (xv == 4) return rows_shape<bf16_t, 4>(p, st);
        if (xv == 2) return rows_shape<bf16_t, 2>(p, st);
        return rows_shape<bf16_t, 1>(p, st);
    }
    if (xv == 4) return rows_shape<float, 4>(p, st);
    if (xv == 2) return rows_shape<float, 2>(p, st);
    return rows_shape<float, 1>(p, st);
}

template <int XV, int FSP, bool W, bool SRCS>
static void hub_t(const Bf16Params &p, Bf16Hub hp, hipStream_t st) {
    constexpr size_t lds = HubLdsB<XV, FSP, W, SRCS>::dwords * sizeof(uint32_t);
    // more than the default 64 KB of dynamic LDS (gfx950 has 160 KB per CU): opt in once
    static const hipError_t opted = hipFuncSetAttribute((const void *)k_spmm_bf16_hub<XV, FSP, W, SRCS>,
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)opted;
    hp.n_slices = (p.F + FSP - 1) / FSP;
    hipLaunchKernelGGL((k_spmm_bf16_hub<XV, FSP, W, SRCS>), dim3((unsigned)(hp.n_hub * hp.n_slices)),
                       dim3(kHubThreads), lds, st, p, hp);
}

template <int XV>
static void hub_v(const Bf16Params &p, const Bf16Hub &hp, hipStream_t st) {
    const bool w = p.val != nullptr, s = p.src_scale != nullptr;
#define GALA_HUB_B(S)                                    \
    if (w && s) hub_t<XV, S, true, true>(p, hp, st);     \
    else if (w) hub_t<XV, S, true, false>(p, hp, st);    \
    else if (s) hub_t<XV, S, false, true>(p, hp, st);    \
    else hub_t<XV, S, false, false>(p, hp, st);
    // slices of 32 features when F <= 32, else of 64 (one chain lane per feature of a wave)
    if (p.F <= 32) { GALA_HUB_B(32) } else { GALA_HUB_B(64) }
#undef GALA_HUB_B
}

int bf16_launch_hub(const Bf16Params &p, Bf16Hub hp, int xv, hipStream_t st) {
    if (xv == 8) hub_v<8>(p, hp, st);
    else if (xv == 4) hub_v<4>(p, hp, st);
    else if (xv == 2) hub_v<2>(p, hp, st);
    else hub_v<1>(p, hp, st);
    return launch_status();
}

int bf16_launch_hub_y2(const Bf16Params &p, Bf16Hub hp, hipStream_t st) {
    hipLaunchKernelGGL(k_spmm_bf16_hub_y2, dim3((unsigned)hp.n_hub), dim3(kBlock), 0, st, p, hp);
    return launch_status();
}

int bf16_pick_vec(bool x_bf16, const void *X, int64_t ldx, const float *Y, int64_t ldy, const void *Y2,
                  int64_t ldy2, bool y2_bf16, int32_t F, int32_t head_dim, bool one_head) {
    auto ok = [&](int v) {
        const int yv = v < 4 ? v : 4;  // Y (and an fp32 Y2) in vectors of yv floats
        const int64_t Fv = ((int64_t)F + v - 1) / v * v;
        const bool padded = one_head && ldx >= Fv && ldy >= Fv && (!Y2 || ldy2 >= Fv);
        const bool fits = (F % v == 0 && head_dim % v == 0) || padded;
        const bool x_ok = ldx % v == 0 && (uintptr_t)X % (size_t)(v * (x_bf16 ? 2 : 4)) == 0;
        const bool y_ok = ldy % yv == 0 && (uintptr_t)Y % (size_t)(4 * yv) == 0;
        const bool y2_ok = !Y2 || (y2_bf16 ? ldy2 % v == 0 && (uintptr_t)Y2 % (size_t)(2 * v) == 0
                                           : ldy2 % yv == 0 && (uintptr_t)Y2 % (size_t)(4 * yv) == 0);
        return fits && x_ok && y_ok && y2_ok;
    };
    int v = x_bf16 ? 8 : 4;
    while (v > 1 && !ok(v)) v >>= 1;
    return v;
}

}  // namespace gala
