// gat_exact_wide.hip -- the exact GAT pair (gat_exact.hip: the stable softmax of
// GALA_SOFTMAX_FIXED and its true gradients from row statistics) for rows of 257 .. 1024
// floats: 8 x 64, 5 x 64, 2 x 384, one head of 260.
//
// The work split is gat_wide.hip's (gat_wide_lanes.h): one wave per row, CH float4 slices per
// lane, the U * H (edge, head) pairs of a batch dealt over the lanes and evaluated once each
// into a per-wave LDS tile, head dots by fma chain, group butterfly and in-order re-add.
//
// Forward: the batch max per head is taken from the tile by lane h < H; a batch that raises
// some head's max rescales acc, accm, sum and sma once through a per-head factor in LDS (a
// batch that raises none skips the pass: the factor would be 1).  The logits in the tile are
// then replaced by exp(z - max) and m exp(z - max), which every lane reads per edge and slice.
//
// Backward: a row-local pre-pass (g, d_aL, the side line {aL, lse, g, 0} per (row, head)), then
// the gather: row c over its stored neighbours r, the U dY rows of a batch requested before
// any use, each pair's lane reading r's side line as one 16-byte vector and rebuilding
// alpha = exp(LeakyReLU(aL[r] + aR[c]) - lse[r]); dX and dXm accumulate by fmaf in CSR order.
#include "gat_exact_wide.h"
#include "gat_wide_lanes.h"

namespace gala {

typedef float F4 __attribute__((ext_vector_type(4)));

// Per-wave LDS as WideCfg lays it out: tile[2][U*H], aux[U*H], hv[64], red[U][GW].
// Forward: tile[b & 1] holds batch b's logits, then its exp terms; aux m * exp; hv the rescale
// factor (later 1 / sum) at h and the running max at 32 + h.
template <int CH, bool RC>
__global__ __launch_bounds__(kBlock) void k_gat_exact_wide_fwd(EdgeParams p, GatDev d, ExactDev x, WideCfg w) {
    constexpr int U = wide_u(CH), NT = U / 2;
    GALA_ROW_PROLOGUE(64);
    if (!row_ok) return;
    extern __shared__ float exact_wide_lds[];
    float *ws = exact_wide_lds + (threadIdx.x / kWave) * w.per_wave;
    const int H = p.heads, D = d.F / H, UH = U * H;
    float *tile = ws, *aux = ws + 2 * UH, *hv = ws + 3 * UH, *red = hv + 64;
    const WideLane<CH> ln(lane, d.F, D);
    const WidePairs<U> pr(lane, H);
    float pal[NT], pb[NT], wr[CH][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        pal[t] = d.aL[row * H + pr.h[t]];
        pb[t] = (RC && d.bR) ? d.bR[pr.h[t]] : 0.0f;
    }
    if (lane < 32) hv[32 + lane] = -INFINITY;  // a head whose logits are never finite keeps it
    if constexpr (RC) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) wr[ch][i] = ln.valid[ch] ? d.wR[ln.off[ch] + i] : 0.0f;
        // the row's own source logit for the backward's alpha: X[row] through the very
        // reduction its edges take (same fma order, butterfly and group order)
        if (d.ar_out) {
            float part[1][CH];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) part[0][ch] = dot4(wr[ch], ln.load(d.X + row * d.ldx, ch, false));
            head_dots_put<CH, 1>(part, red, w, lane);
            lds_sync();
            if (lane < H)
                d.ar_out[row * H + lane] = __fadd_rn(head_dots_get(red, w, 0, lane), d.bR ? d.bR[lane] : 0.0f);
        }
    }
    lds_sync();
    float acc[CH][4], accm[CH][4];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[ch][i] = accm[ch][i] = 0.0f;
    float m = -INFINITY, sum = 0.0f, sma = 0.0f;  // lane h < H: head h's running state
    int64_t e0, e1;
    row_range(p, 0, row, e0, e1);
    const int32_t n = (int32_t)(e1 - e0);
    int32_t win = 0;  // the row's next 64 column indices (load_batch_cols_win)
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V4 xv[U][CH];
        load_batch_cols_win<64, U>(p, e0, n, j0, win, c);
        float ar[NT];
        if constexpr (!RC) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                ar[t] = 0.0f;
                if (64 * t < UH) {
                    const int32_t cj = __shfl(win, (j0 & 63) + pr.k[t], 64);
                    ar[t] = d.aR[(int64_t)cj * H + pr.h[t]];
                }
            }
        }
        // given source logits: the rows are loaded nontemporal (they must not evict the aR table)
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) xv[k][ch] = ln.load(d.X + c[k] * d.ldx, ch, !RC);
        if constexpr (RC) {
            float part[U][CH];
#pragma unroll
            for (int k = 0; k < U; ++k)
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) part[k][ch] = dot4(wr[ch], xv[k][ch]);
            head_dots_put<CH, U>(part, red, w, lane);
            lds_sync();
#pragma unroll
            for (int t = 0; t < NT; ++t)
                ar[t] = (64 * t < UH) ? __fadd_rn(head_dots_get(red, w, pr.k[t], pr.h[t]), pb[t]) : 0.0f;
        }
        float *cur = tile + ((j0 / U) & 1) * UH;
        float z[NT];
        bool pos[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float s = __fadd_rn(pal[t], ar[t]);  // the two fp32 operands of every pass
            pos[t] = s > 0.0f;
            z[t] = pos[t] ? s : __fmul_rn(s, d.slope);
            if (pr.v[t]) cur[lane + 64 * t] = z[t];
        }
        lds_sync();
        const int nb = (n - j0 < U) ? n - j0 : U;
        // the batch maximum per head from the tile.  As in the narrow kernels, a head whose
        // logits so far are all -inf keeps m = -inf and its terms are NaN: finite logits are assumed.
        float mb = -INFINITY;
        if (lane < H)
            for (int k = 0; k < nb; ++k) mb = fmaxf(mb, cur[k * H + lane]);
        const bool up = lane < H && mb > m;
        if (__any(up)) {  // wave-uniform: one rescale of the whole state
            if (lane < H) {
                float r = 1.0f;
                if (up) {
                    r = (m == -INFINITY) ? 0.0f : expf(m - mb);
                    sum = __fmul_rn(sum, r);
                    sma = __fmul_rn(sma, r);
                    m = mb;
                }
                hv[lane] = r;
                hv[32 + lane] = m;
            }
            lds_sync();
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const float r = hv[ln.hd[ch]];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[ch][i] = __fmul_rn(acc[ch][i], r);
                    accm[ch][i] = __fmul_rn(accm[ch][i], r);
                }
            }
        }
        lds_sync();  // the logits are read: their slots take the exp terms
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (!pr.v[t]) continue;
            const float pe = expf(z[t] - hv[32 + pr.h[t]]);
            cur[lane + 64 * t] = pe;
            aux[lane + 64 * t] = pos[t] ? pe : __fmul_rn(pe, d.slope);
        }
        lds_sync();
        if (lane < H) {
            for (int k = 0; k < nb; ++k) {
                sum = __fadd_rn(sum, cur[k * H + lane]);
                sma = __fadd_rn(sma, aux[k * H + lane]);
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    const float pk = cur[k * H + ln.hd[ch]];
                    const float mk = aux[k * H + ln.hd[ch]];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[ch][i] = fmaf(pk, xv[k][ch][i], acc[ch][i]);
                        accm[ch][i] = fmaf(mk, xv[k][ch][i], accm[ch][i]);
                    }
                }
            }
        }
        lds_sync();  // aux / hv / red are rewritten by the next batch
    }
    // Y = acc / sum, Ym = accm / sum, sma / sum, lse = m + log(sum); an empty row gets zeros
    if (lane < H) {
        const bool empty = sum == 0.0f;
        const float q = empty ? 0.0f : 1.0f / sum;
        hv[lane] = q;
        d.sma_out[row * H + lane] = __fmul_rn(sma, q);
        x.lse_out[row * H + lane] = empty ? 0.0f : __fadd_rn(m, logf(sum));
    }
    lds_sync();
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const float q = hv[ln.hd[ch]];
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(acc[ch][i], q);
        ln.store(d.Y + row * d.ldy, ch, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(accm[ch][i], q);
        ln.store(d.ym_out + row * d.ldym, ch, o);
    }
}

// Row-local pre-pass (streams dY, Y, Ym once): g = <dY, Y>_h, d_aL = <dY, Ym>_h - g * sma, and
// the row's side line {aL, lse, g, 0} per head, one 16-byte store (the narrow layout)
template <int CH>
__global__ __launch_bounds__(kBlock) void k_gat_exact_wide_bwd_pre(EdgeParams p, GatDev d, ExactDev x, WideCfg w) {
    GALA_ROW_PROLOGUE(64);
    if (!row_ok) return;
    extern __shared__ float exact_wide_lds[];
    float *ws = exact_wide_lds + (threadIdx.x / kWave) * w.per_wave;
    const int H = p.heads, D = d.F / H;
    float *red = ws + 3 * wide_u(CH) * H + 64;
    const WideLane<CH> ln(lane, d.F, D);
    float part[2][CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const V4 dy = ln.load(d.dY + row * d.lddy, ch, false);
        const float dyv[4] = {dy[0], dy[1], dy[2], dy[3]};
        part[0][ch] = dot4(dyv, ln.load(d.ys + row * d.ldy, ch, false));
        part[1][ch] = dot4(dyv, ln.load(d.yms + row * d.ldym, ch, false));
    }
    head_dots_put<CH, 2>(part, red, w, lane);
    lds_sync();
    if (lane >= H) return;
    const int64_t o = row * H + lane;
    const float g = head_dots_get(red, w, 0, lane);
    const float s1 = head_dots_get(red, w, 1, lane);
    d.d_aL[o] = __fsub_rn(s1, __fmul_rn(g, d.smas[o]));
    F4 line;
    line.x = d.aL[o], line.y = x.lse[o], line.z = g, line.w = 0.0f;
    *reinterpret_cast<F4 *>(x.side + o * 4) = line;
}

// The gather pass: row c (d.aR[c, h] its own source logit) over its stored neighbours r.
// LDS: tile[0] alpha, tile[1] m alpha, aux m alpha g[r], red the epilogue's dot partials.
template <int CH>
__global__ __launch_bounds__(kBlock) void k_gat_exact_wide_bwd(EdgeParams p, GatDev d, ExactDev x, WideCfg w) {
    constexpr int U = wide_u(CH), NT = U / 2;
    GALA_ROW_PROLOGUE(64);
    if (!row_ok) return;
    extern __shared__ float exact_wide_lds[];
    float *ws = exact_wide_lds + (threadIdx.x / kWave) * w.per_wave;
    const int H = p.heads, D = d.F / H, UH = U * H;
    float *ta = ws, *tm = ws + UH, *tg = ws + 2 * UH, *red = ws + 3 * UH + 64;
    const WideLane<CH> ln(lane, d.F, D);
    const WidePairs<U> pr(lane, H);
    float par[NT], dx[CH][4], dxm[CH][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) par[t] = d.aR[row * H + pr.h[t]];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) dx[ch][i] = dxm[ch][i] = 0.0f;
    float sg = 0.0f;  // lane h < H: head h's sum of m alpha g[r]
    int64_t e0, e1;
    row_range(p, 0, row, e0, e1);
    const int32_t n = (int32_t)(e1 - e0);
    int32_t win = 0;
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V4 yv[U][CH];
        load_batch_cols_win<64, U>(p, e0, n, j0, win, c);
        // nontemporal: the gathered dY rows must not evict the side lines every edge also reads
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) yv[k][ch] = ln.load(d.dY + c[k] * d.lddy, ch, true);
        // consecutive lanes: consecutive heads of one neighbour's 16 * H bytes
        F4 sd[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sd[t] = F4{0.0f, 0.0f, 0.0f, 0.0f};
            if (64 * t < UH) {
                const int32_t cj = __shfl(win, (j0 & 63) + pr.k[t], 64);
                sd[t] = *reinterpret_cast<const F4 *>(x.side + ((int64_t)cj * H + pr.h[t]) * 4);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float s = __fadd_rn(sd[t].x, par[t]);  // aL[r] + aR[c], the forward's two operands
            const bool pos = s > 0.0f;
            const float z = pos ? s : __fmul_rn(s, d.slope);
            const float a = expf(z - sd[t].y);
            const float ma = pos ? a : __fmul_rn(a, d.slope);
            if (pr.v[t]) {
                ta[lane + 64 * t] = a;
                tm[lane + 64 * t] = ma;
                tg[lane + 64 * t] = __fmul_rn(ma, sd[t].z);
            }
        }
        lds_sync();
        if (lane < H) {
            const int nb = (n - j0 < U) ? n - j0 : U;
            for (int k = 0; k < nb; ++k) sg = __fadd_rn(sg, tg[k * H + lane]);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    const float ak = ta[k * H + ln.hd[ch]];
                    const float mk = tm[k * H + ln.hd[ch]];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dx[ch][i] = fmaf(ak, yv[k][ch][i], dx[ch][i]);
                        dxm[ch][i] = fmaf(mk, yv[k][ch][i], dxm[ch][i]);
                    }
                }
            }
        }
        lds_sync();  // the tile is rewritten by the next batch
    }
    // dX[c] and d_aR[c] = <dXm[c], X[c]>_h - sg[c]
    float part[1][CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        ln.store(d.dX + row * d.lddx, ch, dx[ch]);
        part[0][ch] = dot4(dxm[ch], ln.load(d.X + row * d.ldx, ch, false));
    }
    head_dots_put<CH, 1>(part, red, w, lane);
    lds_sync();
    if (lane < H) x.d_aR[row * H + lane] = __fsub_rn(head_dots_get(red, w, 0, lane), sg);
}

template <int CH>
static int exact_wide_fwd_rc(const EdgeParams &p, const GatDev &d, const ExactDev &x, hipStream_t hs) {
    return d.aR ? launch_wide(k_gat_exact_wide_fwd<CH, false>, p, d.F, CH, hs, d, x)
                : launch_wide(k_gat_exact_wide_fwd<CH, true>, p, d.F, CH, hs, d, x);
}

int gat_exact_wide_fwd(const EdgeParams &p, const GatDev &d, const ExactDev &x, hipStream_t hs) {
    switch ((d.F + 255) / 256) {
        case 2: return exact_wide_fwd_rc<2>(p, d, x, hs);
        case 3: return exact_wide_fwd_rc<3>(p, d, x, hs);
        default: return exact_wide_fwd_rc<4>(p, d, x, hs);
    }
}

template <int CH>
static int exact_wide_bwd_ch(const EdgeParams &p, const EdgeParams &pt, const GatDev &d, const ExactDev &x,
                             hipStream_t hs) {
    const int st = launch_wide(k_gat_exact_wide_bwd_pre<CH>, p, d.F, CH, hs, d, x);
    return st ? st : launch_wide(k_gat_exact_wide_bwd<CH>, pt, d.F, CH, hs, d, x);
}

int gat_exact_wide_bwd(const EdgeParams &p, const EdgeParams &pt, const GatDev &d, const ExactDev &x, hipStream_t hs) {
    switch ((d.F + 255) / 256) {
        case 2: return exact_wide_bwd_ch<2>(p, pt, d, x, hs);
        case 3: return exact_wide_bwd_ch<3>(p, pt, d, x, hs);
        default: return exact_wide_bwd_ch<4>(p, pt, d, x, hs);
    }
}

}  // namespace gala
