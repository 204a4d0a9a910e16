// gat_wide.hip -- the fused GAT forward (REF, FIXED), the REF row-statistics forward and the
// REF row-statistics backward for rows of 257 .. 1024 floats (8 x 64, 4 x 128, one head of
// 512: the widths the one-float4-per-lane kernels of gat.hip / gat_fused.hip refuse).
//
// One wave walks one row.  Lane l owns CH = ceil(F / 256) float4 slices, slice ch holding
// floats 256 ch + 4 l .. + 3; D = F / heads is a multiple of 4, so a slice lies in one head,
// whose index the lane keeps per slice (a head may span slices, a slice may hold several
// heads, the last slice may be ragged).  The per-edge scalar work of a batch of U edges --
// its U * H (edge, head) pairs -- is dealt over the 64 lanes (pair i = lane + 64 t: edge i / H,
// head i % H, so consecutive lanes read consecutive floats of aR[col] and store consecutive
// floats of alpha / p), each pair evaluated once.  The terms go to a per-wave LDS tile [U][H]
// from which every lane reads, per edge and slice, the one term of its slice's head, and
// from which lane h < H adds head h's running sums in edge order.  The accumulation is
// sequential in CSR order, fmaf(p, x, acc): per head the chain of the narrow kernels, so REF
// results with given source logits equal theirs bit for bit on every 256-float column block
// that holds whole heads.
//
// The LDS of a wave is private to it: DS operations of one wave execute in issue order, so
// a tile written by some lanes is read by others after a compiler-level fence (lds_sync); no
// workgroup barrier (the four waves of a block walk rows of different lengths).
// The lane view, the pair deal and the head-dot scheme: gat_wide_lanes.h.
#include "gat_wide.h"
#include "gat_wide_lanes.h"

namespace gala {

// ---- forward ---------------------------------------------------------------------------
template <int CH, int MODE, bool RC>
__global__ __launch_bounds__(kBlock) void k_gat_wide_fwd(EdgeParams p, GatDev d, WideCfg w) {
    constexpr int U = wide_u(CH), NT = U / 2;
    constexpr bool kRef = ref_mode(MODE), kStats = MODE == kRefStats;
    GALA_ROW_PROLOGUE(64);
    if (!row_ok) return;
    extern __shared__ float wide_lds[];
    float *ws = wide_lds + (threadIdx.x / kWave) * w.per_wave;
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
    if constexpr (RC) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) wr[ch][i] = ln.valid[ch] ? d.wR[ln.off[ch] + i] : 0.0f;
    }
    if constexpr (RC && kStats) {
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
            lds_sync();
        }
    }
    float acc[CH][4], accm[CH][4];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[ch][i] = accm[ch][i] = 0.0f;
    float m = -INFINITY, sum = 0.0f, sma = 0.0f;  // lane h < H: head h's running state
    int64_t e0, e1;
    row_range(p, 0, row, e0, e1);
    const int32_t n = (int32_t)(e1 - e0);
    const bool park = d.alpha_out != nullptr;
    int32_t win = 0;  // the row's next 64 column indices (load_batch_cols_win)
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V4 x[U][CH];
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
        // given source logits: the rows are loaded nontemporal (gat.hip, gat_fwd_range_dist)
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) x[k][ch] = ln.load(d.X + c[k] * d.ldx, ch, !RC);
        // The parked terms of a batch are stored one batch late, after this batch's loads are
        // issued (stores count in vmcnt: gat_fwd_range_dist); a previous batch is always full.
        if (park && j0 > 0) {
            const float *tp = tile + (((j0 / U) - 1) & 1) * UH;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (pr.v[t]) d.alpha_out[(e0 + j0 - U) * H + lane + 64 * t] = tp[lane + 64 * t];
        }
        if constexpr (RC) {
            float part[U][CH];
#pragma unroll
            for (int k = 0; k < U; ++k)
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) part[k][ch] = dot4(wr[ch], x[k][ch]);
            head_dots_put<CH, U>(part, red, w, lane);
            lds_sync();
#pragma unroll
            for (int t = 0; t < NT; ++t)
                ar[t] = (64 * t < UH) ? __fadd_rn(head_dots_get(red, w, pr.k[t], pr.h[t]), pb[t]) : 0.0f;
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
                cur[lane + 64 * t] = pe;
                if constexpr (kStats) aux[lane + 64 * t] = pos ? pe : __fmul_rn(pe, d.slope);
            } else {
                cur[lane + 64 * t] = z[t];
            }
        }
        lds_sync();
        const int nb = (n - j0 < U) ? n - j0 : U;
        if constexpr (!kRef) {
            // the batch maximum per head from the tile; the running state rescaled once.  As in
            // the narrow kernels (gat.hip, FIXED), a head whose logits so far are all -inf keeps
            // m = -inf and its terms are exp(-inf - -inf) = NaN: finite logits are assumed.
            if (lane < H) {
                float mb = -INFINITY, r = 1.0f;
                for (int k = 0; k < nb; ++k) mb = fmaxf(mb, cur[k * H + lane]);
                if (mb > m) {
                    r = (m == -INFINITY) ? 0.0f : expf(m - mb);
                    sum = __fmul_rn(sum, r);
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
                for (int i = 0; i < 4; ++i) acc[ch][i] = __fmul_rn(acc[ch][i], r);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (pr.v[t]) aux[lane + 64 * t] = expf(z[t] - hv[32 + pr.h[t]]);
            lds_sync();
        }
        const float *pt = kRef ? cur : aux;
        if (lane < H) {
            for (int k = 0; k < nb; ++k) {
                sum = __fadd_rn(sum, pt[k * H + lane]);
                if constexpr (kStats) sma = __fadd_rn(sma, aux[k * H + lane]);
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    const float pk = pt[k * H + ln.hd[ch]];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[ch][i] = fmaf(pk, x[k][ch][i], acc[ch][i]);
                    if constexpr (kStats) {
                        const float mk = aux[k * H + ln.hd[ch]];
#pragma unroll
                        for (int i = 0; i < 4; ++i) accm[ch][i] = fmaf(mk, x[k][ch][i], accm[ch][i]);
                    }
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
            if (pr.v[t] && jl + pr.k[t] < n) d.alpha_out[(e0 + jl) * H + lane + 64 * t] = tp[lane + 64 * t];
    }
    // Y = acc * q with q = 1 / (sum [+ S * 1e-12 in REF mode]), as gat_fwd_store
    if (lane < H) {
        const float den = kRef ? sum + (float)p.seg.n * 1e-12f : sum;
        const float q = (!kRef && sum == 0.0f) ? 0.0f : 1.0f / den;
        hv[lane] = q;
        hv[32 + lane] = m;
        if (d.q_out) d.q_out[row * H + lane] = q;
        if constexpr (kStats) d.sma_out[row * H + lane] = __fmul_rn(sma, q);
    }
    lds_sync();
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const float q = hv[ln.hd[ch]];
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(acc[ch][i], q);
        ln.store(d.Y + row * d.ldy, ch, o);
        if constexpr (kStats) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = __fmul_rn(accm[ch][i], q);
            ln.store(d.ym_out + row * d.ldym, ch, o);
        }
    }
    if (!d.alpha_out || d.q_out) return;  // factored: the parked exp terms are the output
    // alpha from the parked terms (REF) / logits (FIXED), stored by other lanes of this wave
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    float *ap = d.alpha_out + e0 * H;
    for (int32_t t = lane; t < n * H; t += 64) {
        const int h = t % H;
        const float pe = kRef ? ap[t] : expf(ap[t] - hv[32 + h]);
        ap[t] = __fmul_rn(pe, hv[h]);
    }
}

// ---- row-statistics backward -------------------------------------------------------------
// dX = A_alpha dY with alpha = fl(p * q) rebuilt per (edge, head) pair from aR (or the
// forward's p), gathering dY[col] only; d_aL from the row's Y, Ym, sma and dY[row].
// FP: alpha = fl(p * q) from the forward's p (d.alpha) instead of the logits.  d.attn_w (the
// source logit's per-head Linear): dX also takes d_aL * attn_w at the store (add_attn_linear).
template <int CH, bool FP>
__global__ __launch_bounds__(kBlock) void k_gat_wide_bwd_stats(EdgeParams p, GatDev d, WideCfg w) {
    constexpr int U = wide_u(CH), NT = U / 2;
    GALA_ROW_PROLOGUE(64);
    if (!row_ok) return;
    extern __shared__ float wide_lds[];
    float *ws = wide_lds + (threadIdx.x / kWave) * w.per_wave;
    const int H = p.heads, D = d.F / H, UH = U * H;
    float *tile = ws, *hv = ws + 3 * UH, *red = hv + 64;
    const WideLane<CH> ln(lane, d.F, D);
    const WidePairs<U> pr(lane, H);
    {   // d_aL = (<dY, Ym> - (<dY, Y> + eps) sma) + eps per head (stats_d_al, gat_fused.hip)
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
        if (lane < H) {
            const float eps = (float)p.seg.n * 1e-12f;
            const float acc = head_dots_get(red, w, 0, lane) + eps;
            const float s1 = head_dots_get(red, w, 1, lane);
            const float dal = (s1 - acc * d.smas[row * H + lane]) + eps;
            d.d_aL[row * H + lane] = dal;
            hv[lane] = dal;  // kept for the Linear's term at the store
        }
        lds_sync();
    }
    float pal[NT], pq[NT], dxa[CH][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        pal[t] = d.aL[row * H + pr.h[t]];
        pq[t] = d.q[row * H + pr.h[t]];
    }
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) dxa[ch][i] = 0.0f;
    int64_t e0, e1;
    row_range(p, 0, row, e0, e1);
    const int32_t n = (int32_t)(e1 - e0);
    int32_t win = 0;
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V4 yv[U][CH];
        load_batch_cols_win<64, U>(p, e0, n, j0, win, c);
        float sv[NT];  // the pair's source logit, or (FP) its exp term p
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sv[t] = 0.0f;
            if (64 * t < UH) {
                if constexpr (FP) {
                    const int32_t j = (j0 + pr.k[t] < n) ? j0 + pr.k[t] : n - 1;
                    sv[t] = d.alpha[(e0 + j) * H + pr.h[t]];
                } else {
                    const int32_t cj = __shfl(win, (j0 & 63) + pr.k[t], 64);
                    sv[t] = d.aR[(int64_t)cj * H + pr.h[t]];
                }
            }
        }
        // nontemporal: the gathered dY rows would evict the aR table (gat_fused.hip)
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) yv[k][ch] = ln.load(d.dY + c[k] * d.lddy, ch, true);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float pe = sv[t];
            if constexpr (!FP) {
                const float s = __fadd_rn(pal[t], sv[t]);
                pe = ref_exp(s > 0.0f ? s : __fmul_rn(s, d.slope));
            }
            if (pr.v[t]) tile[lane + 64 * t] = __fmul_rn(pe, pq[t]);
        }
        lds_sync();
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + k < n) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    const float ak = tile[k * H + ln.hd[ch]];
#pragma unroll
                    for (int i = 0; i < 4; ++i) dxa[ch][i] = fmaf(ak, yv[k][ch][i], dxa[ch][i]);
                }
            }
        }
        lds_sync();  // the tile is rewritten by the next batch
    }
    if (d.attn_w) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            if (!ln.valid[ch]) continue;
            const float dal = hv[ln.hd[ch]];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dxa[ch][i] = __fadd_rn(dxa[ch][i], __fmul_rn(dal, d.attn_w[ln.off[ch] + i]));
        }
    }
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) ln.store(d.dX + row * d.lddx, ch, dxa[ch]);
}

template <int CH, int MODE>
static int wide_fwd_rc(const EdgeParams &p, const GatDev &d, hipStream_t hs) {
    return d.aR ? launch_wide(k_gat_wide_fwd<CH, MODE, false>, p, d.F, CH, hs, d)
                : launch_wide(k_gat_wide_fwd<CH, MODE, true>, p, d.F, CH, hs, d);
}

template <int CH>
static int wide_fwd_mode(const EdgeParams &p, const GatDev &d, int mode, hipStream_t hs) {
    if (mode == kRefStats) return wide_fwd_rc<CH, kRefStats>(p, d, hs);
    if (mode == GALA_SOFTMAX_REF) return wide_fwd_rc<CH, GALA_SOFTMAX_REF>(p, d, hs);
    return wide_fwd_rc<CH, GALA_SOFTMAX_FIXED>(p, d, hs);
}

bool gat_wide_shape(const gala_csr_t *A, int32_t F, int32_t heads, int vec) {
    return F > 256 && F <= 1024 && heads <= 32 && (F / heads) % 4 == 0 && vec == 4 && A->n_seg == 1 &&
           (!A->split || A->split->n_rows_split == 0);
}

int gat_wide_fwd(const EdgeParams &p, const GatDev &d, int mode, hipStream_t hs) {
    switch ((d.F + 255) / 256) {
        case 2: return wide_fwd_mode<2>(p, d, mode, hs);
        case 3: return wide_fwd_mode<3>(p, d, mode, hs);
        default: return wide_fwd_mode<4>(p, d, mode, hs);
    }
}

template <int CH>
static int wide_bwd_from(const EdgeParams &p, const GatDev &d, hipStream_t hs) {
    return d.alpha ? launch_wide(k_gat_wide_bwd_stats<CH, true>, p, d.F, CH, hs, d)
                   : launch_wide(k_gat_wide_bwd_stats<CH, false>, p, d.F, CH, hs, d);
}

int gat_wide_bwd_stats(const EdgeParams &p, const GatDev &d, hipStream_t hs) {
    switch ((d.F + 255) / 256) {
        case 2: return wide_bwd_from<2>(p, d, hs);
        case 3: return wide_bwd_from<3>(p, d, hs);
        default: return wide_bwd_from<4>(p, d, hs);
    }
}

}  // namespace gala
