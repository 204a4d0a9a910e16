// gat_exact.hip -- the GAT layer with its true gradients (the stable softmax of
// GALA_SOFTMAX_FIXED) from row statistics, on a symmetric pattern.
//
// Forward (gala_gat_fwd_stats_exact_f32): one pass per row with the online max, one rescale
// per U-edge batch; writes Y, Ym = sum m alpha X, sma = sum m alpha (m the LeakyReLU factor
// of the edge) and lse = max + log(sum), so that alpha_rc = exp(s_rc - lse_r) can be rebuilt
// from the two logits alone.  No alpha is stored.
//
// Backward (gala_gat_bwd_stats_exact_f32): a row-local pre-pass forms g[r] = <dY[r], Y[r]>_h,
// d_aL[r] = <dY[r], Ym[r]>_h - g[r] sma[r], and the side line {aL, lse, g, 0} per (row, head):
// 16 B per head, 128 B per row at 8 heads.  The gather pass walks row c's neighbours r (the
// in-edges (r, c) of a symmetric pattern), reads dY[r] and r's side line, rebuilds alpha_rc
// and accumulates dX[c] = sum alpha dY[r], dXm[c] = sum m alpha dY[r], sg[c] = sum m alpha g[r];
// d_aR[c] = <dXm[c], X[c]>_h - sg[c].  One gather of dY rows, no transposed graph, no E*H array.
//
// Both sums aL[r] + aR[c] have the same operands in the two passes, so an edge's LeakyReLU
// branch is the same in both.  Every sum is sequential in CSR order (hub rows: per-chunk
// partials added in ascending chunk order from the plan's workspace); no atomics.
//
// Directed pattern (gala_gat_bwd_stats_exact_t_f32): the in-edges of c are row c of A^T, so
// the same gather kernels walk A^T (its own hub plan and workspace) after the pre-pass over
// A's rows; gala_csr_is_transpose_i32 (csr_check.hip) is the test that the second pattern is
// the first one's transpose.
#include "gat_common.h"

namespace gala {

// Operands the exact pair has beyond GatDev's.
struct ExactDev {
    float *lse_out;      // forward [n, H]
    const float *lse;    // backward pre-pass [n, H]
    float *side;         // backward: [n, H, 4] = {aL, lse, g, 0}
    float *d_aR;         // backward [n, H]
    // the column of each row's own vertex when the pattern's columns index gathered tables
    // (X, aR, dY and side are then [n_cols, ...]); NULL: the row itself (square pattern)
    const int32_t *self_col;
};

__device__ __forceinline__ int64_t own_col(const ExactDev &x, int64_t row) {
    return x.self_col ? (int64_t)x.self_col[row] : row;
}

template <int VEC, int CH>
struct ExFwdState {
    float acc[CH][VEC], accm[CH][VEC];
    float m, sum, sma;
    __device__ __forceinline__ ExFwdState() : m(-INFINITY), sum(0.0f), sma(0.0f) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[ch][i] = accm[ch][i] = 0.0f;
    }
};

// Edges [e0, e1) of `row` into the forward state.  Edge k of a U-edge batch is worked by lane
// k mod UH of its head group (source logit, LeakyReLU, exp); the batch's max is taken over the
// group first and the running state rescaled once; the terms are then broadcast and added in
// CSR order.
template <int G, int VEC, int U, int CH, bool RC, int HW>
__device__ __forceinline__ void exact_fwd_range(const EdgeParams &p, const GatDev &d,
                                                const GatLane<G, VEC, CH, RC> &gl_, int64_t e0, int64_t e1,
                                                ExFwdState<VEC, CH> &st) {
    typedef typename GVec<VEC>::T V;
    constexpr int UH = (U < HW) ? U : HW;
    constexpr int NK = U / UH;
    const int H = gl_.H, hh = gl_.hh;
    const int lane = threadIdx.x & (kWave - 1);
    const int hl = lane & (HW - 1);
    const int kl = hl % UH;
    const int32_t n = (int32_t)(e1 - e0);
    int32_t win = 0;
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V x[U][CH];
        load_batch_cols_win<G, U>(p, e0, n, j0, win, c);
        float ar[NK];
        if (!RC) {
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const int32_t j = (j0 + kl + i * UH < n) ? j0 + kl + i * UH : n - 1;
                ar[i] = d.aR[(int64_t)p.col[e0 + j] * H + hh];
            }
        }
        // given source logits: nontemporal rows keep the aR table cached (as k_gat_fwd)
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const V *xp = reinterpret_cast<const V *>(d.X + c[k] * d.ldx + gl_.ln.off[ch]);
                x[k][ch] = mask_pad<VEC>(gl_.ln.nv[ch], RC ? *xp : __builtin_nontemporal_load(xp));
            }
        if (RC) {
            float all[U];
#pragma unroll
            for (int k = 0; k < U; ++k) all[k] = __fadd_rn(attn_dot<HW, VEC, CH>(gl_.w, x[k]), gl_.wb);
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                float v = all[0];
#pragma unroll
                for (int k = 1; k < U; ++k) v = (kl + i * UH == k) ? all[k] : v;
                ar[i] = v;
            }
        }
        float pe[NK], mp[NK], z[NK];
        bool pos[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const float t = __fadd_rn(gl_.al, ar[i]);
            pos[i] = t > 0.0f;
            z[i] = pos[i] ? t : __fmul_rn(t, d.slope);
        }
        float mb = -INFINITY;
#pragma unroll
        for (int i = 0; i < NK; ++i) mb = (j0 + kl + i * UH < n) ? fmaxf(mb, z[i]) : mb;
        mb = group_max<HW>(mb);
        if (mb > st.m) {
            const float r = (st.m == -INFINITY) ? 0.0f : expf(st.m - mb);
            st.sum = __fmul_rn(st.sum, r);
            st.sma = __fmul_rn(st.sma, r);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch)
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    st.acc[ch][i] = __fmul_rn(st.acc[ch][i], r);
                    st.accm[ch][i] = __fmul_rn(st.accm[ch][i], r);
                }
            st.m = mb;
        }
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            pe[i] = expf(z[i] - st.m);
            mp[i] = pos[i] ? pe[i] : __fmul_rn(pe[i], d.slope);
        }
        static_for<0, U>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const float pk = group_bcast<HW, k % UH>(pe[k / UH]);
            const float mk = group_bcast<HW, k % UH>(mp[k / UH]);
            if (j0 + k >= n) return;
            st.sum = __fadd_rn(st.sum, pk);
            st.sma = __fadd_rn(st.sma, mk);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const float *xv = reinterpret_cast<const float *>(&x[k][ch]);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    st.acc[ch][i] = fmaf(pk, xv[i], st.acc[ch][i]);
                    st.accm[ch][i] = fmaf(mk, xv[i], st.accm[ch][i]);
                }
            }
        });
    }
}

// a[ch][i] of the lane's real columns -> base[off + i] (whole vectors where the lane has one)
template <int G, int VEC, int CH>
__device__ __forceinline__ void exact_store_row(const Lanes<G, VEC, CH> &ln, float *base,
                                                const float (&a)[CH][VEC], float scale) {
    typedef typename GVec<VEC>::T V;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        if (!ln.valid[ch]) continue;
        V out;
        float *ov = reinterpret_cast<float *>(&out);
#pragma unroll
        for (int i = 0; i < VEC; ++i) ov[i] = __fmul_rn(a[ch][i], scale);
        float *yp = base + ln.off[ch];
        if (ln.nv[ch] == VEC) {
            *reinterpret_cast<V *>(yp) = out;
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (ln.in(ch, i)) yp[i] = ov[i];
        }
    }
}

// Y = acc / sum, Ym = accm / sum, sma / sum, lse = m + log(sum); an empty row gets zeros
template <int G, int VEC, int CH, bool RC>
__device__ __forceinline__ void exact_fwd_store(const GatDev &d, const ExactDev &x,
                                                const GatLane<G, VEC, CH, RC> &gl_, int64_t row,
                                                const ExFwdState<VEC, CH> &st) {
    const bool empty = st.sum == 0.0f;
    const float q = empty ? 0.0f : 1.0f / st.sum;
    exact_store_row<G, VEC, CH>(gl_.ln, d.Y + row * d.ldy, st.acc, q);
    exact_store_row<G, VEC, CH>(gl_.ln, d.ym_out + row * d.ldym, st.accm, q);
    if (gl_.leader) {
        const int64_t o = row * gl_.H + gl_.hh;
        d.sma_out[o] = __fmul_rn(st.sma, q);
        x.lse_out[o] = empty ? 0.0f : __fadd_rn(st.m, logf(st.sum));
    }
}

template <int G, int VEC, int U, int CH, bool RC, int HW>
__global__ __launch_bounds__(kBlock) void k_gat_exact_fwd(EdgeParams p, GatDev d, ExactDev x,
                                                          int32_t split_threshold) {
    GALA_ROW_PROLOGUE(G);
    if (!row_ok) return;
    const GatLane<G, VEC, CH, RC> gl_(p, d, gl, row);
    if constexpr (RC) {
        // the row's own source logit for the backward, formed as the per-edge recompute forms
        // it (same lanes, fma order and butterfly), so both passes add the same two operands
        if (d.ar_out) {
            typedef typename GVec<VEC>::T V;
            V xr[CH];
            const int64_t s = own_col(x, row);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch)
                xr[ch] = mask_pad<VEC>(gl_.ln.nv[ch], *reinterpret_cast<const V *>(d.X + s * d.ldx + gl_.ln.off[ch]));
            const float a = __fadd_rn(attn_dot<HW, VEC, CH>(gl_.w, xr), gl_.wb);
            if (gl_.leader) d.ar_out[s * gl_.H + gl_.hh] = a;
        }
    }
    if (hub_row(p, split_threshold, row)) return;  // k_gat_exact_fwd_chunk / _fixup
    ExFwdState<VEC, CH> st;
    for (int s = 0; s < p.seg.n; ++s) {
        int64_t e0, e1;
        row_range(p, s, row, e0, e1);
        exact_fwd_range<G, VEC, U, CH, RC, HW>(p, d, gl_, e0, e1, st);
    }
    exact_fwd_store<G, VEC, CH, RC>(d, x, gl_, row, st);
}

// hub rows, forward: chunk partial state -> ws[c] = {acc[F], m[H], sum[H], accm[F], sma[H]}
template <int G, int VEC, int U, int CH, bool RC, int HW>
__global__ __launch_bounds__(kBlock) void k_gat_exact_fwd_chunk(EdgeParams p, GatDev d, HubSplit sp) {
    GALA_CHUNK_PROLOGUE(G);
    const GatLane<G, VEC, CH, RC> gl_(p, d, gl, row);
    ExFwdState<VEC, CH> st;
    exact_fwd_range<G, VEC, U, CH, RC, HW>(p, d, gl_, e0, e1, st);
    float *w = sp.ws + c * sp.ws_cols;
    float *wm = w + d.F + 2 * gl_.H;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (gl_.ln.in(ch, i)) {
                w[gl_.ln.off[ch] + i] = st.acc[ch][i];
                wm[gl_.ln.off[ch] + i] = st.accm[ch][i];
            }
    if (gl_.leader) {
        w[d.F + gl_.hh] = st.m;
        w[d.F + gl_.H + gl_.hh] = st.sum;
        wm[d.F + gl_.hh] = st.sma;
    }
}

// hub rows, forward: the chunk partials combined in ascending chunk order, each step rescaled
// to the larger max
template <int G, int VEC, int CH, bool RC>
__global__ __launch_bounds__(kBlock) void k_gat_exact_fwd_fixup(EdgeParams p, GatDev d, ExactDev x, HubSplit sp) {
    const int lane = threadIdx.x & (kWave - 1);
    const int gl = lane & (G - 1);
    const int64_t ri = ((int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * (kWave / G) + lane / G;
    if (ri >= sp.n_rows_split) return;
    const int64_t row = sp.rows[ri];
    const GatLane<G, VEC, CH, RC> gl_(p, d, gl, row);
    const int F = d.F, H = gl_.H, hh = gl_.hh;
    ExFwdState<VEC, CH> st;
    for (int64_t cc = sp.row_chunk0[ri]; cc < sp.row_chunk0[ri + 1]; ++cc) {
        const float *w = sp.ws + cc * sp.ws_cols;
        const float *wm = w + F + 2 * H;
        const float mc = w[F + hh];
        if (mc == -INFINITY) continue;  // no edges in this chunk's partial
        const float mn = fmaxf(st.m, mc);
        const float a = (st.m == -INFINITY) ? 0.0f : expf(st.m - mn);
        const float b = expf(mc - mn);
        st.m = mn;
        st.sum = fmaf(st.sum, a, __fmul_rn(w[F + H + hh], b));
        st.sma = fmaf(st.sma, a, __fmul_rn(wm[F + hh], b));
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const bool in = gl_.ln.in(ch, i);
                st.acc[ch][i] = fmaf(st.acc[ch][i], a, __fmul_rn(in ? w[gl_.ln.off[ch] + i] : 0.0f, b));
                st.accm[ch][i] = fmaf(st.accm[ch][i], a, __fmul_rn(in ? wm[gl_.ln.off[ch] + i] : 0.0f, b));
            }
    }
    exact_fwd_store<G, VEC, CH, RC>(d, x, gl_, row, st);
}

// ---- backward -------------------------------------------------------------------------

// Row-local pre-pass (streams dY, Y, Ym once): g = <dY, Y>_h, d_aL = <dY, Ym>_h - g * sma, and
// the row's side line {aL, lse, g, 0} per head, one 16-byte store
template <int G, int VEC, int CH, int HW>
__global__ __launch_bounds__(kBlock) void k_gat_exact_bwd_pre(EdgeParams p, GatDev d, ExactDev x) {
    GALA_ROW_PROLOGUE(G);
    if (!row_ok) return;
    typedef typename GVec<VEC>::T V;
    const GatLane<G, VEC, CH, false> gl_(p, d, gl, row);
    float dy[CH][VEC];
    load_dy<G, VEC, CH, false>(d, gl_, row, dy);
    float syy = 0.0f, sym = 0.0f;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const V y = mask_pad<VEC>(gl_.ln.nv[ch], *reinterpret_cast<const V *>(d.ys + row * d.ldy + gl_.ln.off[ch]));
        const V ym = mask_pad<VEC>(gl_.ln.nv[ch], *reinterpret_cast<const V *>(d.yms + row * d.ldym + gl_.ln.off[ch]));
        const float *yv = reinterpret_cast<const float *>(&y);
        const float *mv = reinterpret_cast<const float *>(&ym);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            syy = fmaf(dy[ch][i], yv[i], syy);
            sym = fmaf(dy[ch][i], mv[i], sym);
        }
    }
    const float g = group_sum<HW>(syy);
    const float s1 = group_sum<HW>(sym);
    if (!gl_.leader) return;
    const int64_t o = row * gl_.H + gl_.hh;
    d.d_aL[o] = __fsub_rn(s1, __fmul_rn(g, d.smas[o]));
    typedef float F4 __attribute__((ext_vector_type(4)));
    F4 line;
    line.x = gl_.al, line.y = x.lse[o], line.z = g, line.w = 0.0f;
    *reinterpret_cast<F4 *>(x.side + (own_col(x, row) * gl_.H + gl_.hh) * 4) = line;
}

template <int VEC, int CH>
struct ExBwdState {
    float dx[CH][VEC], dxm[CH][VEC];
    float sg;
    __device__ __forceinline__ ExBwdState() : sg(0.0f) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < VEC; ++i) dx[ch][i] = dxm[ch][i] = 0.0f;
    }
};

// Edges [e0, e1) of row c (gl_.al holds aR[c, h]): per edge the neighbour r's dY row and side
// line; alpha = exp(LeakyReLU(aL[r] + aR[c]) - lse[r]).  The owner lane of an edge forms
// alpha, m alpha and m alpha g; the three are broadcast and added in CSR order.
template <int G, int VEC, int U, int CH, int HW>
__device__ __forceinline__ void exact_bwd_range(const EdgeParams &p, const GatDev &d, const ExactDev &x,
                                                const GatLane<G, VEC, CH, false> &gl_, int64_t e0, int64_t e1,
                                                ExBwdState<VEC, CH> &st) {
    typedef typename GVec<VEC>::T V;
    typedef float F4 __attribute__((ext_vector_type(4)));
    constexpr int UH = (U < HW) ? U : HW;
    constexpr int NK = U / UH;
    const int H = gl_.H, hh = gl_.hh;
    const float ar = gl_.al;  // the gather's lane view is built over aR: this row's own source logit aR[c, h]
    const int lane = threadIdx.x & (kWave - 1);
    const int hl = lane & (HW - 1);
    const int kl = hl % UH;
    const int32_t n = (int32_t)(e1 - e0);
    int32_t win = 0;
    for (int32_t j0 = 0; j0 < n; j0 += U) {
        int64_t c[U];
        V yv[U][CH];
        load_batch_cols_win<G, U>(p, e0, n, j0, win, c);
        F4 sd[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int32_t j = (j0 + kl + i * UH < n) ? j0 + kl + i * UH : n - 1;
            sd[i] = *reinterpret_cast<const F4 *>(x.side + ((int64_t)p.col[e0 + j] * H + hh) * 4);
        }
        // nontemporal: the gathered dY rows must not evict the side lines every edge also reads
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch)
                yv[k][ch] = mask_pad<VEC>(gl_.ln.nv[ch], __builtin_nontemporal_load(reinterpret_cast<const V *>(
                                                             d.dY + c[k] * d.lddy + gl_.ln.off[ch])));
        float a[NK], ma[NK], mg[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const float t = __fadd_rn(sd[i].x, ar);  // aL[r] + aR[c], the forward's two operands
            const bool pos = t > 0.0f;
            const float z = pos ? t : __fmul_rn(t, d.slope);
            a[i] = expf(z - sd[i].y);
            ma[i] = pos ? a[i] : __fmul_rn(a[i], d.slope);
            mg[i] = __fmul_rn(ma[i], sd[i].z);
        }
        static_for<0, U>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const float ak = group_bcast<HW, k % UH>(a[k / UH]);
            const float mk = group_bcast<HW, k % UH>(ma[k / UH]);
            const float gk = group_bcast<HW, k % UH>(mg[k / UH]);
            if (j0 + k >= n) return;
            st.sg = __fadd_rn(st.sg, gk);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const float *yk = reinterpret_cast<const float *>(&yv[k][ch]);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    st.dx[ch][i] = fmaf(ak, yk[i], st.dx[ch][i]);
                    st.dxm[ch][i] = fmaf(mk, yk[i], st.dxm[ch][i]);
                }
            }
        });
    }
}

// dX[c] and d_aR[c] = <dXm[c], X[c]>_h - sg[c]; s: the table column of row c's own vertex
template <int G, int VEC, int CH, int HW>
__device__ __forceinline__ void exact_bwd_store(const GatDev &d, const ExactDev &x,
                                                const GatLane<G, VEC, CH, false> &gl_, int64_t row, int64_t s,
                                                const ExBwdState<VEC, CH> &st) {
    typedef typename GVec<VEC>::T V;
    exact_store_row<G, VEC, CH>(gl_.ln, d.dX + row * d.lddx, st.dx, 1.0f);
    float dot = 0.0f;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const V xr = mask_pad<VEC>(gl_.ln.nv[ch], *reinterpret_cast<const V *>(d.X + s * d.ldx + gl_.ln.off[ch]));
        const float *xv = reinterpret_cast<const float *>(&xr);
#pragma unroll
        for (int i = 0; i < VEC; ++i) dot = fmaf(st.dxm[ch][i], xv[i], dot);
    }
    dot = group_sum<HW>(dot);
    if (gl_.leader) x.d_aR[row * gl_.H + gl_.hh] = __fsub_rn(dot, st.sg);
}

template <int G, int VEC, int U, int CH, int HW>
__global__ __launch_bounds__(kBlock) void k_gat_exact_bwd(EdgeParams p, GatDev d, ExactDev x,
                                                          int32_t split_threshold) {
    GALA_ROW_PROLOGUE(G);
    if (!row_ok) return;
    if (hub_row(p, split_threshold, row)) return;  // k_gat_exact_bwd_chunk / _fixup
    const int64_t own = own_col(x, row);
    const GatLane<G, VEC, CH, false> gl_(p, d, gl, own);  // d.aL = the aR table: al = aR[own, h]
    ExBwdState<VEC, CH> st;
    for (int s = 0; s < p.seg.n; ++s) {
        int64_t e0, e1;
        row_range(p, s, row, e0, e1);
        exact_bwd_range<G, VEC, U, CH, HW>(p, d, x, gl_, e0, e1, st);
    }
    exact_bwd_store<G, VEC, CH, HW>(d, x, gl_, row, own, st);
}

// hub rows, backward: chunk partials -> ws[c] = {dX[F], dXm[F], sg[H]}
template <int G, int VEC, int U, int CH, int HW>
__global__ __launch_bounds__(kBlock) void k_gat_exact_bwd_chunk(EdgeParams p, GatDev d, ExactDev x, HubSplit sp) {
    GALA_CHUNK_PROLOGUE(G);
    const GatLane<G, VEC, CH, false> gl_(p, d, gl, own_col(x, row));
    ExBwdState<VEC, CH> st;
    exact_bwd_range<G, VEC, U, CH, HW>(p, d, x, gl_, e0, e1, st);
    float *w = sp.ws + c * sp.ws_cols;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (gl_.ln.in(ch, i)) {
                w[gl_.ln.off[ch] + i] = st.dx[ch][i];
                w[d.F + gl_.ln.off[ch] + i] = st.dxm[ch][i];
            }
    if (gl_.leader) w[2 * d.F + gl_.hh] = st.sg;
}

// hub rows, backward: the chunk partials added in ascending chunk order (alpha <= 1: no max)
template <int G, int VEC, int CH, int HW>
__global__ __launch_bounds__(kBlock) void k_gat_exact_bwd_fixup(EdgeParams p, GatDev d, ExactDev x, HubSplit sp) {
    const int lane = threadIdx.x & (kWave - 1);
    const int gl = lane & (G - 1);
    const int64_t ri = ((int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * (kWave / G) + lane / G;
    if (ri >= sp.n_rows_split) return;
    const int64_t row = sp.rows[ri];
    const int64_t s = own_col(x, row);
    const GatLane<G, VEC, CH, false> gl_(p, d, gl, s);
    const int F = d.F;
    ExBwdState<VEC, CH> st;
    for (int64_t cc = sp.row_chunk0[ri]; cc < sp.row_chunk0[ri + 1]; ++cc) {
        const float *w = sp.ws + cc * sp.ws_cols;
        st.sg = __fadd_rn(st.sg, w[2 * F + gl_.hh]);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const bool in = gl_.ln.in(ch, i);
                st.dx[ch][i] = __fadd_rn(st.dx[ch][i], in ? w[gl_.ln.off[ch] + i] : 0.0f);
                st.dxm[ch][i] = __fadd_rn(st.dxm[ch][i], in ? w[F + gl_.ln.off[ch] + i] : 0.0f);
            }
    }
    exact_bwd_store<G, VEC, CH, HW>(d, x, gl_, row, s, st);
}

}  // namespace gala

using namespace gala;

namespace {

struct ExactArgs {
    EdgeParams p;
    GatDev d;
    ExactDev x;
    HubSplit sp;
    bool split, bwd;
    bool pre = true, gather = true;  // the backward's two passes (the _ex calls run one each)
    hipStream_t hs;
};

template <int G, int VEC, int HW, int CH, bool RC>
void launch_exact(const ExactArgs &a) {
    constexpr int U = 8;
    // several vectors per lane only below float4 (narrow_chunks), and the backward never recomputes
    static_assert(CH == 1 || VEC < 4, "CH > 1 with float4 vectors is never dispatched");
    const dim3 rows(blocks_for(a.p.n_rows, G)), blk(kBlock);
    const int32_t thr = a.split ? a.sp.threshold : 0;
    if (!a.bwd) {
        hipLaunchKernelGGL((k_gat_exact_fwd<G, VEC, U, CH, RC, HW>), rows, blk, 0, a.hs, a.p, a.d, a.x, thr);
        if (!a.split) return;
        hipLaunchKernelGGL((k_gat_exact_fwd_chunk<G, VEC, U, CH, RC, HW>), dim3(blocks_for_groups(a.sp.n_chunks, G)),
                           blk, 0, a.hs, a.p, a.d, a.sp);
        hipLaunchKernelGGL((k_gat_exact_fwd_fixup<G, VEC, CH, RC>), dim3(blocks_for_groups(a.sp.n_rows_split, G)),
                           blk, 0, a.hs, a.p, a.d, a.x, a.sp);
        return;
    }
    if constexpr (!RC) {
        // the pre-pass reads the rows' aL (d.aL); the gather the rows' aR in its place
        ExactArgs g = a;
        g.d.aL = a.d.aR;
        if (a.pre) hipLaunchKernelGGL((k_gat_exact_bwd_pre<G, VEC, CH, HW>), rows, blk, 0, a.hs, a.p, a.d, a.x);
        if (!a.gather) return;
        hipLaunchKernelGGL((k_gat_exact_bwd<G, VEC, U, CH, HW>), rows, blk, 0, a.hs, g.p, g.d, g.x, thr);
        if (!a.split) return;
        hipLaunchKernelGGL((k_gat_exact_bwd_chunk<G, VEC, U, CH, HW>), dim3(blocks_for_groups(a.sp.n_chunks, G)), blk,
                           0, a.hs, g.p, g.d, g.x, g.sp);
        hipLaunchKernelGGL((k_gat_exact_bwd_fixup<G, VEC, CH, HW>), dim3(blocks_for_groups(a.sp.n_rows_split, G)),
                           blk, 0, a.hs, g.p, g.d, g.x, g.sp);
    }
}

template <int G, int VEC, bool RC>
int exact_g(const ExactArgs &a, int heads, int hw) {
    if (heads == 1) {
        launch_exact<G, VEC, G, 1, RC>(a);
        return GALA_OK;
    }
    if constexpr (G >= 2) {
        switch (hw) {
            case 1: launch_exact<G, VEC, 1, 1, RC>(a); return GALA_OK;
            case 2: if constexpr (G > 2) { launch_exact<G, VEC, 2, 1, RC>(a); return GALA_OK; } break;
            case 4: if constexpr (G > 4) { launch_exact<G, VEC, 4, 1, RC>(a); return GALA_OK; } break;
            case 8: if constexpr (G > 8) { launch_exact<G, VEC, 8, 1, RC>(a); return GALA_OK; } break;
            case 16: if constexpr (G > 16) { launch_exact<G, VEC, 16, 1, RC>(a); return GALA_OK; } break;
            case 32: if constexpr (G > 32) { launch_exact<G, VEC, 32, 1, RC>(a); return GALA_OK; } break;
            default: break;
        }
    }
    return GALA_ERR_UNSUPPORTED;
}

template <int VEC, bool RC>
int exact_vec(const ExactArgs &a, int L, int ch, int heads, int hw) {
    if (ch > 1) {
        if constexpr (VEC < 4) {
            if (ch == 2) launch_exact<16, VEC, 16, 2, RC>(a);
            else if (ch == 3) launch_exact<16, VEC, 16, 3, RC>(a);
            else if (ch == 4) launch_exact<16, VEC, 16, 4, RC>(a);
            else return GALA_ERR_UNSUPPORTED;
            return GALA_OK;
        }
        return GALA_ERR_UNSUPPORTED;
    }
    if (L <= 1) launch_exact<1, VEC, 1, 1, RC>(a);
    else if (L <= 2) return exact_g<2, VEC, RC>(a, heads, hw);
    else if (L <= 4) return exact_g<4, VEC, RC>(a, heads, hw);
    else if (L <= 8) return exact_g<8, VEC, RC>(a, heads, hw);
    else if (L <= 16) return exact_g<16, VEC, RC>(a, heads, hw);
    else if (L <= 32) return exact_g<32, VEC, RC>(a, heads, hw);
    else if (L <= 64) return exact_g<64, VEC, RC>(a, heads, hw);
    else return GALA_ERR_UNSUPPORTED;
    return GALA_OK;
}

// a graph with hub rows brings the workspace their chunk partials need
bool plan_ws_short(const gala_csr_t *A, int64_t ws_need) {
    const gala_split_plan_t *plan = A->split;
    return ws_need > 0 && plan && plan->n_chunks > 0 && plan->n_rows_split > 0 && A->n_seg == 1 &&
           (!plan->workspace || plan->ws_cols < ws_need);
}

// The shape checks and the launch: nothing is launched unless every check passed.
int exact_dispatch(const gala_csr_t *A, ExactArgs &a, int F, int heads, int vec, bool rc, int64_t ws_need) {
    const int D = F / heads;
    const int L = (F + vec - 1) / vec;
    const int ch = narrow_chunks(heads, vec, L);
    const int hw = (D % vec == 0) ? D / vec : 0;
    if (L > 64) return GALA_ERR_UNSUPPORTED;
    if (heads > 1 && (hw == 0 || (hw & (hw - 1)))) return GALA_ERR_UNSUPPORTED;
    if (plan_ws_short(A, ws_need)) return GALA_ERR_INVALID_ARG;
    a.split = ws_need > 0 && hub_split(A, ws_need, &a.sp);
    int r;
    if (rc && a.bwd) return GALA_ERR_INVALID_ARG;  // the backward reads aR: it has no recompute
    if (vec == 4) r = rc ? exact_vec<4, true>(a, L, ch, heads, hw) : exact_vec<4, false>(a, L, ch, heads, hw);
    else if (vec == 2) r = rc ? exact_vec<2, true>(a, L, ch, heads, hw) : exact_vec<2, false>(a, L, ch, heads, hw);
    else r = rc ? exact_vec<1, true>(a, L, ch, heads, hw) : exact_vec<1, false>(a, L, ch, heads, hw);
    if (r) return r;
    return launch_status();
}

inline bool aligned_to(const void *ptr, int v) { return ((uintptr_t)ptr % (4 * v)) == 0; }

}  // namespace

// self_col NULL needs a square pattern (a row is then its own column); with it the columns
// index gathered tables of n_cols >= n_rows rows
static int exact_pattern_ok(const gala_csr_t *A, const int32_t *self_col) {
    if (A->n_rows > A->n_cols) return GALA_ERR_INVALID_ARG;
    if (!self_col && A->n_cols != A->n_rows) return GALA_ERR_INVALID_ARG;
    return GALA_OK;
}

extern "C" int gala_gat_fwd_stats_exact_ex_f32(const gala_csr_t *A, const float *aL, const float *aR, const float *wR,
                                               const float *bR, const float *X, int64_t ldx, int32_t F, int32_t heads,
                                               float slope, float *Y, int64_t ldy, float *lse, float *Ym,
                                               int64_t ldym, float *sma, const int32_t *self_col, float *aR_out,
                                               void *stream) {
    ExactArgs a{};
    int st = edge_setup(A, heads, &a.p);
    if (st) return st;
    if (F < 1 || F % heads != 0 || ldx < F || ldy < F || ldym < F) return GALA_ERR_INVALID_ARG;
    if (A->n_rows == 0) return GALA_OK;
    if ((st = exact_pattern_ok(A, self_col))) return st;
    if (!aL || (!aR && !wR) || !Y || !lse || !Ym || !sma || !X) return GALA_ERR_INVALID_ARG;
    if (aR_out && aR) return GALA_ERR_INVALID_ARG;
    const int D = F / heads;
    auto ok = [&](int v) {
        const bool fits = D % v == 0 || (heads == 1 && ldx >= pad_to(F, v) && ldy >= pad_to(F, v) && ldym >= pad_to(F, v));
        return fits && ldx % v == 0 && ldy % v == 0 && ldym % v == 0 && aligned_to(X, v) && aligned_to(Y, v) &&
               aligned_to(Ym, v);
    };
    int vec = 4;
    while (vec > 1 && !ok(vec)) vec >>= 1;
    const bool rc = aR == nullptr;
    a.d.aL = aL, a.d.aR = aR, a.d.wR = rc ? wR : nullptr, a.d.bR = rc ? bR : nullptr;
    a.d.X = X, a.d.ldx = ldx, a.d.F = F, a.d.slope = slope;
    a.d.Y = Y, a.d.ldy = ldy, a.d.ym_out = Ym, a.d.ldym = ldym, a.d.sma_out = sma, a.d.ar_out = aR_out;
    a.x.lse_out = lse, a.x.self_col = self_col;
    a.hs = (hipStream_t)stream;
    a.bwd = false;
    return exact_dispatch(A, a, F, heads, vec, rc, 2 * (int64_t)F + 3 * heads);
}

extern "C" int gala_gat_fwd_stats_exact_f32(const gala_csr_t *A, const float *aL, const float *aR, const float *wR,
                                            const float *bR, const float *X, int64_t ldx, int32_t F, int32_t heads,
                                            float slope, float *Y, int64_t ldy, float *lse, float *Ym, int64_t ldym,
                                            float *sma, float *aR_out, void *stream) {
    return gala_gat_fwd_stats_exact_ex_f32(A, aL, aR, wR, bR, X, ldx, F, heads, slope, Y, ldy, lse, Ym, ldym, sma,
                                           nullptr, aR_out, stream);
}

namespace {

// The backward's operands; pre / gather: the passes to run.  One vector width serves every
// operand a pass reads (dY_rows and the dY table too: the own block of a table whose rows are
// no multiple of 16 bytes may start off the table's alignment).
struct ExactBwd {
    const float *aL, *aR, *X, *dY, *dY_rows, *lse, *Y, *Ym, *sma;
    int64_t ldx, lddy, ldy, ldym, lddx;
    const int32_t *self_col;
    float *side, *dX, *d_aL, *d_aR;
};

// AT (NULL: A itself) is the pattern the gather pass walks, A's transpose: row c of AT lists
// the rows r with an edge (r, c) of A.  The pre-pass is row-local and takes of A its n_rows.
int exact_backward(const gala_csr_t *A, const gala_csr_t *AT, const ExactBwd &b, int32_t F, int32_t heads,
                   float slope, bool pre, bool gather, void *stream) {
    ExactArgs a{};
    int st = edge_setup(A, heads, &a.p);
    if (st) return st;
    EdgeParams pt{};
    if (AT) {
        if ((st = edge_setup(AT, heads, &pt))) return st;
        if (A->n_seg != 1 || AT->n_seg != 1) return GALA_ERR_INVALID_ARG;
        if (A->n_cols != A->n_rows || AT->n_cols != AT->n_rows || AT->n_rows != A->n_rows || AT->nnz != A->nnz)
            return GALA_ERR_INVALID_ARG;
    }
    if (F < 1 || F % heads != 0 || b.lddy < F) return GALA_ERR_INVALID_ARG;
    if (pre && (b.ldy < F || b.ldym < F)) return GALA_ERR_INVALID_ARG;
    if (gather && (b.ldx < F || b.lddx < F)) return GALA_ERR_INVALID_ARG;
    if (A->n_rows == 0) return GALA_OK;
    if ((st = exact_pattern_ok(A, b.self_col))) return st;
    if (!b.side || ((uintptr_t)b.side % 16) != 0) return GALA_ERR_INVALID_ARG;
    if (pre && (!b.aL || !b.dY_rows || !b.lse || !b.Y || !b.Ym || !b.sma || !b.d_aL)) return GALA_ERR_INVALID_ARG;
    if (gather && (!b.aR || !b.X || !b.dY || !b.dX || !b.d_aR)) return GALA_ERR_INVALID_ARG;
    const int D = F / heads;
    auto ok = [&](int v) {
        bool padded = heads == 1 && b.lddy >= pad_to(F, v);
        bool mult = b.lddy % v == 0;
        if (pre) {
            padded = padded && b.ldy >= pad_to(F, v) && b.ldym >= pad_to(F, v);
            mult = mult && b.ldy % v == 0 && b.ldym % v == 0 && aligned_to(b.dY_rows, v) && aligned_to(b.Y, v) &&
                   aligned_to(b.Ym, v);
        }
        if (gather) {
            padded = padded && b.ldx >= pad_to(F, v) && b.lddx >= pad_to(F, v);
            mult = mult && b.ldx % v == 0 && b.lddx % v == 0 && aligned_to(b.X, v) && aligned_to(b.dY, v) &&
                   aligned_to(b.dX, v);
        }
        return (D % v == 0 || padded) && mult;
    };
    int vec = 4;
    while (vec > 1 && !ok(vec)) vec >>= 1;
    a.d.aL = b.aL, a.d.aR = b.aR, a.d.X = b.X, a.d.ldx = b.ldx, a.d.F = F, a.d.slope = slope;
    a.d.dY = b.dY, a.d.dy_rows = b.dY_rows, a.d.lddy = b.lddy, a.d.ys = b.Y, a.d.ldy = b.ldy, a.d.yms = b.Ym;
    a.d.ldym = b.ldym, a.d.smas = b.sma;
    a.d.dX = b.dX, a.d.lddx = b.lddx, a.d.d_aL = b.d_aL;
    a.x.lse = b.lse, a.x.side = b.side, a.x.d_aR = b.d_aR, a.x.self_col = b.self_col;
    a.hs = (hipStream_t)stream;
    a.bwd = true, a.pre = pre, a.gather = gather;
    // the pre-pass is row-local: no hub chunks, no workspace
    const int64_t ws_need = gather ? 2 * (int64_t)F + heads : 0;
    if (!AT) return exact_dispatch(A, a, F, heads, vec, false, ws_need);
    // the two passes apart, each over its own pattern, with the one vector width; AT's plan is
    // looked at before the pre-pass goes out, so a short workspace launches nothing.  "Nothing is
    // launched unless every check passed" rests on the two dispatches below sharing F, heads and
    // vec: the shape checks of exact_dispatch then give the same answer for both, and the one
    // check that reads the pattern (the plan's workspace) is this line.  A check added to
    // exact_dispatch that can differ between A and AT must be made here too, before the pre-pass
    if (plan_ws_short(AT, ws_need)) return GALA_ERR_INVALID_ARG;
    ExactArgs g = a;
    g.p = pt, g.pre = false;
    a.gather = false;
    if ((st = exact_dispatch(A, a, F, heads, vec, false, 0))) return st;
    return exact_dispatch(AT, g, F, heads, vec, false, ws_need);
}

}  // namespace

extern "C" int gala_gat_bwd_stats_exact_f32(const gala_csr_t *A, const float *aL, const float *aR, const float *X,
                                            int64_t ldx, const float *dY, int64_t lddy, int32_t F, int32_t heads,
                                            float slope, const float *lse, const float *Y, int64_t ldy,
                                            const float *Ym, int64_t ldym, const float *sma, float *side, float *dX,
                                            int64_t lddx, float *d_aL, float *d_aR, void *stream) {
    ExactBwd b{};
    b.aL = aL, b.aR = aR, b.X = X, b.dY = dY, b.dY_rows = dY, b.lse = lse, b.Y = Y, b.Ym = Ym, b.sma = sma;
    b.ldx = ldx, b.lddy = lddy, b.ldy = ldy, b.ldym = ldym, b.lddx = lddx;
    b.side = side, b.dX = dX, b.d_aL = d_aL, b.d_aR = d_aR;
    return exact_backward(A, nullptr, b, F, heads, slope, true, true, stream);
}

extern "C" int gala_gat_bwd_stats_exact_t_f32(const gala_csr_t *A, const gala_csr_t *AT, const float *aL,
                                              const float *aR, const float *X, int64_t ldx, const float *dY,
                                              int64_t lddy, int32_t F, int32_t heads, float slope, const float *lse,
                                              const float *Y, int64_t ldy, const float *Ym, int64_t ldym,
                                              const float *sma, float *side, float *dX, int64_t lddx, float *d_aL,
                                              float *d_aR, void *stream) {
    if (!AT) return GALA_ERR_INVALID_ARG;
    ExactBwd b{};
    b.aL = aL, b.aR = aR, b.X = X, b.dY = dY, b.dY_rows = dY, b.lse = lse, b.Y = Y, b.Ym = Ym, b.sma = sma;
    b.ldx = ldx, b.lddy = lddy, b.ldy = ldy, b.ldym = ldym, b.lddx = lddx;
    b.side = side, b.dX = dX, b.d_aL = d_aL, b.d_aR = d_aR;
    return exact_backward(A, AT, b, F, heads, slope, true, true, stream);
}

extern "C" int gala_gat_bwd_exact_pre_ex_f32(const gala_csr_t *A, const float *aL, const float *dY_rows, int64_t lddy,
                                             int32_t F, int32_t heads, const float *lse, const float *Y, int64_t ldy,
                                             const float *Ym, int64_t ldym, const float *sma, const int32_t *self_col,
                                             float *side, float *d_aL, void *stream) {
    ExactBwd b{};
    b.aL = aL, b.dY_rows = dY_rows, b.lse = lse, b.Y = Y, b.Ym = Ym, b.sma = sma;
    b.lddy = lddy, b.ldy = ldy, b.ldym = ldym, b.self_col = self_col, b.side = side, b.d_aL = d_aL;
    return exact_backward(A, nullptr, b, F, heads, 0.0f, true, false, stream);
}

extern "C" int gala_gat_bwd_exact_gather_ex_f32(const gala_csr_t *A, const float *aR, const float *X, int64_t ldx,
                                                const float *dY, int64_t lddy, int32_t F, int32_t heads, float slope,
                                                const float *side, const int32_t *self_col, float *dX, int64_t lddx,
                                                float *d_aR, void *stream) {
    ExactBwd b{};
    b.aR = aR, b.X = X, b.dY = dY, b.ldx = ldx, b.lddy = lddy, b.lddx = lddx, b.self_col = self_col;
    b.side = const_cast<float *>(side), b.dX = dX, b.d_aR = d_aR;
    return exact_backward(A, nullptr, b, F, heads, slope, false, true, stream);
}
