// C++/libtorch mirror of GALA's emitted operator API over the C ABI (see gala_torch.h).
#include "gala_torch.h"
#include <climits>
#include <cstring>

#include "gala_cpu.h"


#include <c10/hip/HIPStream.h>

namespace gala {

namespace {

void *stream() { return (void *)c10::hip::getCurrentHIPStream().stream(); }

// The operator set of one device: libgala_hip.so (include/gala_hip.h) for GPU tensors,
// libgala_cpu.so (include/gala_cpu.h) for tensors a program placed on the host
// (--device cpu).  The graph's device selects the table; every other operand must be on
// that device (check_on), so nothing moves between devices behind the caller's back and a
// GPU call never runs on the CPU.
struct Backend {
    decltype(&gala_spmm_ex_f32) spmm;
    decltype(&gala_degree_f32) degree;
    decltype(&gala_row_broadcast_f32) row_broadcast;
    decltype(&gala_row_scale_relu_f32) scale_relu;
    decltype(&gala_relu_scale_backward_f32) relu_bwd;
    decltype(&gala_ffn_fwd_f32) ffn_fwd;
    decltype(&gala_sddvv_f32) sddvv;
    decltype(&gala_row_sum_f32) row_sum;
    decltype(&gala_row_scale_f32) row_scale;
    decltype(&gala_sddmm_dot_f32) sddmm;
    decltype(&gala_edge_softmax_fwd_f32) softmax_fwd;
    decltype(&gala_edge_softmax_bwd_f32) softmax_bwd;
    decltype(&gala_gat_fwd_f32) gat_fwd;
    decltype(&gala_gat_bwd_f32) gat_bwd;
    decltype(&gala_gat_fwd_attn_f32) gat_fwd_attn;
    decltype(&gala_gat_bwd_attn_f32) gat_bwd_attn;
    decltype(&gala_gat_fwd_ex_f32) gat_fwd_ex;
    decltype(&gala_gat_bwd_ex_f32) gat_bwd_ex;
    decltype(&gala_gat_bwd_fused_f32) gat_bwd_fused;
    decltype(&gala_gat_fwd_stats_f32) gat_fwd_stats;
    decltype(&gala_gat_bwd_stats_f32) gat_bwd_stats;
    decltype(&gala_gat_bwd_stats_linear_f32) gat_bwd_stats_linear;
    decltype(&gala_gat_fwd_stats_exact_f32) gat_fwd_stats_exact;
    decltype(&gala_gat_bwd_stats_exact_f32) gat_bwd_stats_exact;
    decltype(&gala_gat_bwd_stats_exact_t_f32) gat_bwd_stats_exact_t;
    decltype(&gala_csr_is_transpose_i32) csr_is_transpose;
    decltype(&gala_head_attn_f32) head_attn;
    decltype(&gala_head_attn_bwd_f32) head_attn_bwd;
    decltype(&gala_edge_permute_f32) permute;
    decltype(&gala_dense_grad_workspace) dense_ws;
    decltype(&gala_dense_grad_f32) dense_grad;
    decltype(&gala_gat_in_prep_f32) gat_in_prep;
    decltype(&gala_gat_in_fwd_f32) gat_in_fwd;
    decltype(&gala_gat_in_bwd_workspace) gat_in_ws;
    decltype(&gala_gat_in_bwd_f32) gat_in_bwd;
    decltype(&gala_gat_in_fwd_t_f32) gat_in_fwd_t;   // T mode: GPU only (null on the host backend)
    decltype(&gala_gat_in_bwd_t_f32) gat_in_bwd_t;
};
const Backend kHip{gala_spmm_ex_f32, gala_degree_f32, gala_row_broadcast_f32,
                   gala_row_scale_relu_f32, gala_relu_scale_backward_f32, gala_ffn_fwd_f32,
                   gala_sddvv_f32,
                   gala_row_sum_f32, gala_row_scale_f32, gala_sddmm_dot_f32,
                   gala_edge_softmax_fwd_f32, gala_edge_softmax_bwd_f32, gala_gat_fwd_f32,
                   gala_gat_bwd_f32, gala_gat_fwd_attn_f32, gala_gat_bwd_attn_f32,
                   gala_gat_fwd_ex_f32, gala_gat_bwd_ex_f32, gala_gat_bwd_fused_f32,
                   gala_gat_fwd_stats_f32, gala_gat_bwd_stats_f32, gala_gat_bwd_stats_linear_f32,
                   gala_gat_fwd_stats_exact_f32, gala_gat_bwd_stats_exact_f32,
                   gala_gat_bwd_stats_exact_t_f32, gala_csr_is_transpose_i32,
                   gala_head_attn_f32, gala_head_attn_bwd_f32,
                   gala_edge_permute_f32, gala_dense_grad_workspace, gala_dense_grad_f32,
                   gala_gat_in_prep_f32, gala_gat_in_fwd_f32, gala_gat_in_bwd_workspace, gala_gat_in_bwd_f32,
                   gala_gat_in_fwd_t_f32, gala_gat_in_bwd_t_f32};
const Backend kCpu{gala_cpu_spmm_ex_f32, gala_cpu_degree_f32, gala_cpu_row_broadcast_f32,
                   gala_cpu_row_scale_relu_f32, gala_cpu_relu_scale_backward_f32, gala_cpu_ffn_fwd_f32,
                   gala_cpu_sddvv_f32, gala_cpu_row_sum_f32, gala_cpu_row_scale_f32,
                   gala_cpu_sddmm_dot_f32, gala_cpu_edge_softmax_fwd_f32,
                   gala_cpu_edge_softmax_bwd_f32, gala_cpu_gat_fwd_f32, gala_cpu_gat_bwd_f32,
                   gala_cpu_gat_fwd_attn_f32, gala_cpu_gat_bwd_attn_f32,
                   gala_cpu_gat_fwd_ex_f32, gala_cpu_gat_bwd_ex_f32, gala_cpu_gat_bwd_fused_f32,
                   gala_cpu_gat_fwd_stats_f32, gala_cpu_gat_bwd_stats_f32, gala_cpu_gat_bwd_stats_linear_f32,
                   gala_cpu_gat_fwd_stats_exact_f32, gala_cpu_gat_bwd_stats_exact_f32,
                   gala_cpu_gat_bwd_stats_exact_t_f32, gala_cpu_csr_is_transpose_i32,
                   gala_cpu_head_attn_f32, gala_cpu_head_attn_bwd_f32,
                   gala_cpu_edge_permute_f32, gala_cpu_dense_grad_workspace,
                   gala_cpu_dense_grad_f32, gala_cpu_gat_in_prep_f32, gala_cpu_gat_in_fwd_f32,
                   gala_cpu_gat_in_bwd_workspace, gala_cpu_gat_in_bwd_f32, nullptr, nullptr};

const Backend &be(const torch::Tensor &t) {
    TORCH_CHECK(t.is_cuda() || t.is_cpu(), "gala: unsupported device ", t.device());
    return t.is_cuda() ? kHip : kCpu;
}
void *stream_of(const torch::Tensor &t) { return t.is_cuda() ? stream() : nullptr; }

void check(int status, const char *fn) {
    TORCH_CHECK(status == GALA_OK, "gala: ", fn, " failed: ", gala_status_string(status),
                status == GALA_ERR_HIP ? " (hipError " + std::to_string(gala_last_hip_error()) + ")"
                                       : std::string());
}

// a row-padded [N, F] view (see pad_rows4 below): row stride F rounded up to 4 floats
bool row_padded(const torch::Tensor &x) {
    return x.dim() == 2 && x.size(0) > 0 && x.stride(1) == 1 && x.size(1) % 4 != 0 &&
           x.stride(0) == (x.size(1) + 3) / 4 * 4;
}

void check_dev(const torch::Tensor &t, torch::ScalarType ty, const char *name) {
    TORCH_CHECK(t.defined(), "gala: ", name, " is undefined");
    TORCH_CHECK(t.is_cuda() || t.is_cpu(), "gala: ", name, " is on unsupported device ", t.device());
    TORCH_CHECK(t.scalar_type() == ty, "gala: ", name, " has dtype ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous() || row_padded(t), "gala: ", name, " must be contiguous");
}

// operand `t` must live on the graph's device (no implicit copies, no CPU fallback)
void check_on(const torch::Tensor &t, const torch::Tensor &graph, const char *name) {
    TORCH_CHECK(t.device() == graph.device(), "gala: ", name, " is on ", t.device(),
                " but the graph is on ", graph.device());
}

// A gala_csr_t view of the generated program's (offset, columns, value, bounds) tensors.
struct CsrView {
    gala_csr_t c{};
    torch::Tensor bounds_host;  // keeps the host bounds alive
};

// the split plan registered for this offsets tensor (same TensorImpl as a slot's, or as a
// slot's merged rowptr)
SplitState *find_split(const torch::Tensor &offsets) {
    auto &S = global_slots();
    for (size_t i = 0; i < S.offset_graph.size(); ++i) {
        if (S.split[i] && S.offset_graph[i].unsafeGetTensorImpl() == offsets.unsafeGetTensorImpl())
            return S.split[i].get();
        if (S.merged[i] && S.merged[i]->split &&
            S.merged[i]->rowptr.unsafeGetTensorImpl() == offsets.unsafeGetTensorImpl())
            return S.merged[i]->split.get();
    }
    return nullptr;
}

// the merged rows registered for this tiled offsets tensor
const MergedCsr *find_merged(const torch::Tensor &offsets) {
    auto &S = global_slots();
    for (size_t i = 0; i < S.offset_graph.size(); ++i)
        if (S.merged[i] && S.offset_graph[i].unsafeGetTensorImpl() == offsets.unsafeGetTensorImpl())
            return S.merged[i].get();
    return nullptr;
}

// a graph view whose hub-row plan carries a workspace of at least `cols` floats per chunk
void with_workspace(CsrView &cv, const torch::Tensor &offsets, int64_t cols) {
    if (!cv.c.split) return;
    SplitState *sp = find_split(offsets);
    sp->ensure_workspace(cols);
    cv.c.split = &sp->plan;
}

CsrView view(const torch::Tensor &offsets, const torch::Tensor &cols, const torch::Tensor *vals,
             const torch::Tensor &bounds, int64_t segments, int val_heads = 1) {
    check_dev(offsets, torch::kInt, "offset_graph");
    check_dev(cols, torch::kInt, "columns_graph");
    TORCH_CHECK(segments >= 1, "gala: segments must be >= 1");
    TORCH_CHECK(offsets.numel() % segments == 0, "gala: offset_graph size is not (nrows+1)*segments");
    CsrView v;
    v.c.n_rows = offsets.numel() / segments - 1;
    v.c.n_cols = v.c.n_rows;
    v.c.nnz = cols.numel();
    v.c.rowptr = offsets.data_ptr<int32_t>();
    v.c.col = cols.data_ptr<int32_t>();
    v.c.val = nullptr;
    v.c.val_heads = val_heads;
    if (vals) {
        check_dev(*vals, torch::kFloat, "value_graph");
        v.c.val = vals->data_ptr<float>();
    }
    v.c.n_seg = (int32_t)segments;
    v.c.seg_bounds = nullptr;
    v.c.split = nullptr;
    if (segments == 1) {
        if (SplitState *sp = find_split(offsets)) v.c.split = &sp->plan;
    }
    if (segments > 1) {
        TORCH_CHECK(bounds.defined() && bounds.numel() >= 2 * segments, "gala: bounds missing");
        v.bounds_host = bounds.to(torch::kCPU, torch::kInt).contiguous();
        v.c.seg_bounds = v.bounds_host.data_ptr<int32_t>();
    }
    return v;
}

torch::TensorOptions fopts(const torch::Tensor &like) {
    return torch::TensorOptions().dtype(torch::kFloat).device(like.device());
}

// Row-padded feature matrices: an [N, F] view of storage whose row stride is F rounded up
// to 4 floats.  With F % 4 != 0 (F = 47, the Products class count) the kernels then move
// whole float4 vectors and a gathered row spans 2 cache lines instead of 2.4 on average;
// the padding columns are read, zeroed before any dot product, and never written.

// (row_padded() is defined above check_dev)
// x itself when contiguous or row-padded, else a row-padded copy (GPU, one head only:
// callers pass heads == 1) -- or a contiguous one on the CPU backend
torch::Tensor pad_rows4(const torch::Tensor &x) {
    if (row_padded(x)) return x;
    if (!x.is_cuda() || x.dim() != 2 || x.size(1) % 4 == 0 || x.size(0) == 0) return x.contiguous();
    const int64_t F = x.size(1);
    auto v = torch::empty({x.size(0), (F + 3) / 4 * 4}, fopts(x)).narrow(1, 0, F);
    v.copy_(x);
    return v;
}

// an [nrows, F] output with x's row padding
torch::Tensor rows_like(const torch::Tensor &x, int64_t nrows) {
    if (row_padded(x)) return torch::empty({nrows, x.stride(0)}, fopts(x)).narrow(1, 0, x.size(1));
    return torch::empty({nrows, x.size(1)}, fopts(x));
}

torch::Tensor row_sum_impl(const torch::Tensor &offsets, const torch::Tensor &cols,
                           const torch::Tensor &v, const torch::Tensor &bounds, int64_t nrows,
                           int64_t segments, float eps) {
    auto vv = v.contiguous();
    CsrView cv = view(offsets, cols, nullptr, bounds, segments);
    TORCH_CHECK(cv.c.n_rows == nrows, "gala: nrows does not match offset_graph");
    check_dev(vv, torch::kFloat, "value_graph");
    const int heads = (int)(vv.numel() / std::max<int64_t>(cols.numel(), 1));
    with_workspace(cv, offsets, 2 * std::max(heads, 1));  // hub-row partial sums
    auto out = torch::empty({nrows, std::max(heads, 1)}, fopts(v));
    check_on(vv, offsets, "value_graph");
    check(be(offsets).row_sum(&cv.c, vv.data_ptr<float>(), std::max(heads, 1), eps,
                              out.data_ptr<float>(), 0, stream_of(offsets)),
          "gala_row_sum_f32");
    return out;
}

torch::Tensor row_scale_impl(const torch::Tensor &row_val, const torch::Tensor &offsets,
                             const torch::Tensor &cols, torch::Tensor value_graph,
                             const torch::Tensor &bounds, int64_t nrows, int64_t segments) {
    CsrView cv = view(offsets, cols, nullptr, bounds, segments);
    TORCH_CHECK(cv.c.n_rows == nrows, "gala: nrows does not match offset_graph");
    auto q = row_val.contiguous();
    check_dev(q, torch::kFloat, "row_val");
    check_dev(value_graph, torch::kFloat, "value_graph");
    const int heads = (int)(q.numel() / std::max<int64_t>(nrows, 1));
    check_on(q, offsets, "row_val");
    check_on(value_graph, offsets, "value_graph");
    check(be(offsets).row_scale(&cv.c, q.data_ptr<float>(), std::max(heads, 1),
                                value_graph.data_ptr<float>(), stream_of(offsets)),
          "gala_row_scale_f32");
    return value_graph;
}

torch::Tensor sddvv_impl(const torch::Tensor &a, const torch::Tensor &b,
                         const torch::Tensor &offsets, const torch::Tensor &cols,
                         const torch::Tensor &bounds, int64_t segments, int op, float slope) {
    CsrView cv = view(offsets, cols, nullptr, bounds, segments);
    auto ac = a.contiguous(), bc = b.contiguous();
    check_dev(ac, torch::kFloat, "input_dense1");
    check_dev(bc, torch::kFloat, "input_dense2");
    const int64_t nrows = cv.c.n_rows;
    const int heads = (int)std::max<int64_t>(ac.numel() / std::max<int64_t>(nrows, 1), 1);
    cv.c.n_cols = bc.numel() / heads;
    auto out = heads == 1 ? torch::empty({cols.numel()}, fopts(a))
                          : torch::empty({cols.numel(), heads}, fopts(a));
    check_on(ac, offsets, "input_dense1");
    check_on(bc, offsets, "input_dense2");
    check(be(offsets).sddvv(&cv.c, ac.data_ptr<float>(), bc.data_ptr<float>(), heads, op, slope,
                            out.data_ptr<float>(), stream_of(offsets)),
          "gala_sddvv_f32");
    return out;
}

torch::Tensor spmm_impl(const torch::Tensor &X, const torch::Tensor &offsets,
                        const torch::Tensor &cols, const torch::Tensor *vals,
                        const torch::Tensor &bounds, int64_t segments, int val_heads,
                        const torch::Tensor *src_scale, const torch::Tensor *dst_scale,
                        int64_t nsamples, int64_t ra, int64_t rb,
                        const torch::Tensor *val_row_scale = nullptr,
                        const gala_spmm_epilogue_t *epi = nullptr) {
    if (!vals && nsamples == 0 && segments > 1 && offsets.is_cuda()) {
        if (const MergedCsr *m = find_merged(offsets))  // the same sums over one segment
            return spmm_impl(X, m->rowptr, m->col, nullptr, torch::Tensor(), 1, val_heads, src_scale, dst_scale, 0,
                             ra, rb, nullptr, epi);
    }
    CsrView cv = view(offsets, cols, vals, bounds, segments, val_heads);
    // the ReLU prologue / epilogue (gcn_aggregate_relu_apply) run on unweighted, unsampled
    // graphs without hub rows: otherwise an undefined result, and the caller runs the passes
    if (epi && (epi->src_relu || epi->relu_x) &&
        (vals || nsamples > 0 || (cv.c.split && cv.c.split->n_rows_split > 0)))
        return torch::Tensor();
    if (val_row_scale) {  // factored edge values (GAT p with its per-row q)
        check_dev(*val_row_scale, torch::kFloat, "val_row_scale");
        check_on(*val_row_scale, offsets, "val_row_scale");
        cv.c.val_row_scale = val_row_scale->data_ptr<float>();
    }
    const bool padded = row_padded(X);
    auto x = padded ? X : X.contiguous();
    check_dev(x, torch::kFloat, "input_dense");
    const int64_t nrows = cv.c.n_rows;
    // reference: dcols = input_dense.numel() / nrows (cuda.h:453-454)
    const int64_t dcols = x.dim() == 2 ? x.size(1) : x.numel() / std::max<int64_t>(nrows, 1);
    if (cv.c.split) {
        SplitState *sp = find_split(offsets);
        sp->ensure_workspace(std::min<int64_t>(dcols, 2048));
        cv.c.split = &sp->plan;
    }
    cv.c.n_cols = dcols ? x.numel() / dcols : 0;
    auto out = padded ? rows_like(x, nrows) : torch::empty({nrows, dcols}, fopts(X));
    const int64_t ldx = padded ? x.stride(0) : dcols, ldy = padded ? out.stride(0) : dcols;
    const float *ss = nullptr, *ds = nullptr;
    torch::Tensor ssc, dsc;
    if (src_scale) {
        ssc = src_scale->contiguous();
        check_dev(ssc, torch::kFloat, "src_scale");
        ss = ssc.data_ptr<float>();
    }
    if (dst_scale) {
        dsc = dst_scale->contiguous();
        check_dev(dsc, torch::kFloat, "dst_scale");
        ds = dsc.data_ptr<float>();
    }
    const int32_t flags = nsamples > 0 ? GALA_SPMM_SAMPLE : spmm_hub_flag();
    check_on(x, offsets, "input_dense");
    if (ss) check_on(ssc, offsets, "src_scale");
    if (ds) check_on(dsc, offsets, "dst_scale");
    check(be(offsets).spmm(&cv.c, x.data_ptr<float>(), ldx, out.data_ptr<float>(), ldy,
                           (int32_t)dcols, ss, ds, flags, (int32_t)nsamples, (int32_t)ra,
                           (int32_t)rb, epi, stream_of(offsets)),
          "gala_spmm_ex_f32");
    return out;
}

}  // namespace

// ---- split plans ----------------------------------------------------------------------
int32_t spmm_hub_flag() {
    static const int32_t f = [] {
        const char *v = std::getenv("GALA_SPMM_HUB");
        if (!v || !*v || std::string(v) == "exact") return 0;
        TORCH_CHECK(std::string(v) == "chunked", "GALA_SPMM_HUB: exact | chunked, got ", v);
        return (int32_t)GALA_SPMM_HUB_CHUNKED;
    }();
    return f;
}

void SplitState::ensure_workspace(int64_t F) {
    F = (F + 3) / 4 * 4;  // chunk rows hold whole float4 vectors (padded rows included)
    if (plan.ws_cols >= F) return;
    ws = torch::empty({std::max<int64_t>(plan.n_chunks, 1) * F},
                      torch::TensorOptions().dtype(torch::kFloat).device(rows.device()));
    plan.workspace = ws.data_ptr<float>();
    plan.ws_cols = F;
}

// Hub-row split plan and degree-ordered row schedule of a device graph (gala_split_plan_t),
// built once per graph on the host: hub rows (deg > max(1024, 8 x mean)) are split into
// chunks; a skewed graph (max deg > 4 x mean) also gets the descending-degree row order.
std::shared_ptr<SplitState> make_split_plan(const torch::Tensor &offsets, int segments) {
    if (segments != 1 || !offsets.defined() || offsets.numel() < 2) return nullptr;
    auto rp = offsets.to(torch::kCPU, torch::kInt).contiguous();
    const int64_t n = rp.numel() - 1;
    const int32_t *r = rp.data_ptr<int32_t>();
    const int64_t nnz = r[n];
    const double mean = (double)nnz / (double)std::max<int64_t>(n, 1);
    int64_t max_deg = 0;
    for (int64_t i = 0; i < n; ++i) max_deg = std::max<int64_t>(max_deg, r[i + 1] - r[i]);
    const int32_t thr = gala_host_split_threshold(n, nnz);
    const int32_t chunk = 512;
    const bool skewed = (double)max_deg > 4.0 * std::max(mean, 1.0);
    int64_t nr = 0, nc = 0;
    check(gala_host_split_plan(n, r, thr, chunk, nullptr, nullptr, nullptr, &nr, &nc),
          "gala_host_split_plan");
    if (nr == 0 && !skewed) return nullptr;
    auto io = torch::TensorOptions().dtype(torch::kInt);
    auto rows = torch::empty({std::max<int64_t>(nr, 1)}, io), rc0 = torch::zeros({nr + 1}, io),
         crow = torch::empty({std::max<int64_t>(nc, 1)}, io);
    if (nr > 0)
        check(gala_host_split_plan(n, r, thr, chunk, rows.data_ptr<int32_t>(), rc0.data_ptr<int32_t>(),
                                   crow.data_ptr<int32_t>(), &nr, &nc),
              "gala_host_split_plan");
    auto st = std::make_shared<SplitState>();
    st->rows = rows.to(offsets.device());
    st->row_chunk0 = rc0.to(offsets.device());
    st->chunk_row = crow.to(offsets.device());
    if (skewed) {
        auto order = torch::empty({n}, io);
        check(gala_host_row_order(n, r, order.data_ptr<int32_t>()), "gala_host_row_order");
        st->row_order = order.to(offsets.device());
    }
    if (nr > 0 && offsets.is_cuda()) {
        // the REF-order hub rows run on a side stream beside the row kernel: a high-priority
        // one, so the longest serial chains are dispatched before the row kernel fills the CUs
        auto aux = c10::hip::getStreamFromPool(true, offsets.device().index());
        st->plan.aux_stream = (void *)aux.stream();
        for (int i = 0; i < 2; ++i) {
            hipEvent_t ev = nullptr;
            TORCH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess, "hipEventCreate");
            st->aux_events[i] = st->plan.aux_events[i] = (void *)ev;
        }
    }
    st->plan.threshold = thr;
    st->plan.chunk = chunk;
    st->plan.n_rows_split = nr;
    st->plan.n_chunks = nc;
    st->plan.rows = st->rows.data_ptr<int32_t>();
    st->plan.row_chunk0 = st->row_chunk0.data_ptr<int32_t>();
    st->plan.chunk_row = st->chunk_row.data_ptr<int32_t>();
    st->plan.workspace = nullptr;
    st->plan.ws_cols = 0;
    st->plan.row_order = st->row_order.defined() ? st->row_order.data_ptr<int32_t>() : nullptr;
    return st;
}

std::shared_ptr<MergedCsr> make_merged_csr(const torch::Tensor &offsets, const torch::Tensor &cols,
                                           const torch::Tensor &bounds_host, int segments) {
    if (segments <= 1 || !offsets.defined() || !cols.defined() || !bounds_host.defined() ||
        offsets.scalar_type() != torch::kInt || cols.scalar_type() != torch::kInt ||
        offsets.numel() % segments != 0 || bounds_host.numel() < 2 * segments)
        return nullptr;
    auto rp = offsets.to(torch::kCPU).contiguous();
    auto cl = cols.to(torch::kCPU).contiguous();
    auto bd = bounds_host.to(torch::kCPU, torch::kInt).contiguous();
    const int64_t n = offsets.numel() / segments - 1, nnz = cl.numel();
    const int32_t *r = rp.data_ptr<int32_t>(), *c = cl.data_ptr<int32_t>(), *b = bd.data_ptr<int32_t>();
    // the kernels' own checks (fill_segments, the rowptr contract): anything else stays tiled
    int64_t total = 0;
    for (int s = 0; s < segments; ++s) {
        const int32_t *q = r + (int64_t)s * (n + 1);
        if (b[2 * s] < 0 || b[2 * s + 1] < b[2 * s] || b[2 * s + 1] > nnz || q[0] < 0 ||
            (int64_t)b[2 * s] + q[n] > nnz)
            return nullptr;
        for (int64_t i = 0; i < n; ++i)
            if (q[i + 1] < q[i]) return nullptr;
        total += q[n] - q[0];
    }
    if (total > INT32_MAX) return nullptr;
    auto io = torch::TensorOptions().dtype(torch::kInt);
    auto mrp = torch::empty({n + 1}, io), mcol = torch::empty({std::max<int64_t>(total, 1)}, io);
    int32_t *o = mrp.data_ptr<int32_t>(), *oc = mcol.data_ptr<int32_t>();
    int64_t k = 0;
    o[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        for (int s = 0; s < segments; ++s) {
            const int32_t *q = r + (int64_t)s * (n + 1);
            const int64_t e0 = (int64_t)b[2 * s] + q[i], e1 = (int64_t)b[2 * s] + q[i + 1];
            std::memcpy(oc + k, c + e0, (size_t)(e1 - e0) * sizeof(int32_t));
            k += e1 - e0;
        }
        o[i + 1] = (int32_t)k;
    }
    auto m = std::make_shared<MergedCsr>();
    m->rowptr = mrp.to(offsets.device());
    m->col = mcol.to(offsets.device());
    m->split = make_split_plan(m->rowptr, 1);
    return m;
}

// ---- slots ----------------------------------------------------------------------------
int GraphSlots::push(torch::Tensor offsets, torch::Tensor cols, torch::Tensor vals,
                     torch::Tensor b, int segs, bool w) {
    offset_graph.push_back(offsets);
    columns_graph.push_back(cols);
    value_graph.push_back(vals);
    bounds.push_back(b.defined() ? b.to(torch::kCPU, torch::kInt).contiguous() : b);
    segments.push_back(segs);
    weighted.push_back(w);
    transpose_perm.push_back(torch::Tensor());
    // a slot sharing the previous slot's tensors (undirected backward) shares its plan
    std::shared_ptr<SplitState> sp;
    if (!split.empty() && offset_graph.size() >= 2 &&
        offset_graph[offset_graph.size() - 2].unsafeGetTensorImpl() == offsets.unsafeGetTensorImpl())
        sp = split.back();
    else if (offsets.is_cuda())  // the CPU backend runs every row in one sequential pass
        sp = make_split_plan(offsets, segs);
    split.push_back(sp);
    std::shared_ptr<MergedCsr> mg;
    if (!merged.empty() && offset_graph.size() >= 2 &&
        offset_graph[offset_graph.size() - 2].unsafeGetTensorImpl() == offsets.unsafeGetTensorImpl())
        mg = merged.back();
    else if (offsets.is_cuda() && segs > 1 && !w)
        mg = make_merged_csr(offsets, cols, bounds.back(), segs);
    merged.push_back(mg);
    pattern_t.push_back(nullptr);
    holds_previous.push_back(-1);
    transposes_previous.push_back(-1);
    if (offset_graph.size() == 1) nrows = offsets.numel() / segs - 1;
    return (int)offset_graph.size() - 1;
}

void GraphSlots::clear() { *this = GraphSlots(); }

GraphSlots &global_slots() {
    // never destroyed: device tensors must not be freed from a static destructor, after
    // the HIP caching allocator may already be gone (process exit)
    static GraphSlots *s = new GraphSlots();
    return *s;
}

// ---- emitted free functions ---------------------------------------------------------------
torch::Tensor aggregate_node_mul_sum_call(torch::Tensor input_dense, torch::Tensor offset_graph,
                                          torch::Tensor columns_graph, torch::Tensor value_graph,
                                          torch::Tensor bounds, int64_t segments, bool weighted,
                                          int64_t nsamples, int64_t ra, int64_t rb) {
    return spmm_impl(input_dense, offset_graph, columns_graph, weighted ? &value_graph : nullptr,
                     bounds, segments, 1, nullptr, nullptr, nsamples, ra, rb);
}

torch::Tensor aggregate_node_mul_sum_direct_call(torch::Tensor input_dense,
                                                 torch::Tensor offset_graph,
                                                 torch::Tensor columns_graph,
                                                 torch::Tensor value_graph, torch::Tensor bounds,
                                                 int64_t segments, bool weighted) {
    return aggregate_node_mul_sum_call(input_dense, offset_graph, columns_graph, value_graph,
                                       bounds, segments, weighted);
}

torch::Tensor gather_forward(torch::Tensor input_dense, torch::Tensor offset_graph,
                             torch::Tensor columns_graph, torch::Tensor value_graph) {
    // cuSPARSE CSR_ALG2 path, alpha = beta = 1 onto a zero output (cuda.h:211-279)
    return aggregate_node_mul_sum_call(input_dense, offset_graph, columns_graph, value_graph, {},
                                       1, true);
}

torch::Tensor node_spmv_backward_of_sddmm_nln(torch::Tensor offset_graph,
                                              torch::Tensor columns_graph,
                                              torch::Tensor value_graph, torch::Tensor bounds,
                                              int64_t nrows, int64_t segments) {
    return row_sum_impl(offset_graph, columns_graph, value_graph, bounds, nrows, segments, 1e-12f);
}

torch::Tensor node_spmv_backward_of_sddmm_eaggr(torch::Tensor offset_graph,
                                                torch::Tensor columns_graph,
                                                torch::Tensor value_graph, torch::Tensor bounds,
                                                int64_t nrows, int64_t segments) {
    return row_sum_impl(offset_graph, columns_graph, value_graph, bounds, nrows, segments, 1e-12f);
}

torch::Tensor inplace_softmax_sddvv(torch::Tensor row_val, torch::Tensor offset_graph,
                                    torch::Tensor columns_graph, torch::Tensor value_graph,
                                    torch::Tensor bounds, int64_t nrows, int64_t segments) {
    return row_scale_impl(row_val, offset_graph, columns_graph, value_graph, bounds, nrows,
                          segments);
}

torch::Tensor inplace_softmax_sddvv_mult(torch::Tensor row_val, torch::Tensor offset_graph,
                                         torch::Tensor columns_graph, torch::Tensor value_graph,
                                         torch::Tensor bounds, int64_t nrows, int64_t segments) {
    return row_scale_impl(row_val, offset_graph, columns_graph, value_graph, bounds, nrows,
                          segments);
}

torch::Tensor edge_sddvv(torch::Tensor input_dense1, torch::Tensor input_dense2,
                         torch::Tensor offset_graph, torch::Tensor columns_graph,
                         torch::Tensor value_graph, torch::Tensor bounds, int64_t nrows,
                         int64_t segments) {
    (void)value_graph;
    (void)nrows;
    return sddvv_impl(input_dense1, input_dense2, offset_graph, columns_graph, bounds, segments,
                      GALA_SDDVV_ADD, 0.0f);
}

torch::Tensor edge_sddmm(torch::Tensor input_dense1, torch::Tensor input_dense2,
                         torch::Tensor offset_graph, torch::Tensor columns_graph,
                         torch::Tensor value_graph, torch::Tensor bounds, int64_t nrows,
                         int64_t segments) {
    (void)value_graph;
    CsrView cv = view(offset_graph, columns_graph, nullptr, bounds, segments);
    TORCH_CHECK(cv.c.n_rows == nrows, "gala: nrows does not match offset_graph");
    auto a = input_dense1.contiguous(), b = input_dense2.contiguous();
    check_dev(a, torch::kFloat, "input_dense1");
    check_dev(b, torch::kFloat, "input_dense2");
    const int64_t dcols = a.numel() / std::max<int64_t>(nrows, 1);  // cuda.h:813-814
    cv.c.n_cols = b.numel() / std::max<int64_t>(dcols, 1);
    auto out = torch::empty({columns_graph.numel()}, fopts(a));
    check_on(a, offset_graph, "input_dense1");
    check_on(b, offset_graph, "input_dense2");
    check(be(offset_graph).sddmm(&cv.c, a.data_ptr<float>(), dcols, b.data_ptr<float>(), dcols,
                                 (int32_t)dcols, 1, out.data_ptr<float>(), stream_of(offset_graph)),
          "gala_sddmm_dot_f32");
    return out;
}

torch::Tensor aggregate_edge_mul(torch::Tensor input_dense1, torch::Tensor input_dense2,
                                 torch::Tensor offset_graph, torch::Tensor columns_graph,
                                 torch::Tensor value_graph, torch::Tensor bounds,
                                 int64_t segments) {
    (void)value_graph;
    return sddvv_impl(input_dense1, input_dense2, offset_graph, columns_graph, bounds, segments,
                      GALA_SDDVV_MUL, 0.0f);
}

torch::Tensor aggregate_edge_mul_dir(torch::Tensor input_dense1, torch::Tensor input_dense2,
                                     torch::Tensor offset_graph, torch::Tensor columns_graph,
                                     torch::Tensor value_graph) {
    return aggregate_edge_mul(input_dense1, input_dense2, offset_graph, columns_graph,
                              value_graph, {}, 1);
}

torch::Tensor row_broadcast(torch::Tensor scale, torch::Tensor X) {
    auto s = scale.contiguous(), x = X.contiguous();
    check_dev(s, torch::kFloat, "scale");
    check_dev(x, torch::kFloat, "X");
    const int64_t n = x.size(0), F = x.numel() / std::max<int64_t>(n, 1);
    auto out = torch::empty_like(x);
    check_on(s, x, "scale");
    check(be(x).row_broadcast(n, (int32_t)F, s.data_ptr<float>(), x.data_ptr<float>(), F,
                              out.data_ptr<float>(), F, stream_of(x)),
          "gala_row_broadcast_f32");
    return out;
}

torch::Tensor degree_norm(torch::Tensor offset_graph, torch::Tensor bounds, int64_t segments,
                          double power, torch::Tensor columns_graph) {
    TORCH_CHECK(segments == 1 || columns_graph.defined(),
                "gala: degree_norm of a column-tiled graph needs its columns_graph");
    // the degree kernel reads rowptr only; the columns give the segment bounds their range
    auto cols = columns_graph.defined() ? columns_graph : torch::empty({0}, offset_graph.options());
    CsrView cv = view(offset_graph, cols, nullptr, bounds, segments);
    auto out = torch::empty({cv.c.n_rows, 1}, fopts(offset_graph));
    check(be(offset_graph).degree(&cv.c, out.data_ptr<float>(), (float)power, 0, 0,
                                  stream_of(offset_graph)),
          "gala_degree_f32");
    return out;
}

torch::Tensor gcn_aggregate(torch::Tensor X, torch::Tensor norm, torch::Tensor offset_graph,
                            torch::Tensor columns_graph, torch::Tensor bounds, int64_t segments) {
    // norm * A (norm * X): prescale pass (streaming) + SpMM with the dst norm fused; the
    // src norm is not fused into the SpMM because a per-edge norm[col] gather costs as much
    // as the feature row itself at F <= 32
    auto xs = row_broadcast(norm, X);
    return spmm_impl(xs, offset_graph, columns_graph, nullptr, bounds, segments, 1, nullptr,
                     &norm, 0, 5, 7);
}

// ---- autograd Functions ------------------------------------------------------------------
using torch::autograd::AutogradContext;
using torch::autograd::tensor_list;

namespace {

struct Slot {
    torch::Tensor off, cols, vals, bounds, perm;
    int segs;
    bool weighted;
};

Slot slot(int64_t idx) {
    auto &S = global_slots();
    TORCH_CHECK(idx >= 0 && idx < (int64_t)S.offset_graph.size(), "gala: graph slot ", idx,
                " not registered");
    return {S.offset_graph[idx], S.columns_graph[idx], S.value_graph[idx], S.bounds[idx],
            S.transpose_perm[idx], S.segments[idx], S.weighted[idx]};
}

// aggregate_node_mul_sum_coarse{C}_AutoGrad (common.h:928-978; gala.cu:391-414)
struct AggregateNodeMulSum : public torch::autograd::Function<AggregateNodeMulSum> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor input_dense, int64_t li) {
        ctx->saved_data["li"] = li;
        Slot s = slot(2 * li);
        auto &S = global_slots();
        return aggregate_node_mul_sum_call(input_dense, s.off, s.cols, s.vals, s.bounds, s.segs,
                                           s.weighted, S.nsamples, S.ra, S.rb);
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        const int64_t li = ctx->saved_data["li"].toInt();
        Slot s = slot(2 * li + 1);
        auto &S = global_slots();
        return {aggregate_node_mul_sum_call(grad_outputs[0], s.off, s.cols, s.vals, s.bounds,
                                            s.segs, s.weighted, S.nsamples, S.ra, S.rb),
                torch::Tensor()};
    }
};

// attention-weighted variant (hasFFNEdgeUpdate, common.h:835-894)
struct AggregateNodeMulSumAttn : public torch::autograd::Function<AggregateNodeMulSumAttn> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor input_dense,
                                 torch::Tensor value_graph, int64_t li) {
        ctx->saved_data["li"] = li;
        ctx->save_for_backward({value_graph, input_dense});
        Slot s = slot(2 * li);
        return aggregate_node_mul_sum_call(input_dense, s.off, s.cols, value_graph.contiguous(),
                                           s.bounds, s.segs, true);
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        auto saved = ctx->get_saved_variables();
        torch::Tensor value_graph = saved[0], X = saved[1];
        torch::Tensor dZ = grad_outputs[0].contiguous();
        const int64_t li = ctx->saved_data["li"].toInt();
        Slot s = slot(2 * li + 1);
        const int64_t nrows = s.off.numel() / s.segs - 1;
        // fixed weights (the sparse rewrite's norm_i * norm_j) need no d alpha
        torch::Tensor dalpha = ctx->needs_input_grad(1)
                                   ? edge_sddmm(dZ, X, s.off, s.cols, value_graph, s.bounds, nrows, s.segs)
                                   : torch::Tensor();
        return {aggregate_node_mul_sum_call(dZ, s.off, s.cols, value_graph, s.bounds, s.segs, true),
                dalpha, torch::Tensor()};
    }
};

// aggregate_edge_sum_AutoGrad (common.h:622-675)
struct AggregateEdgeSum : public torch::autograd::Function<AggregateEdgeSum> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor in1, torch::Tensor in2,
                                 int64_t li) {
        ctx->saved_data["li"] = li;
        Slot s = slot(2 * li);
        const int64_t nrows = s.off.numel() / s.segs - 1;
        return edge_sddvv(in1, in2, s.off, s.cols, s.vals, s.bounds, nrows, s.segs);
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        const int64_t li = ctx->saved_data["li"].toInt();
        Slot s = slot(2 * li + 1);
        const int64_t nrows = s.off.numel() / s.segs - 1;
        auto back_res = node_spmv_backward_of_sddmm_eaggr(s.off, s.cols, grad_outputs[0], s.bounds,
                                                          nrows, s.segs);
        return {back_res, back_res, torch::Tensor()};
    }
};

// non_lnr_op_softmax_AutoGrad (common.h:735-810), fused: one kernel per direction
struct NonLnrOpSoftmax : public torch::autograd::Function<NonLnrOpSoftmax> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor value_graph, int64_t li) {
        ctx->saved_data["li"] = li;
        Slot s = slot(2 * li);
        CsrView cv = view(s.off, s.cols, nullptr, s.bounds, s.segs);
        with_workspace(cv, s.off, 2);
        auto v = value_graph.contiguous();
        check_dev(v, torch::kFloat, "value_graph");
        auto alpha = torch::empty_like(v);
        check_on(v, s.off, "value_graph");
        check(be(s.off).softmax_fwd(&cv.c, v.data_ptr<float>(), 1, GALA_SOFTMAX_REF,
                                    alpha.data_ptr<float>(), stream_of(s.off)),
              "gala_edge_softmax_fwd_f32");
        ctx->save_for_backward({alpha});
        return alpha;
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        const int64_t li = ctx->saved_data["li"].toInt();
        Slot s = slot(2 * li + 1);
        CsrView cv = view(s.off, s.cols, nullptr, s.bounds, s.segs);
        with_workspace(cv, s.off, 2);
        auto alpha = ctx->get_saved_variables()[0];
        auto d = grad_outputs[0].contiguous();
        auto ds = torch::empty_like(alpha);
        check_on(d, s.off, "grad");
        check(be(s.off).softmax_bwd(&cv.c, alpha.data_ptr<float>(), d.data_ptr<float>(), 1,
                                    GALA_SOFTMAX_REF, ds.data_ptr<float>(), stream_of(s.off)),
              "gala_edge_softmax_bwd_f32");
        return {ds, torch::Tensor()};
    }
};

torch::Tensor permute_edges(const torch::Tensor &perm, const torch::Tensor &v, int heads) {
    auto out = torch::empty_like(v);
    check_on(v, perm, "edge values");
    check(be(perm).permute(perm.data_ptr<int32_t>(), v.data_ptr<float>(), perm.numel(), heads,
                           out.data_ptr<float>(), stream_of(perm)),
          "gala_edge_permute_f32");
    return out;
}

// slot 2li+1 is slot 2li itself (the runtime registers an undirected graph's backward
// slot with the forward tensors, as gala.cu does)
bool same_pattern(const Slot &a, const Slot &b) {
    return a.off.data_ptr() == b.off.data_ptr() && a.cols.data_ptr() == b.cols.data_ptr() &&
           a.segs == b.segs;
}

struct GatGrads {
    torch::Tensor daL, daR, dX;
};

// Gradients of the per-head Linear(D, 1) out[r,h] = <x[r, head h], w[head h]> + b[h]:
// dW[head h] = sum_r g[r,h] x[r, head h], db[h] = sum_r g[r,h] -- the block diagonal of
// gala_dense_grad_f32's [heads, F] dW = g^T x.
void head_linear_grads(const torch::Tensor &x, const torch::Tensor &g, const torch::Tensor &w, int heads,
                       torch::Tensor &dW, torch::Tensor &db) {
    const int64_t N = x.size(0);
    const int32_t F = (int32_t)x.size(1), D = F / heads;
    auto full = torch::empty({heads, F}, fopts(x));
    db = torch::empty({heads}, fopts(x));
    const Backend &B = be(x);
    const int64_t wsb = B.dense_ws(N, F, heads);
    TORCH_CHECK(wsb >= 0, "gala: gala_dense_grad_workspace failed");
    auto ws = torch::empty({std::max<int64_t>(wsb / 4, 1)}, fopts(x));
    check(B.dense_grad(N, F, heads, x.data_ptr<float>(), x.stride(0), g.data_ptr<float>(), heads,
                       full.data_ptr<float>(), db.data_ptr<float>(), 0, ws.data_ptr<float>(), wsb, stream_of(x)),
          "gala_dense_grad_f32");
    dW = full.view({heads, heads, D}).diagonal(0, 0, 1).t().reshape(w.sizes());  // [h, h*D + d]
}

// alpha = p * q (rounded) of a factored attention output, materialised on the forward
// pattern (gala_row_scale_f32: the same product the fused kernels form per edge)
torch::Tensor materialise_alpha(const Slot &fw, const torch::Tensor &p, const torch::Tensor &q) {
    auto a = p.clone();
    return row_scale_impl(q, fw.off, fw.cols, a, fw.bounds, fw.off.numel() / fw.segs - 1, fw.segs);
}

// Backward of the fused GAT layer (both autograd Functions below).  r is the source logit
// aR; with wR defined and r undefined, aR[j,h] = <X[j, head h], wR[head h]> + bR[h] was
// recomputed inside the forward kernel, and is either recomputed again by the backward
// kernel (REF on one pattern) or formed here for the other paths.  q defined: `alpha`
// holds the forward's factored p (REF), alpha = p * q.
GatGrads gat_backward(const torch::Tensor &l, torch::Tensor r, const torch::Tensor &x,
                      torch::Tensor alpha, torch::Tensor q, const torch::Tensor &dY_in, int64_t li,
                      double slope, int64_t mode, int heads, const torch::Tensor &wR,
                      const torch::Tensor &bR) {
    Slot fw = slot(2 * li), bw = slot(2 * li + 1);
    const int64_t nrows = fw.off.numel() / fw.segs - 1, F = x.size(1);
    // one head: dY row-padded like x (the dX SpMM gathers it), strides passed through
    const torch::Tensor dY = heads == 1 ? pad_rows4(dY_in) : dY_in.contiguous();
    const int64_t ldx = x.stride(0), lddy = dY.stride(0);
    CsrView cf = view(fw.off, fw.cols, nullptr, fw.bounds, fw.segs);
    cf.c.n_cols = x.size(0);
    with_workspace(cf, fw.off, 3 * heads);  // hub-row partials of the backward
    check_on(dY, fw.off, "grad");
    const bool fixed = mode == GALA_SOFTMAX_FIXED;
    TORCH_CHECK(!fixed || bw.perm.defined(),
                "gala: FIXED-mode GAT backward needs the transposed graph and its edge "
                "permutation in slot 2*li+1 (transpose_perm)");
    const bool same = same_pattern(fw, bw);
    // the factored (p, q) pair feeds the dX SpMM and the fused kernel directly when both run
    // on the forward pattern; elsewhere alpha is materialised once
    if (q.defined() && (fixed || !same)) {
        alpha = materialise_alpha(fw, alpha, q);
        q = torch::Tensor();
    }
    // dX: reference multiplies by alpha on slot 2li+1's pattern (common.h:876);
    // FIXED: A^T with the transposed alpha
    torch::Tensor alpha_b = fixed ? permute_edges(bw.perm, alpha, heads) : alpha;
    torch::Tensor dX = spmm_impl(dY, bw.off, bw.cols, &alpha_b, bw.bounds, bw.segs, heads,
                                 nullptr, nullptr, 0, 5, 7, q.defined() ? &q : nullptr);
    // one fused edge kernel for d alpha -> softmax bwd -> LeakyReLU bwd -> row sum when
    // every step runs on one pattern: FIXED always (slot 2li), REF when slot 2li+1 is
    // the forward graph itself (undirected graphs: cuda.h:1253-1257)
    const float *qp = q.defined() ? q.data_ptr<float>() : nullptr;
    if (!r.defined() && !fixed && same) {
        auto daL = torch::empty_like(l);
        const int st = be(fw.off).gat_bwd_ex(&cf.c, l.data_ptr<float>(), nullptr, wR.data_ptr<float>(),
                                             bR.defined() ? bR.data_ptr<float>() : nullptr,
                                             x.data_ptr<float>(), ldx, dY.data_ptr<float>(), lddy,
                                             (int32_t)F, heads, (float)slope, GALA_SOFTMAX_REF,
                                             alpha.data_ptr<float>(), qp, nullptr, daL.data_ptr<float>(),
                                             stream_of(fw.off));
        if (st != GALA_ERR_UNSUPPORTED) {
            check(st, "gala_gat_bwd_ex_f32");
            return {daL, daL, dX};
        }
    }
    if (q.defined()) {  // the paths below take alpha itself
        alpha = materialise_alpha(fw, alpha, q);
        q = torch::Tensor();
        qp = nullptr;
    }
    if (!r.defined()) {  // the explicit (per-head) source logits for the other paths
        if (heads == 1) {
            r = x.mv(wR.reshape({-1}));
        } else {
            const int64_t D = F / heads;
            r = (x.reshape({x.size(0), heads, D}) * wR.reshape({1, heads, D})).sum(2);
        }
        if (bR.defined()) r = r + bR.reshape({-1});
        r = r.contiguous();
    }
    if (fixed || same) {
        auto daL = torch::empty_like(l);
        torch::Tensor dz = fixed ? torch::empty_like(alpha) : torch::Tensor();
        const int st = be(fw.off).gat_bwd(&cf.c, l.data_ptr<float>(), r.data_ptr<float>(),
                                          x.data_ptr<float>(), ldx, dY.data_ptr<float>(), lddy,
                                          (int32_t)F, heads, (float)slope, (int32_t)mode,
                                          alpha.data_ptr<float>(),
                                          fixed ? dz.data_ptr<float>() : nullptr,
                                          daL.data_ptr<float>(), stream_of(fw.off));
        if (st != GALA_ERR_UNSUPPORTED) {
            check(st, "gala_gat_bwd_f32");
            torch::Tensor daR = daL;
            if (fixed) {
                auto dzT = permute_edges(bw.perm, dz, heads);
                daR = row_sum_impl(bw.off, bw.cols, dzT, bw.bounds,
                                   bw.off.numel() / bw.segs - 1, bw.segs, 0.0f);
            }
            return {daL, daR, dX};
        }
    }
    // d alpha_e = <dY_row, X_col> per head (edge_sddmm, cuda.h:808-845)
    const Slot &ps = fixed ? fw : bw;
    CsrView cp = view(ps.off, ps.cols, nullptr, ps.bounds, ps.segs);
    cp.c.n_cols = x.size(0);
    with_workspace(cp, ps.off, 2 * heads);
    auto dalpha = torch::empty_like(alpha);
    check(be(ps.off).sddmm(&cp.c, dY.data_ptr<float>(), lddy, x.data_ptr<float>(), ldx,
                           (int32_t)F, heads, dalpha.data_ptr<float>(), stream_of(ps.off)),
          "gala_sddmm_dot_f32");
    auto ds = torch::empty_like(alpha);
    check(be(ps.off).softmax_bwd(&cp.c, alpha.data_ptr<float>(), dalpha.data_ptr<float>(),
                                 heads, (int32_t)mode, ds.data_ptr<float>(), stream_of(ps.off)),
          "gala_edge_softmax_bwd_f32");
    // LeakyReLU backward on the recomputed logits z = aL[row] + aR[col]
    auto z = torch::empty_like(alpha);
    check(be(fw.off).sddvv(&cf.c, l.data_ptr<float>(), r.data_ptr<float>(), heads,
                           GALA_SDDVV_ADD, 0.0f, z.data_ptr<float>(), stream_of(fw.off)),
          "gala_sddvv_f32");
    auto dz = torch::where(z > 0, ds, ds * slope).contiguous();
    torch::Tensor daL, daR;
    if (!fixed) {
        // reference: d aL = d aR = K7(ds) on slot 2li+1 (common.h:662-667)
        daL = row_sum_impl(bw.off, bw.cols, dz, bw.bounds, nrows, bw.segs, 1e-12f);
        daR = daL;
    } else {
        daL = row_sum_impl(fw.off, fw.cols, dz, fw.bounds, nrows, fw.segs, 0.0f);
        auto dzT = permute_edges(bw.perm, dz, heads);
        daR = row_sum_impl(bw.off, bw.cols, dzT, bw.bounds, bw.off.numel() / bw.segs - 1,
                           bw.segs, 0.0f);
    }
    return {daL, daR, dX};
}

// One launch of the fused GAT forward (gala_gat_fwd_ex_f32) on slot 2li: aR, or its
// per-head recompute from x (wR, bR).  alpha / q as the entry point documents.
torch::Tensor gat_forward_launch(const Slot &s, const torch::Tensor &l, const torch::Tensor &r,
                                 const torch::Tensor &x, const torch::Tensor &wR, const torch::Tensor &bR,
                                 int heads, double slope, int64_t mode, float *alpha, float *q) {
    CsrView cv = view(s.off, s.cols, nullptr, s.bounds, s.segs);
    const int64_t nrows = cv.c.n_rows, F = x.size(1);
    cv.c.n_cols = x.size(0);
    with_workspace(cv, s.off, F + 2 * heads);  // hub-row partials: acc[F], m[H], sum[H]
    auto Y = rows_like(x, nrows);
    check(be(s.off).gat_fwd_ex(&cv.c, l.data_ptr<float>(), r.defined() ? r.data_ptr<float>() : nullptr,
                               r.defined() ? nullptr : wR.data_ptr<float>(),
                               (!r.defined() && bR.defined()) ? bR.data_ptr<float>() : nullptr,
                               x.data_ptr<float>(), x.stride(0), (int32_t)F, heads, (float)slope,
                               (int32_t)mode, Y.data_ptr<float>(), Y.stride(0), alpha, q, stream_of(s.off)),
          "gala_gat_fwd_ex_f32");
    return Y;
}

// REF backward with the attention recomputed from the forward's q (the forward stored no
// alpha): one kernel for dX and d_aL (= d_aR), gala_gat_bwd_fused_f32.  Returns false when
// the kernel does not take this shape (then the caller rebuilds alpha).
bool gat_backward_recompute(const torch::Tensor &l, const torch::Tensor &r, const torch::Tensor &x,
                            const torch::Tensor &q, const torch::Tensor &dY_in, int64_t li, double slope,
                            int heads, const torch::Tensor &wR, const torch::Tensor &bR, GatGrads &g) {
    Slot fw = slot(2 * li);
    const torch::Tensor dY = heads == 1 ? pad_rows4(dY_in) : dY_in.contiguous();
    const int64_t F = x.size(1), nrows = fw.off.numel() / fw.segs - 1;
    CsrView cf = view(fw.off, fw.cols, nullptr, fw.bounds, fw.segs);
    cf.c.n_cols = x.size(0);
    with_workspace(cf, fw.off, (F + 3) / 4 * 4 + 3 * heads);  // hub rows: dX[F] + 3 sums per head
    check_on(dY, fw.off, "grad");
    auto dX = rows_like(dY, nrows);
    auto daL = torch::empty_like(l);
    const int st = be(fw.off).gat_bwd_fused(&cf.c, l.data_ptr<float>(), r.defined() ? r.data_ptr<float>() : nullptr,
                                            r.defined() ? nullptr : wR.data_ptr<float>(),
                                            (!r.defined() && bR.defined()) ? bR.data_ptr<float>() : nullptr,
                                            x.data_ptr<float>(), x.stride(0), dY.data_ptr<float>(), dY.stride(0),
                                            (int32_t)F, heads, (float)slope, q.data_ptr<float>(),
                                            dX.data_ptr<float>(), dX.stride(0), daL.data_ptr<float>(),
                                            stream_of(fw.off));
    if (st == GALA_ERR_UNSUPPORTED) return false;
    check(st, "gala_gat_bwd_fused_f32");
    g = {daL, daL, dX};
    return true;
}

// REF on one pattern: the forward keeps only q (alpha is recomputed by the backward)
bool recompute_attention(int64_t li, int64_t mode) {
    return mode == GALA_SOFTMAX_REF && same_pattern(slot(2 * li), slot(2 * li + 1));
}

// The row-statistics variant of the recomputed REF layer (gala_gat_{fwd,bwd}_stats_f32):
// the forward also keeps Ym = sum m*alpha*X and sma = sum m*alpha per row, and the backward
// gathers dY[col] only.  GALA_GAT_ROWSTATS=0 keeps the X-gathering fused backward.
bool rowstats_enabled() {
    static const bool on = [] {
        const char *e = std::getenv("GALA_GAT_ROWSTATS");
        return !(e && e[0] == '0');
    }();
    return on;
}

// What the row-statistics forward leaves for its backward.
struct GatStats {
    torch::Tensor Y, q, Ym, sma, aR;  // aR: the given logits, or the recomputed ones (RC)
    torch::Tensor p;                  // narrow rows: the edges' exp terms (else empty)
};

// Narrow layers keep the forward's per-edge exp terms p (4 B per edge and head, written and
// read in edge order) so the backward skips its aR[col] gather, which costs a whole cache
// line per edge next to a 1-2 line row gather; wide rows hide that read.
bool keep_edge_terms(int64_t F) { return F <= 64; }

// One launch of gala_gat_fwd_stats_f32 on slot 2li; false when the kernel does not take
// this shape (the caller then takes the plain recomputed path).
bool gat_forward_stats(const Slot &s, const torch::Tensor &l, const torch::Tensor &r, const torch::Tensor &x,
                       const torch::Tensor &wR, const torch::Tensor &bR, int heads, double slope, GatStats &o) {
    CsrView cv = view(s.off, s.cols, nullptr, s.bounds, s.segs);
    const int64_t nrows = cv.c.n_rows, F = x.size(1);
    if (x.size(0) != nrows) return false;  // a square pattern only
    cv.c.n_cols = x.size(0);
    with_workspace(cv, s.off, 2 * ((F + 3) / 4 * 4) + 3 * heads);  // hub rows: {acc, m, sum, accm, sma}
    auto Y = rows_like(x, nrows), Ym = rows_like(x, nrows);
    auto q = torch::empty({nrows * heads}, fopts(x)), sma = torch::empty({nrows * heads}, fopts(x));
    torch::Tensor aR = r.defined() ? r : torch::empty({nrows * heads}, fopts(x));
    torch::Tensor p = keep_edge_terms(F) ? torch::empty({s.cols.numel() * heads}, fopts(x)) : torch::Tensor();
    const int st = be(s.off).gat_fwd_stats(
        &cv.c, l.data_ptr<float>(), r.defined() ? r.data_ptr<float>() : nullptr,
        r.defined() ? nullptr : wR.data_ptr<float>(), (!r.defined() && bR.defined()) ? bR.data_ptr<float>() : nullptr,
        x.data_ptr<float>(), x.stride(0), (int32_t)F, heads, (float)slope, Y.data_ptr<float>(), Y.stride(0),
        q.data_ptr<float>(), Ym.data_ptr<float>(), Ym.stride(0), sma.data_ptr<float>(),
        r.defined() ? nullptr : aR.data_ptr<float>(), p.defined() ? p.data_ptr<float>() : nullptr,
        stream_of(s.off));
    if (st == GALA_ERR_UNSUPPORTED) return false;
    check(st, "gala_gat_fwd_stats_f32");
    o = {Y, q, Ym, sma, aR, p.defined() ? p : torch::empty({0}, fopts(x))};
    return true;
}

// REF backward from the row statistics: dX and d_aL (= d_aR) in one kernel that gathers
// dY[col] only.  wR (defined): dX also takes the source logit's per-head Linear, d_aR * wR
// (gala_gat_bwd_stats_linear_f32, bit-identical to a gala_head_attn_bwd_f32 pass after it).
bool gat_backward_stats(const torch::Tensor &l, const GatStats &o, const torch::Tensor &dY_in, int64_t li,
                        double slope, int heads, GatGrads &g, const torch::Tensor &wR = torch::Tensor()) {
    Slot fw = slot(2 * li);
    const torch::Tensor dY = heads == 1 ? pad_rows4(dY_in) : dY_in.contiguous();
    const int64_t F = o.Y.size(1), nrows = fw.off.numel() / fw.segs - 1;
    CsrView cf = view(fw.off, fw.cols, nullptr, fw.bounds, fw.segs);
    cf.c.n_cols = dY.size(0);
    with_workspace(cf, fw.off, (F + 3) / 4 * 4);  // hub rows: dX[F] chunk partials
    check_on(dY, fw.off, "grad");
    auto dX = rows_like(dY, nrows);
    auto daL = torch::empty_like(l);
    const float *pp = o.p.numel() > 0 ? o.p.data_ptr<float>() : nullptr;
    const int st = wR.defined()
        ? be(fw.off).gat_bwd_stats_linear(&cf.c, l.data_ptr<float>(), o.aR.data_ptr<float>(), pp,
                                          dY.data_ptr<float>(), dY.stride(0), nullptr, (int32_t)F, heads,
                                          (float)slope, o.q.data_ptr<float>(), o.Y.data_ptr<float>(), o.Y.stride(0),
                                          o.Ym.data_ptr<float>(), o.Ym.stride(0), o.sma.data_ptr<float>(),
                                          wR.data_ptr<float>(), dX.data_ptr<float>(), dX.stride(0),
                                          daL.data_ptr<float>(), stream_of(fw.off))
        : be(fw.off).gat_bwd_stats(&cf.c, l.data_ptr<float>(), o.aR.data_ptr<float>(), pp,
                                   dY.data_ptr<float>(), dY.stride(0), (int32_t)F, heads, (float)slope,
                                   o.q.data_ptr<float>(), o.Y.data_ptr<float>(), o.Y.stride(0),
                                   o.Ym.data_ptr<float>(), o.Ym.stride(0), o.sma.data_ptr<float>(),
                                   dX.data_ptr<float>(), dX.stride(0), daL.data_ptr<float>(),
                                   stream_of(fw.off));
    if (st == GALA_ERR_UNSUPPORTED) return false;
    check(st, "gala_gat_bwd_stats_f32");
    g = {daL, daL, dX};
    return true;
}

// The exact pair for a FIXED layer (gala_gat_{fwd,bwd}_stats_exact_f32): the stable softmax
// and the true gradients from row statistics -- no alpha, no permutation, one gather of dY
// rows.  Taken when the forward pattern is one square segment that is symmetric (a host
// transpose on first use, kept with the pattern) and slot 2li+1 holds that same pattern (the
// runtime uploads the transpose there: compared once per pair of slots).
// GALA_GAT_EXACT_STATS=0 keeps the alpha-storing path.
}  // namespace
const PatternT &transposed_pattern(int64_t idx);
namespace {
bool exact_stats_enabled() {  // read per layer call: an A/B run switches it inside one process
    const char *e = std::getenv("GALA_GAT_EXACT_STATS");
    return !(e && e[0] == '0');
}

bool exact_stats_layer(int64_t li, int64_t x_rows) {
    if (!exact_stats_enabled()) return false;
    Slot fw = slot(2 * li), bw = slot(2 * li + 1);
    if (fw.segs != 1 || bw.segs != 1 || fw.off.numel() - 1 != x_rows) return false;
    // slot 2li+1 must hold the forward's pattern: the same tensors, or equal ones (compared on
    // the device once per slot).  A directed graph's transpose differs from it, so such a layer
    // leaves here without the host transpose below
    if (!same_pattern(fw, bw)) {
        int8_t &same = global_slots().holds_previous[2 * li + 1];
        if (same < 0)
            same = bw.off.numel() == fw.off.numel() && bw.cols.numel() == fw.cols.numel() &&
                   torch::equal(bw.off, fw.off) && torch::equal(bw.cols, fw.cols);
        if (!same) return false;
    }
    return transposed_pattern(2 * li).symmetric;  // tested once, kept with the slot
}

// The directed pair (GALA_GAT_EXACT_DIRECTED=1, off by default; read per layer call like the
// switch above): the exact forward on slot 2li and gala_gat_bwd_stats_exact_t_f32, whose gather
// pass walks slot 2li+1, for a FIXED layer whose two slots are distinct, single-segment,
// square, unweighted and unsampled -- once gala_csr_is_transpose_i32 has found slot 2li+1 to
// be slot 2li's transpose (one pass over the edges on the device, once per pair of slots; no
// host transpose).
bool exact_directed_enabled() {
    const char *e = std::getenv("GALA_GAT_EXACT_DIRECTED");
    return e && e[0] == '1';
}

bool exact_directed_layer(int64_t li, int64_t x_rows) {
    if (!exact_directed_enabled()) return false;
    Slot fw = slot(2 * li), bw = slot(2 * li + 1);
    auto &S = global_slots();
    if (fw.segs != 1 || bw.segs != 1 || fw.weighted || bw.weighted || S.nsamples != 0) return false;
    if (fw.off.numel() - 1 != x_rows || bw.off.numel() != fw.off.numel()) return false;
    if (same_pattern(fw, bw) || fw.off.device() != bw.off.device()) return false;
    int8_t &tr = S.transposes_previous[2 * li + 1];
    if (tr < 0) {
        CsrView a = view(fw.off, fw.cols, nullptr, fw.bounds, fw.segs);
        CsrView t = view(bw.off, bw.cols, nullptr, bw.bounds, bw.segs);
        auto count = torch::empty({1}, torch::TensorOptions().dtype(torch::kInt).device(fw.off.device()));
        check(be(fw.off).csr_is_transpose(&a.c, &t.c, count.data_ptr<int32_t>(), stream_of(fw.off)),
              "gala_csr_is_transpose_i32");
        tr = count.item<int32_t>() == 0;
    }
    return tr;
}

struct GatExact {
    torch::Tensor Y, lse, Ym, sma, aR;  // aR: the given logits, or the kernel's recompute
};

// One launch of gala_gat_fwd_stats_exact_f32 on slot 2li; false when the kernel does not
// take this shape (the caller keeps the alpha-storing path).
bool gat_forward_exact(const Slot &s, const torch::Tensor &l, const torch::Tensor &r, const torch::Tensor &x,
                       const torch::Tensor &wR, const torch::Tensor &bR, int heads, double slope, GatExact &o) {
    CsrView cv = view(s.off, s.cols, nullptr, s.bounds, s.segs);
    const int64_t nrows = cv.c.n_rows, F = x.size(1);
    cv.c.n_cols = x.size(0);
    with_workspace(cv, s.off, 2 * ((F + 3) / 4 * 4) + 3 * heads);  // hub rows: {acc, m, sum, accm, sma}
    auto Y = rows_like(x, nrows), Ym = rows_like(x, nrows);
    auto lse = torch::empty({nrows * heads}, fopts(x)), sma = torch::empty({nrows * heads}, fopts(x));
    torch::Tensor aR = r.defined() ? r : torch::empty({nrows * heads}, fopts(x));
    const int st = be(s.off).gat_fwd_stats_exact(
        &cv.c, l.data_ptr<float>(), r.defined() ? r.data_ptr<float>() : nullptr,
        r.defined() ? nullptr : wR.data_ptr<float>(), (!r.defined() && bR.defined()) ? bR.data_ptr<float>() : nullptr,
        x.data_ptr<float>(), x.stride(0), (int32_t)F, heads, (float)slope, Y.data_ptr<float>(), Y.stride(0),
        lse.data_ptr<float>(), Ym.data_ptr<float>(), Ym.stride(0), sma.data_ptr<float>(),
        r.defined() ? nullptr : aR.data_ptr<float>(), stream_of(s.off));
    if (st == GALA_ERR_UNSUPPORTED) return false;
    check(st, "gala_gat_fwd_stats_exact_f32");
    o = {Y, lse, Ym, sma, aR};
    return true;
}

// The exact backward: dX, d_aL and d_aR (distinct) from the forward's rows.
// directed: the gather pass over slot 2li+1, the forward pattern's transpose (its own plan).
bool gat_backward_exact(const torch::Tensor &l, const GatExact &o, const torch::Tensor &x,
                        const torch::Tensor &dY_in, int64_t li, double slope, int heads, GatGrads &g,
                        bool directed = false) {
    Slot fw = slot(2 * li);
    const torch::Tensor dY = heads == 1 ? pad_rows4(dY_in) : dY_in.contiguous();
    const int64_t F = o.Y.size(1), nrows = fw.off.numel() / fw.segs - 1;
    CsrView cf = view(fw.off, fw.cols, nullptr, fw.bounds, fw.segs);
    cf.c.n_cols = dY.size(0);
    if (!directed) with_workspace(cf, fw.off, 2 * ((F + 3) / 4 * 4) + heads);  // hub rows: {dX, dXm, sg}
    check_on(dY, fw.off, "grad");
    auto dX = rows_like(dY, nrows);
    auto daL = torch::empty_like(l), daR = torch::empty_like(l);
    auto side = torch::empty({nrows * heads * 4}, fopts(x));   // {aL, lse, g, 0} per (row, head)
    if (directed) {
        Slot bw = slot(2 * li + 1);
        CsrView ct = view(bw.off, bw.cols, nullptr, bw.bounds, bw.segs);
        with_workspace(ct, bw.off, 2 * ((F + 3) / 4 * 4) + heads);  // hub rows of A^T: {dX, dXm, sg}
        const int st = be(fw.off).gat_bwd_stats_exact_t(
            &cf.c, &ct.c, l.data_ptr<float>(), o.aR.data_ptr<float>(), x.data_ptr<float>(), x.stride(0),
            dY.data_ptr<float>(), dY.stride(0), (int32_t)F, heads, (float)slope, o.lse.data_ptr<float>(),
            o.Y.data_ptr<float>(), o.Y.stride(0), o.Ym.data_ptr<float>(), o.Ym.stride(0), o.sma.data_ptr<float>(),
            side.data_ptr<float>(), dX.data_ptr<float>(), dX.stride(0), daL.data_ptr<float>(), daR.data_ptr<float>(),
            stream_of(fw.off));
        if (st == GALA_ERR_UNSUPPORTED) return false;
        check(st, "gala_gat_bwd_stats_exact_t_f32");
        g = {daL, daR, dX};
        return true;
    }
    const int st = be(fw.off).gat_bwd_stats_exact(
        &cf.c, l.data_ptr<float>(), o.aR.data_ptr<float>(), x.data_ptr<float>(), x.stride(0), dY.data_ptr<float>(),
        dY.stride(0), (int32_t)F, heads, (float)slope, o.lse.data_ptr<float>(), o.Y.data_ptr<float>(), o.Y.stride(0),
        o.Ym.data_ptr<float>(), o.Ym.stride(0), o.sma.data_ptr<float>(), side.data_ptr<float>(),
        dX.data_ptr<float>(), dX.stride(0), daL.data_ptr<float>(), daR.data_ptr<float>(), stream_of(fw.off));
    if (st == GALA_ERR_UNSUPPORTED) return false;
    check(st, "gala_gat_bwd_stats_exact_f32");
    g = {daL, daR, dX};
    return true;
}

// fused GAT layer: sddvv + LeakyReLU + edge softmax + weighted aggregation in one pass.
// REF mode keeps the attention factored (p per edge, q per row: no normalisation pass over
// the edges); FIXED materialises alpha (its backward needs the transposed alpha).
struct GatAggregate : public torch::autograd::Function<GatAggregate> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor aL, torch::Tensor aR,
                                 torch::Tensor X, int64_t li, double slope, int64_t mode) {
        Slot s = slot(2 * li);
        auto l = aL.contiguous(), r = aR.contiguous();
        const int64_t nrows = s.off.numel() / s.segs - 1;
        const int heads = (int)(l.numel() / std::max<int64_t>(nrows, 1));
        auto x = heads == 1 ? pad_rows4(X) : X.contiguous();
        check_dev(l, torch::kFloat, "attn_l");
        check_dev(r, torch::kFloat, "attn_r");
        check_dev(x, torch::kFloat, "X");
        check_on(l, s.off, "attn_l");
        check_on(r, s.off, "attn_r");
        check_on(x, s.off, "X");
        // REF on one pattern: q only (the backward recomputes alpha); REF otherwise: the
        // factored (p, q); FIXED: alpha itself (its backward permutes it onto A^T)
        const bool recompute = recompute_attention(li, mode);
        const bool factored = mode == GALA_SOFTMAX_REF;
        ctx->saved_data["li"] = li;
        ctx->saved_data["slope"] = slope;
        ctx->saved_data["mode"] = mode;
        ctx->saved_data["heads"] = (int64_t)heads;
        GatStats o;
        // the statistics only serve a backward: none without gradients (eval forwards)
        const bool grad = ctx->needs_input_grad(0) || ctx->needs_input_grad(1) || ctx->needs_input_grad(2);
        GatExact ex;
        const bool fixed_grad = mode == GALA_SOFTMAX_FIXED && grad;
        const bool symm = fixed_grad && exact_stats_layer(li, x.size(0));
        const bool directed = fixed_grad && !symm && exact_directed_layer(li, x.size(0));
        if ((symm || directed) &&
            gat_forward_exact(s, l, r, x, {}, {}, heads, slope, ex)) {
            ctx->saved_data["exact"] = true;
            if (directed) ctx->saved_data["exact_t"] = true;
            ctx->save_for_backward({l, r, x, ex.lse, ex.Y, ex.Ym, ex.sma});
            return ex.Y;
        }
        if (recompute && grad && rowstats_enabled() && gat_forward_stats(s, l, r, x, {}, {}, heads, slope, o)) {
            ctx->saved_data["stats"] = true;
            ctx->save_for_backward({l, r, x, o.q, o.Y, o.Ym, o.sma, o.p});
            return o.Y;
        }
        auto alpha = recompute ? torch::empty({0}, fopts(x)) : torch::empty({s.cols.numel() * heads}, fopts(x));
        auto q = factored ? torch::empty({nrows * heads}, fopts(x)) : torch::empty({0}, fopts(x));
        auto Y = gat_forward_launch(s, l, r, x, {}, {}, heads, slope, mode,
                                    recompute ? nullptr : alpha.data_ptr<float>(),
                                    factored ? q.data_ptr<float>() : nullptr);
        ctx->save_for_backward({l, r, x, alpha, q});
        return Y;
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        auto sv = ctx->get_saved_variables();
        const int64_t li = ctx->saved_data["li"].toInt(), mode = ctx->saved_data["mode"].toInt();
        const double slope = ctx->saved_data["slope"].toDouble();
        const int heads = (int)ctx->saved_data["heads"].toInt();
        auto l = sv[0], r = sv[1], x = sv[2];
        GatGrads g;
        if (ctx->saved_data.count("exact")) {
            const GatExact ex{sv[4], sv[3], sv[5], sv[6], r};
            if (!gat_backward_exact(l, ex, x, grad_outputs[0], li, slope, heads, g,
                                    ctx->saved_data.count("exact_t") > 0)) {
                auto alpha = torch::empty({slot(2 * li).cols.numel() * heads}, fopts(x));  // rebuild alpha
                gat_forward_launch(slot(2 * li), l, r, x, {}, {}, heads, slope, mode, alpha.data_ptr<float>(), nullptr);
                g = gat_backward(l, r, x, alpha, {}, grad_outputs[0], li, slope, mode, heads, {}, {});
            }
            return {g.daL.view_as(l), g.daR.view_as(r), g.dX, torch::Tensor(), torch::Tensor(), torch::Tensor()};
        }
        if (ctx->saved_data.count("stats")) {
            const GatStats o{sv[4], sv[3], sv[5], sv[6], r, sv[7]};
            if (!gat_backward_stats(l, o, grad_outputs[0], li, slope, heads, g) &&
                !gat_backward_recompute(l, r, x, o.q, grad_outputs[0], li, slope, heads, {}, {}, g)) {
                auto q = o.q.clone();  // rebuild the factored p (the forward writes the same q)
                auto alpha = torch::empty({slot(2 * li).cols.numel() * heads}, fopts(x));
                gat_forward_launch(slot(2 * li), l, r, x, {}, {}, heads, slope, mode, alpha.data_ptr<float>(),
                                   q.data_ptr<float>());
                g = gat_backward(l, r, x, alpha, q, grad_outputs[0], li, slope, mode, heads, {}, {});
            }
            return {g.daL.view_as(l), g.daR.view_as(r), g.dX, torch::Tensor(), torch::Tensor(), torch::Tensor()};
        }
        auto alpha = sv[3];
        torch::Tensor q = sv[4].numel() > 0 ? sv[4] : torch::Tensor();
        if (alpha.numel() == 0 && !gat_backward_recompute(l, r, x, q, grad_outputs[0], li, slope, heads, {}, {}, g)) {
            // the fused kernel does not take this shape: rebuild the factored p
            alpha = torch::empty({slot(2 * li).cols.numel() * heads}, fopts(x));
            gat_forward_launch(slot(2 * li), l, r, x, {}, {}, heads, slope, mode, alpha.data_ptr<float>(),
                               q.data_ptr<float>());
        }
        if (alpha.numel() > 0)
            g = gat_backward(l, r, x, alpha, q, grad_outputs[0], li, slope, mode, heads, {}, {});
        return {g.daL.view_as(l), g.daR.view_as(r), g.dX, torch::Tensor(), torch::Tensor(),
                torch::Tensor()};
    }
};

// The DSL's GAT layer (tests/GALA-DSL/gat/*: attnR = dsl.nn.ffn(res, out=1); ...;
// res = aggregate_fn(G.graphs, res)): the source logit is a Linear of the aggregated rows,
// so the kernels recompute aR[col] from the X row they gather instead of reading aR
// (gala_gat_{fwd,bwd}_ex_f32 with wR).  With H heads (the galac heads(H) extension) the
// Linear is per head: aR[j,h] = <X[j, hD:(h+1)D], wR[hD:(h+1)D]> + bR[h], wR of F
// elements, bR of H.  Its gradients follow from d_aR: d wR[head h] = sum_j d_aR[j,h]
// X[j, head h], d bR = sum d_aR, dX[:, head h] += d_aR[:, h] wR[head h].
struct GatAggregateFfn : public torch::autograd::Function<GatAggregateFfn> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor aL, torch::Tensor X,
                                 torch::Tensor wR, torch::Tensor bR, int64_t li, double slope,
                                 int64_t mode) {
        Slot s = slot(2 * li);
        auto l = aL.contiguous(), w = wR.contiguous();
        torch::Tensor b = bR.defined() && bR.numel() > 0 ? bR.contiguous() : torch::Tensor();
        const int64_t nrows = s.off.numel() / s.segs - 1;
        const int heads = (int)(l.numel() / std::max<int64_t>(nrows, 1));
        auto x = heads == 1 ? pad_rows4(X) : X.contiguous();
        check_dev(l, torch::kFloat, "attn_l");
        check_dev(x, torch::kFloat, "X");
        check_dev(w, torch::kFloat, "attn_r weight");
        const int64_t F = x.size(1);
        TORCH_CHECK(l.numel() == nrows * heads && w.numel() == F && F % heads == 0,
                    "gala: gat_aggregate_ffn: attn_l [N, H], attn_r weight of F = H*D elements");
        TORCH_CHECK(!b.defined() || b.numel() == heads, "gala: gat_aggregate_ffn: attn_r bias of H elements");
        check_on(l, s.off, "attn_l");
        check_on(x, s.off, "X");
        check_on(w, s.off, "attn_r weight");
        if (b.defined()) check_on(b, s.off, "attn_r bias");
        const bool recompute = recompute_attention(li, mode);
        const bool factored = mode == GALA_SOFTMAX_REF;
        ctx->saved_data["li"] = li;
        ctx->saved_data["slope"] = slope;
        ctx->saved_data["mode"] = mode;
        ctx->saved_data["heads"] = (int64_t)heads;
        ctx->saved_data["has_bias"] = b.defined();
        const torch::Tensor b_saved = b.defined() ? b : torch::empty({0}, fopts(x));
        GatStats o;
        const bool grad = ctx->needs_input_grad(0) || ctx->needs_input_grad(1) || ctx->needs_input_grad(2) ||
                          ctx->needs_input_grad(3);
        GatExact ex;
        const bool fixed_grad = mode == GALA_SOFTMAX_FIXED && grad;
        const bool symm = fixed_grad && exact_stats_layer(li, x.size(0));
        const bool directed = fixed_grad && !symm && exact_directed_layer(li, x.size(0));
        if ((symm || directed) &&
            gat_forward_exact(s, l, {}, x, w, b, heads, slope, ex)) {
            // ex.aR: the recomputed source logits, the backward's second operand of every logit
            ctx->saved_data["exact"] = true;
            if (directed) ctx->saved_data["exact_t"] = true;
            ctx->save_for_backward({l, x, w, b_saved, ex.aR, ex.lse, ex.Y, ex.Ym, ex.sma});
            return ex.Y;
        }
        if (recompute && grad && rowstats_enabled() && gat_forward_stats(s, l, {}, x, w, b, heads, slope, o)) {
            // o.aR: the recomputed source logits, read by the backward
            ctx->saved_data["stats"] = true;
            ctx->save_for_backward({l, x, w, b_saved, o.aR, o.q, o.Y, o.Ym, o.sma, o.p});
            return o.Y;
        }
        auto alpha = recompute ? torch::empty({0}, fopts(x)) : torch::empty({s.cols.numel() * heads}, fopts(x));
        auto q = factored ? torch::empty({nrows * heads}, fopts(x)) : torch::empty({0}, fopts(x));
        auto Y = gat_forward_launch(s, l, {}, x, w, b, heads, slope, mode,
                                    recompute ? nullptr : alpha.data_ptr<float>(),
                                    factored ? q.data_ptr<float>() : nullptr);
        ctx->save_for_backward({l, x, w, b_saved, alpha, q});
        return Y;
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        auto sv = ctx->get_saved_variables();
        auto l = sv[0], x = sv[1], w = sv[2], alpha = sv[4];
        const bool stats = ctx->saved_data.count("stats") > 0;
        const bool exact = ctx->saved_data.count("exact") > 0;   // sv[4..8] = aR, lse, Y, Ym, sma
        torch::Tensor q = stats ? sv[5] : ((!exact && sv[5].numel() > 0) ? sv[5] : torch::Tensor());
        const bool has_bias = ctx->saved_data["has_bias"].toBool();
        const int heads = (int)ctx->saved_data["heads"].toInt();
        const int64_t li = ctx->saved_data["li"].toInt(), mode = ctx->saved_data["mode"].toInt();
        const double slope = ctx->saved_data["slope"].toDouble();
        torch::Tensor b = has_bias ? sv[3] : torch::Tensor();
        GatGrads g;
        bool done = false, fused_linear = false;
        if (exact) {
            const GatExact ex{sv[6], sv[5], sv[7], sv[8], sv[4]};
            done = gat_backward_exact(l, ex, x, grad_outputs[0], li, slope, heads, g,
                                      ctx->saved_data.count("exact_t") > 0);
            alpha = torch::empty({0}, fopts(x));
            if (!done) {  // rebuild alpha for the alpha-storing backward
                alpha = torch::empty({slot(2 * li).cols.numel() * heads}, fopts(x));
                gat_forward_launch(slot(2 * li), l, {}, x, w, b, heads, slope, mode, alpha.data_ptr<float>(), nullptr);
            }
        }
        if (stats) {
            const GatStats o{sv[6], q, sv[7], sv[8], sv[4], sv[9]};
            // several heads: the Linear's dX term goes into the kernel's dX store
            fused_linear = heads > 1;
            done = gat_backward_stats(l, o, grad_outputs[0], li, slope, heads, g,
                                      fused_linear ? w.contiguous() : torch::Tensor());
            fused_linear = fused_linear && done;
            alpha = torch::empty({0}, fopts(x));  // otherwise: the recomputed path below
        }
        if (!done && !exact && alpha.numel() == 0 && !gat_backward_recompute(l, {}, x, q, grad_outputs[0], li, slope, heads, w, b, g)) {
            if (stats) q = q.clone();
            alpha = torch::empty({slot(2 * li).cols.numel() * heads}, fopts(x));
            gat_forward_launch(slot(2 * li), l, {}, x, w, b, heads, slope, mode, alpha.data_ptr<float>(),
                               q.data_ptr<float>());
        }
        if (alpha.numel() > 0) g = gat_backward(l, {}, x, alpha, q, grad_outputs[0], li, slope, mode, heads, w, b);
        const int64_t N = x.size(0);
        const int32_t F = (int32_t)x.size(1);
        torch::Tensor dW, db;
        if (heads == 1) {
            auto daR = g.daR.reshape({-1, 1}).contiguous();
            dW = torch::empty({1, F}, fopts(x));
            db = torch::empty({1}, fopts(x));
            const Backend &B = be(x);
            const int64_t wsb = B.dense_ws(N, F, 1);
            TORCH_CHECK(wsb >= 0, "gala: gala_dense_grad_workspace failed");
            auto ws = torch::empty({std::max<int64_t>(wsb / 4, 1)}, fopts(x));
            check(B.dense_grad(N, F, 1, x.data_ptr<float>(), x.stride(0), daR.data_ptr<float>(), 1,
                               dW.data_ptr<float>(), db.data_ptr<float>(), 0, ws.data_ptr<float>(),
                               wsb, stream_of(x)),
                  "gala_dense_grad_f32");
            g.dX.addr_(daR.reshape({-1}), w.reshape({-1}));  // through aR = X wR^T + bR
        } else {  // per head: the block-diagonal Linear
            auto daR = g.daR.reshape({N, heads}).contiguous();
            head_linear_grads(x, daR, w, heads, dW, db);
            if (!fused_linear)
                check(be(x).head_attn_bwd(N, F, heads, daR.data_ptr<float>(), w.data_ptr<float>(),
                                          g.dX.data_ptr<float>(), g.dX.stride(0), 1, stream_of(x)),
                      "gala_head_attn_bwd_f32");  // dX[:, head h] += d_aR[:, h] wR[head h]
        }
        return {g.daL.view_as(l), g.dX, dW.view_as(w), has_bias ? db.view_as(b) : torch::Tensor(),
                torch::Tensor(), torch::Tensor(), torch::Tensor()};
    }
};

// post * A (pre * X) with autograd: the ROW_BROADCAST / AGGREGATE / ROW_BROADCAST chain
// of a GCN layer (or of SAGE's mean, pre undefined) as one op.  Backward is the same
// chain on slot 2li+1: pre * A_b (post * dY), which is what autograd through the
// reference's unfused ops computes (torch mul, <K>_AutoGrad::backward, torch mul), with
// the same roundings.
struct GcnAggregate : public torch::autograd::Function<GcnAggregate> {
    static torch::Tensor run(const torch::Tensor &X, const torch::Tensor &pre,
                             const torch::Tensor &post, const Slot &s) {
        auto &S = global_slots();
        const bool has_pre = pre.numel() > 0, has_post = post.numel() > 0;
        // pre * X: on short rows (< 8 edges per row on average, config 5) as the SpMM's source
        // scale (fl(pre[c] * X[c]) per gathered element: the ROW_BROADCAST's roundings without
        // its pass over [N, F], 2.3 ms at 11 M x 128), else the pass
        const int64_t n = X.size(0) > 0 ? X.size(0) : 1;
        const bool fold = has_pre && S.nsamples == 0 && s.cols.numel() < 8 * n;
        torch::Tensor xs = has_pre && !fold ? row_broadcast(pre, X) : X.contiguous();
        return spmm_impl(xs, s.off, s.cols, s.weighted ? &s.vals : nullptr, s.bounds, s.segs, 1,
                         fold ? &pre : nullptr, has_post ? &post : nullptr, S.nsamples, S.ra, S.rb);
    }
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor X, torch::Tensor pre,
                                 torch::Tensor post, int64_t li) {
        ctx->saved_data["li"] = li;
        ctx->saved_data["pre"] = pre.detach();
        ctx->saved_data["post"] = post.detach();
        return run(X, pre, post, slot(2 * li));
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        const int64_t li = ctx->saved_data["li"].toInt();
        auto pre = ctx->saved_data["pre"].toTensor();
        auto post = ctx->saved_data["post"].toTensor();
        return {run(grad_outputs[0], post, pre, slot(2 * li + 1)), torch::Tensor(),
                torch::Tensor(), torch::Tensor()};
    }
};

// pre * relu(act * X) (gala_row_scale_relu_f32) and its backward (undefined factors: 1)
torch::Tensor scale_relu(const torch::Tensor &X, const torch::Tensor &act, const torch::Tensor &pre) {
    auto x = X.contiguous();
    check_dev(x, torch::kFloat, "X");
    const int64_t n = x.size(0), F = x.numel() / std::max<int64_t>(n, 1);
    torch::Tensor a = act.defined() ? act.contiguous() : torch::Tensor();
    torch::Tensor p = pre.defined() ? pre.contiguous() : torch::Tensor();
    if (a.defined()) check_on(a, x, "act");
    if (p.defined()) check_on(p, x, "pre");
    auto out = torch::empty_like(x);
    check(be(x).scale_relu(n, (int32_t)F, a.defined() ? a.data_ptr<float>() : nullptr,
                           p.defined() ? p.data_ptr<float>() : nullptr, x.data_ptr<float>(), F,
                           out.data_ptr<float>(), F, stream_of(x)),
          "gala_row_scale_relu_f32");
    return out;
}

torch::Tensor relu_scale_backward(const torch::Tensor &act, const torch::Tensor &X,
                                  const torch::Tensor &G) {
    auto x = X.contiguous(), g = G.contiguous();
    check_dev(g, torch::kFloat, "grad");
    check_on(g, x, "grad");
    const int64_t n = x.size(0), F = x.numel() / std::max<int64_t>(n, 1);
    torch::Tensor a = act.defined() ? act.contiguous() : torch::Tensor();
    auto dx = torch::empty_like(x);
    check(be(x).relu_bwd(n, (int32_t)F, a.defined() ? a.data_ptr<float>() : nullptr,
                         x.data_ptr<float>(), F, g.data_ptr<float>(), F, dx.data_ptr<float>(), F,
                         stream_of(x)),
          "gala_relu_scale_backward_f32");
    return dx;
}

// post * A (pre * relu(act * X)): the next layer's ReLU (and the row broadcast in front of
// it) fused into the elementwise pass the aggregation needs anyway.  Backward: the
// aggregation's backward gives G = pre * A_b (post * dY) (the gradient of relu(act * X)),
// then one pass forms act * (relu(act * X) <= 0 ? 0 : G) -- the roundings of torch's
// threshold_backward and mul backward.
struct GcnAggregateRelu : public torch::autograd::Function<GcnAggregateRelu> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor X, torch::Tensor act,
                                 torch::Tensor pre, torch::Tensor post, int64_t li) {
        auto &S = global_slots();
        Slot s = slot(2 * li);
        const bool has_act = act.numel() > 0, has_pre = pre.numel() > 0, has_post = post.numel() > 0;
        auto x = X.contiguous();
        ctx->save_for_backward({x});
        ctx->saved_data["li"] = li;
        ctx->saved_data["act"] = act.detach();
        ctx->saved_data["pre"] = pre.detach();
        ctx->saved_data["post"] = post.detach();
        // on short rows (< 8 edges per row on average, config 5) the SpMM forms
        // pre[c] * relu(act[c] * X[c]) per gathered element (its ReLU prologue, the pass's
        // roundings) instead of the pass over [N, F]; on long rows the pass is cheaper than two
        // factor loads per edge
        const int64_t n = x.size(0) > 0 ? x.size(0) : 1;
        if (s.cols.numel() < 8 * n) {
            torch::Tensor a = has_act ? act.contiguous() : torch::Tensor();
            if (has_act) {
                check_dev(a, torch::kFloat, "act");
                check_on(a, x, "act");
                TORCH_CHECK(a.numel() == x.size(0), "gala: act holds one factor per row");
            }
            gala_spmm_epilogue_t epi{};
            epi.src_relu = 1;
            epi.src_act = has_act ? a.data_ptr<float>() : nullptr;
            auto y = spmm_impl(x, s.off, s.cols, s.weighted ? &s.vals : nullptr, s.bounds, s.segs, 1,
                               has_pre ? &pre : nullptr, has_post ? &post : nullptr, S.nsamples, S.ra, S.rb,
                               nullptr, &epi);
            if (y.defined()) return y;
        }
        auto xs = scale_relu(x, has_act ? act : torch::Tensor(), has_pre ? pre : torch::Tensor());
        return spmm_impl(xs, s.off, s.cols, s.weighted ? &s.vals : nullptr, s.bounds, s.segs, 1,
                         nullptr, has_post ? &post : nullptr, S.nsamples, S.ra, S.rb);
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        const int64_t li = ctx->saved_data["li"].toInt();
        auto act = ctx->saved_data["act"].toTensor();
        auto pre = ctx->saved_data["pre"].toTensor();
        auto post = ctx->saved_data["post"].toTensor();
        auto x = ctx->get_saved_variables()[0];
        auto &S = global_slots();
        Slot b = slot(2 * li + 1);
        // post * dY: on short rows (< 8 edges per row on average, config 5) as the SpMM's
        // source scale -- fl(post[c] * dY[c]) per gathered element, the ROW_BROADCAST pass's
        // roundings without its pass over [N, F]; on long rows the pass is cheaper than a
        // scale load per edge
        const bool has_post = post.numel() > 0;
        const bool fold = has_post && b.cols.numel() < 8 * (x.size(0) > 0 ? x.size(0) : 1);
        torch::Tensor dys = has_post && !fold ? row_broadcast(post, grad_outputs[0]) : grad_outputs[0].contiguous();
        // the ReLU backward as the SpMM's epilogue: act * (relu(act * x) <= 0 ? 0 : G) on the
        // row in registers, without G's round trip through HBM
        torch::Tensor a = act.numel() > 0 ? act.contiguous() : torch::Tensor();
        gala_spmm_epilogue_t epi{};
        epi.relu_x = x.data_ptr<float>();
        epi.ldrx = x.size(0) > 0 ? x.numel() / x.size(0) : 0;
        epi.relu_act = a.defined() ? a.data_ptr<float>() : nullptr;
        auto dx = spmm_impl(dys, b.off, b.cols, b.weighted ? &b.vals : nullptr, b.bounds, b.segs, 1,
                            fold ? &post : nullptr, pre.numel() > 0 ? &pre : nullptr, S.nsamples, S.ra, S.rb,
                            nullptr, &epi);
        if (!dx.defined()) {
            auto G = spmm_impl(dys, b.off, b.cols, b.weighted ? &b.vals : nullptr, b.bounds, b.segs, 1,
                               fold ? &post : nullptr, pre.numel() > 0 ? &pre : nullptr, S.nsamples, S.ra, S.rb);
            dx = relu_scale_backward(act.numel() > 0 ? act : torch::Tensor(), x, G);
        }
        return {dx, torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
    }
};

// X W^T (+ b) for one Linear: on gala_ffn_fwd_f32 where it beats the library GEMM on this
// chip -- a GPU operand with 33..64 outputs from at most 64 inputs (Products' 32 -> 47:
// 0.28 vs 0.44 ms, tools/dense_bench.py) -- else at::addmm.
torch::Tensor linear_fwd(const torch::Tensor &X, const torch::Tensor &W, const torch::Tensor &b) {
    const bool has_b = b.defined() && b.numel() > 0;
    const int64_t K = W.size(1), M = W.size(0);
    // the matrix-core kernel takes K and M from W and reads X rows / the bias on faith:
    // every operand shape and device is checked here (mismatches go to at::addmm, which
    // raises its usual shape error)
    const bool shapes_ok = X.dim() == 2 && W.dim() == 2 && X.size(1) == K && W.device() == X.device() &&
                           W.scalar_type() == torch::kFloat &&
                           (!has_b || (b.numel() == M && b.device() == X.device() && b.scalar_type() == torch::kFloat));
    if (shapes_ok && X.is_cuda() && X.scalar_type() == torch::kFloat && X.stride(1) == 1 &&
        M > 32 && M <= 64 && K <= 64) {
        auto w = W.contiguous();
        torch::Tensor bb = has_b ? b.contiguous() : torch::Tensor();
        auto Y = torch::empty({X.size(0), M}, fopts(X));
        const int st = be(X).ffn_fwd(X.size(0), (int32_t)K, (int32_t)M, X.data_ptr<float>(),
                                     std::max<int64_t>(X.stride(0), K), w.data_ptr<float>(),
                                     has_b ? bb.data_ptr<float>() : nullptr, Y.data_ptr<float>(), M,
                                     stream_of(X));
        if (st != GALA_ERR_UNSUPPORTED) {
            check(st, "gala_ffn_fwd_f32");
            return Y;
        }
    }
    return has_b ? torch::addmm(b, X, W.t()) : X.mm(W.t());
}

// FFN_OP: forward linear_fwd (matrix cores for the narrow widths, else at::addmm); weight /
// bias gradients on gala_dense_grad_f32 (split over rows); dX = dY W through linear_fwd
// with W^T.
struct Ffn : public torch::autograd::Function<Ffn> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor X, torch::Tensor weight,
                                 torch::Tensor bias) {
        ctx->save_for_backward({X, weight});
        ctx->saved_data["has_bias"] = bias.defined() && bias.numel() > 0;
        return linear_fwd(X, weight, bias);
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        auto sv = ctx->get_saved_variables();
        torch::Tensor X = sv[0].contiguous(), W = sv[1];
        torch::Tensor dY = grad_outputs[0].contiguous();
        const bool has_bias = ctx->saved_data["has_bias"].toBool();
        torch::Tensor dX = ctx->needs_input_grad(0) ? linear_fwd(dY, W.t(), torch::Tensor()) : torch::Tensor();
        check_dev(X, torch::kFloat, "X");
        check_dev(dY, torch::kFloat, "dY");
        const int64_t N = X.size(0);
        const int32_t K = (int32_t)X.size(1), M = (int32_t)dY.size(1);
        auto dW = torch::empty({M, K}, fopts(X));
        torch::Tensor db = has_bias ? torch::empty({M}, fopts(X)) : torch::Tensor();
        check_on(dY, X, "dY");
        const Backend &B = be(X);
        const int64_t wsb = B.dense_ws(N, K, M);
        TORCH_CHECK(wsb >= 0, "gala: gala_dense_grad_workspace failed");
        auto ws = torch::empty({std::max<int64_t>(wsb / 4, 1)}, fopts(X));
        check(B.dense_grad(N, K, M, X.data_ptr<float>(), K, dY.data_ptr<float>(), M,
                           dW.data_ptr<float>(), has_bias ? db.data_ptr<float>() : nullptr, 0,
                           ws.data_ptr<float>(), wsb, stream_of(X)),
              "gala_dense_grad_f32");
        return {dX, dW, db};
    }
};

}  // namespace

torch::Tensor ffn_apply(torch::Tensor X, torch::Tensor weight, torch::Tensor bias) {
    return Ffn::apply(X, weight, bias.defined() ? bias : torch::empty({0}, weight.options()));
}

torch::Tensor gcn_aggregate_apply(torch::Tensor X, torch::Tensor pre, torch::Tensor post,
                                  int64_t li) {
    // autograd::Function::apply needs defined tensors: an absent scale travels as a
    // zero-element tensor
    auto absent = [&](const torch::Tensor &t) {
        return t.defined() ? t : torch::empty({0}, X.options().requires_grad(false));
    };
    return GcnAggregate::apply(X, absent(pre), absent(post), li);
}

torch::Tensor gcn_aggregate_relu_apply(torch::Tensor X, torch::Tensor act, torch::Tensor pre,
                                       torch::Tensor post, int64_t li) {
    auto absent = [&](const torch::Tensor &t) {
        return t.defined() ? t : torch::empty({0}, X.options().requires_grad(false));
    };
    return GcnAggregateRelu::apply(X, absent(act), absent(pre), absent(post), li);
}

torch::Tensor aggregate_node_mul_sum_apply(torch::Tensor input_dense, int64_t li) {
    return AggregateNodeMulSum::apply(input_dense, li);
}
torch::Tensor aggregate_node_mul_sum_attn_apply(torch::Tensor input_dense,
                                                torch::Tensor value_graph, int64_t li) {
    return AggregateNodeMulSumAttn::apply(input_dense, value_graph, li);
}
torch::Tensor aggregate_edge_sum_apply(torch::Tensor input_dense1, torch::Tensor input_dense2,
                                       int64_t li) {
    return AggregateEdgeSum::apply(input_dense1, input_dense2, li);
}
torch::Tensor non_lnr_op_softmax_apply(torch::Tensor value_graph, int64_t li) {
    return NonLnrOpSoftmax::apply(value_graph, li);
}
torch::Tensor gat_aggregate_apply(torch::Tensor attn_l, torch::Tensor attn_r, torch::Tensor X,
                                  int64_t li, double slope, int64_t mode) {
    return GatAggregate::apply(attn_l, attn_r, X, li, slope, mode);
}

torch::Tensor gat_aggregate_ffn_apply(torch::Tensor attn_l, torch::Tensor X, torch::Tensor attn_r_weight,
                                      torch::Tensor attn_r_bias, int64_t li, double slope,
                                      int64_t mode) {
    return GatAggregateFfn::apply(attn_l, X, attn_r_weight, attn_r_bias, li, slope, mode);
}

// The multi-head GAT layer in input space (gala_gat_in_*, include/gala_hip.h): the chain
// ffn_apply(X, W, b) -> head_attn_apply(., wL, bL) -> gat_aggregate_ffn_apply(., ., wR, bR)
// as one autograd op whose kernels gather X's fin-float rows instead of the H*D-float Linear
// output.  Forward: the attention vectors folded through the Linear (uL_h = W_h^T wL_h, cL_h
// = b_h . wL_h + bL_h; the same for R), the extended rows, the aggregation with the
// projection in its epilogue.  Backward (REF, the reference's chain on the undirected
// graph): d_aL and M = sum_r dX[r]^T X_ext[r] from the kernel, G = d_aL^T X_ext from the
// dense gradient kernel, then
//   dW_h = M_h[:, :fin] + (wL_h + wR_h) G_h,   db_h = M_h[:, fin] + (wL_h + wR_h) sum d_aL_h
//   d wL_h = d wR_h = W_h G_h + b_h sum d_aL_h,  d bL = d bR = sum d_aL   (REF: d aR = d aL)
// -- exactly the gradients autograd forms through the three ops (Ffn, HeadAttnFn,
// GatAggregateFfn), regrouped.  X itself gets no gradient (the layer's input is the
// dataset's features); the apply wrapper keeps the three-op chain whenever X needs one.
const PatternT &transposed_pattern(int64_t idx);
bool gat_in_tmode_enabled();
int64_t gat_in_tmode_max_bytes();

struct GatInputLayer : public torch::autograd::Function<GatInputLayer> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor X, torch::Tensor W, torch::Tensor b,
                                 torch::Tensor wL, torch::Tensor bL, torch::Tensor wR, torch::Tensor bR,
                                 int64_t li, double slope, int64_t heads, bool relu) {
        Slot s = slot(2 * li);
        auto x = X.contiguous(), w = W.contiguous();
        const bool has_b = b.defined() && b.numel() > 0;
        check_dev(x, torch::kFloat, "X");
        check_dev(w, torch::kFloat, "weight");
        check_on(x, s.off, "X");
        check_on(w, s.off, "weight");
        const int64_t N = x.size(0), fin = x.size(1), F = w.size(0), H = heads, D = F / H;
        TORCH_CHECK(w.size(1) == fin && F % H == 0 && wL.numel() == F && wR.numel() == F && bL.numel() == H &&
                        bR.numel() == H && (!has_b || b.numel() == F),
                    "gala: gat_input_layer: X [N, fin], W [H*D, fin], b [H*D], attention vectors [H*D] and biases [H]");
        auto w3 = w.view({H, D, fin});
        auto bb = has_b ? b.contiguous().view({H, D}) : torch::zeros({H, D}, fopts(x));
        auto uL = (w3 * wL.reshape({H, D, 1})).sum(1), uR = (w3 * wR.reshape({H, D, 1})).sum(1);
        auto cL = (bb * wL.reshape({H, D})).sum(1) + bL.reshape({H}), cR = (bb * wR.reshape({H, D})).sum(1) + bR.reshape({H});
        auto u = torch::cat({uL, uR}).contiguous(), c = torch::cat({cL, cR}).contiguous();
        auto xext = torch::empty({N, 128}, fopts(x));
        const Backend &B = be(x);
        check(B.gat_in_prep(N, (int32_t)fin, x.data_ptr<float>(), x.stride(0), (int32_t)H, u.data_ptr<float>(),
                            c.data_ptr<float>(), xext.data_ptr<float>(), stream_of(x)),
              "gala_gat_in_prep_f32");
        CsrView cv = view(s.off, s.cols, nullptr, s.bounds, s.segs);
        auto Y = torch::empty({N, F}, fopts(x)), Ym = torch::empty({N, F}, fopts(x));
        auto q = torch::empty({N, H}, fopts(x)), sma = torch::empty({N, H}, fopts(x));
        torch::Tensor bc = has_b ? b.contiguous() : torch::Tensor();
        const PatternT &pt = transposed_pattern(2 * li);
        // T mode (GPU, symmetric pattern, gradients wanted): the forward also forms the
        // backward's per-column aggregates, so the backward does not walk the graph again
        const bool grad = ctx->needs_input_grad(1) || ctx->needs_input_grad(2) || ctx->needs_input_grad(3) ||
                          ctx->needs_input_grad(4) || ctx->needs_input_grad(5) || ctx->needs_input_grad(6);
        // T holds 3.5 KB per row until the backward: within gat_in_tmode_max_bytes() (the walk
        // otherwise: e.g. papers100M's 111 M rows would need 389 GB)
        const bool tmode = grad && B.gat_in_fwd_t && pt.symmetric && gat_in_tmode_enabled() &&
                           N * 896 * (int64_t)sizeof(float) <= gat_in_tmode_max_bytes();
        torch::Tensor T = tmode ? torch::empty({N, 896}, fopts(x)) : torch::empty({0}, fopts(x));
        // hub rows: the pre-pass's chunk tiles live in the plan's workspace
        with_workspace(cv, s.off, gala_gat_in_split_ws_cols(tmode ? GALA_GAT_IN_WS_FWD_T : GALA_GAT_IN_WS_FWD));
        if (tmode)
            check(B.gat_in_fwd_t(&cv.c, pt.order.data_ptr<int32_t>(), (int32_t)fin, (int32_t)H, (int32_t)D, (float)slope,
                                 xext.data_ptr<float>(), w.data_ptr<float>(), fin, has_b ? bc.data_ptr<float>() : nullptr,
                                 Y.data_ptr<float>(), Ym.data_ptr<float>(), F, q.data_ptr<float>(), sma.data_ptr<float>(),
                                 relu ? GALA_GAT_IN_RELU : 0, T.data_ptr<float>(), stream_of(x)),
                  "gala_gat_in_fwd_t_f32");
        else
            check(B.gat_in_fwd(&cv.c, pt.order.data_ptr<int32_t>(), (int32_t)fin, (int32_t)H, (int32_t)D, (float)slope, xext.data_ptr<float>(),
                               w.data_ptr<float>(), fin, has_b ? bc.data_ptr<float>() : nullptr, Y.data_ptr<float>(),
                               Ym.data_ptr<float>(), F, q.data_ptr<float>(), sma.data_ptr<float>(),
                               relu ? GALA_GAT_IN_RELU : 0, stream_of(x)),
                  "gala_gat_in_fwd_f32");
        ctx->saved_data["li"] = li;
        ctx->saved_data["slope"] = slope;
        ctx->saved_data["heads"] = heads;
        ctx->saved_data["has_b"] = has_b;
        ctx->saved_data["relu"] = relu;
        ctx->save_for_backward({x, w, has_b ? bc : torch::empty({0}, fopts(x)), wL, wR, xext, Y, Ym, sma, T});
        return Y;
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        auto sv = ctx->get_saved_variables();
        auto x = sv[0], w = sv[1], b = sv[2], wL = sv[3], wR = sv[4], xext = sv[5], Y = sv[6], Ym = sv[7], sma = sv[8],
             T = sv[9];
        const int64_t li = ctx->saved_data["li"].toInt(), H = ctx->saved_data["heads"].toInt();
        const double slope = ctx->saved_data["slope"].toDouble();
        const bool has_b = ctx->saved_data["has_b"].toBool(), relu = ctx->saved_data["relu"].toBool();
        const int64_t N = x.size(0), fin = x.size(1), F = w.size(0), D = F / H;
        auto dY = grad_outputs[0].contiguous();
        check_dev(dY, torch::kFloat, "grad");
        check_on(dY, x, "grad");
        // the backward reads dY rows as float4: a contiguous grad at a storage offset that is
        // not 16-byte aligned (a view into a larger buffer) is copied to a fresh allocation
        if (reinterpret_cast<uintptr_t>(dY.data_ptr<float>()) & 15) dY = dY.clone();
        // the reference's REF backward on the undirected graph is dX = A_alpha dY over A itself;
        // regrouped by column it walks A's transposed pattern (A's own tensors when symmetric)
        const PatternT &pt = transposed_pattern(2 * li);
        CsrView cv = view(pt.rowptr, pt.col, nullptr, torch::Tensor(), 1);
        if (T.numel() == 0) {   // the walk: the transposed pattern's hub-row plan with its workspace
            const int64_t cols = gala_gat_in_split_ws_cols(GALA_GAT_IN_WS_BWD);
            if (pt.split) {     // (a non-symmetric pattern's transpose is in no slot)
                if (pt.split->plan.n_rows_split > 0) pt.split->ensure_workspace(cols);
                cv.c.split = &pt.split->plan;
            } else {
                with_workspace(cv, pt.rowptr, cols);
            }
        }
        const Backend &B = be(x);
        auto daL = torch::empty({N, H}, fopts(x));
        auto M = torch::empty({H, D, fin + 1}, fopts(x));
        const int64_t wsb = B.gat_in_ws((int32_t)H);
        TORCH_CHECK(wsb > 0, "gala: gala_gat_in_bwd_workspace failed");
        auto ws = torch::empty({wsb / 4}, fopts(x));
        if (T.numel() > 0)   // T mode: the forward's per-column aggregates
            check(B.gat_in_bwd_t(N, pt.order_t.data_ptr<int32_t>(), (int32_t)fin, (int32_t)H, (int32_t)D,
                                 T.data_ptr<float>(), dY.data_ptr<float>(), Y.data_ptr<float>(), Ym.data_ptr<float>(), F,
                                 sma.data_ptr<float>(), daL.data_ptr<float>(), M.data_ptr<float>(), ws.data_ptr<float>(),
                                 wsb, relu ? GALA_GAT_IN_RELU : 0, stream_of(x)),
                  "gala_gat_in_bwd_t_f32");
        else
            check(B.gat_in_bwd(&cv.c, pt.order_t.data_ptr<int32_t>(), (int32_t)fin, (int32_t)H, (int32_t)D, (float)slope, xext.data_ptr<float>(),
                               dY.data_ptr<float>(), Y.data_ptr<float>(), Ym.data_ptr<float>(), F, sma.data_ptr<float>(),
                               daL.data_ptr<float>(), M.data_ptr<float>(), ws.data_ptr<float>(), wsb,
                               relu ? GALA_GAT_IN_RELU : 0, stream_of(x)),
                  "gala_gat_in_bwd_f32");
        // G = d_aL^T X (and its column sums): the attention Linears' terms
        auto Gw = torch::empty({H, fin}, fopts(x)), Gb = torch::empty({H}, fopts(x));
        const int64_t gws = B.dense_ws(N, (int32_t)fin, (int32_t)H);
        TORCH_CHECK(gws >= 0, "gala: gala_dense_grad_workspace failed");
        auto gw = torch::empty({std::max<int64_t>(gws / 4, 1)}, fopts(x));
        check(B.dense_grad(N, (int32_t)fin, (int32_t)H, x.data_ptr<float>(), x.stride(0), daL.data_ptr<float>(), H,
                           Gw.data_ptr<float>(), Gb.data_ptr<float>(), 0, gw.data_ptr<float>(), gws, stream_of(x)),
              "gala_dense_grad_f32");
        auto sLR = (wL.reshape({H, D}) + wR.reshape({H, D}));
        auto dW = (M.narrow(2, 0, fin) + sLR.unsqueeze(2) * Gw.unsqueeze(1)).reshape({F, fin});
        torch::Tensor db = has_b ? (M.select(2, fin) + sLR * Gb.unsqueeze(1)).reshape({F}) : torch::Tensor();
        auto bb = has_b ? b.view({H, D}) : torch::zeros({H, D}, fopts(x));
        auto dw = ((w.view({H, D, fin}) * Gw.unsqueeze(1)).sum(2) + bb * Gb.unsqueeze(1));
        return {torch::Tensor(), dW, db, dw.reshape(wL.sizes()), Gb.reshape({H}), dw.reshape(wR.sizes()),
                Gb.reshape({H}), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
    }
};

// slot idx's transposed pattern (one segment): a host transpose on first use
// (gala_host_csr_transpose), compared with the pattern itself; kept on the graph's device
const PatternT &transposed_pattern(int64_t idx) {
    auto &S = global_slots();
    auto &pt = S.pattern_t[idx];
    if (pt) return *pt;
    for (size_t i = 0; i < S.pattern_t.size(); ++i)
        if (S.pattern_t[i] && S.offset_graph[i].unsafeGetTensorImpl() == S.offset_graph[idx].unsafeGetTensorImpl() &&
            S.columns_graph[i].unsafeGetTensorImpl() == S.columns_graph[idx].unsafeGetTensorImpl()) {
            pt = S.pattern_t[i];
            return *pt;
        }
    TORCH_CHECK(S.segments[idx] == 1, "gala: transposed pattern of a column-tiled graph");
    auto off = S.offset_graph[idx].to(torch::kCPU).contiguous(), col = S.columns_graph[idx].to(torch::kCPU).contiguous();
    const int64_t n = off.numel() - 1, nnz = col.numel();
    auto io = torch::TensorOptions().dtype(torch::kInt);
    auto tr = torch::empty({n + 1}, io), tc = torch::empty({nnz}, io), perm = torch::empty({nnz}, io);
    check(gala_host_csr_transpose(n, n, off.data_ptr<int32_t>(), col.data_ptr<int32_t>(), tr.data_ptr<int32_t>(),
                                  tc.data_ptr<int32_t>(), perm.data_ptr<int32_t>()),
          "gala_host_csr_transpose");
    auto p = std::make_shared<PatternT>();
    p->symmetric = torch::equal(tr, off) && torch::equal(tc, col);
    const auto dev = S.offset_graph[idx].device();
    auto ord = torch::empty({n}, io);
    check(gala_host_row_order(n, off.data_ptr<int32_t>(), ord.data_ptr<int32_t>()), "gala_host_row_order");
    p->order = ord.to(dev);
    if (p->symmetric) {
        p->rowptr = S.offset_graph[idx];
        p->col = S.columns_graph[idx];
        p->order_t = p->order;
    } else {
        p->rowptr = tr.to(dev);
        p->col = tc.to(dev);
        auto ot = torch::empty({n}, io);
        check(gala_host_row_order(n, tr.data_ptr<int32_t>(), ot.data_ptr<int32_t>()), "gala_host_row_order");
        p->order_t = ot.to(dev);
        // the transposed rowptr is in no slot: its hub-row plan is kept here
        if (dev.is_cuda()) p->split = make_split_plan(p->rowptr, 1);
    }
    pt = p;
    return *pt;
}

// GALA_GAT_IN_T=0 keeps the backward's own walk over the pattern (A/B runs)
bool gat_in_tmode_enabled() {
    static const bool on = [] {
        const char *e = std::getenv("GALA_GAT_IN_T");
        return !(e && e[0] == '0');
    }();
    return on;
}

// GALA_GAT_IN_T_MAX_GB (default 64): the largest T buffer T mode may hold between the forward
// and the backward
int64_t gat_in_tmode_max_bytes() {
    static const int64_t cap = [] {
        const char *e = std::getenv("GALA_GAT_IN_T_MAX_GB");
        const double gb = e ? std::atof(e) : 64.0;
        return (int64_t)(gb * 1073741824.0);
    }();
    return cap;
}

// GALA_GAT_INPUT=0 keeps the three-op chain (A/B runs, the tests' reference spelling)
bool gat_input_enabled() {
    static const bool on = [] {
        const char *e = std::getenv("GALA_GAT_INPUT");
        return !(e && e[0] == '0');
    }();
    return on;
}

HeadAttnImpl::HeadAttnImpl(int64_t in, int64_t heads) {
    TORCH_CHECK(heads >= 1 && in % heads == 0, "gala: HeadAttn(", in, ", ", heads, "): in is not a whole number of heads");
    const double bound = 1.0 / std::sqrt((double)(in / heads));  // torch Linear(D, 1) init range
    weight = register_parameter("weight", torch::empty({1, in}).uniform_(-bound, bound));
    bias = register_parameter("bias", torch::empty({heads}).uniform_(-bound, bound));
}

// The per-head attention Linear (gala_head_attn_f32 forward; backward: dX by
// gala_head_attn_bwd_f32, dW / db by the dense gradient kernel).
struct HeadAttnFn : public torch::autograd::Function<HeadAttnFn> {
    static torch::Tensor forward(AutogradContext *ctx, torch::Tensor X, torch::Tensor weight, torch::Tensor bias) {
        auto x = X.contiguous(), w = weight.contiguous(), b = bias.contiguous();
        const int64_t H = b.numel(), F = w.numel(), N = x.size(0);
        check_dev(x, torch::kFloat, "X");
        check_dev(w, torch::kFloat, "attention weight");
        check_dev(b, torch::kFloat, "attention bias");
        TORCH_CHECK(w.device() == x.device() && b.device() == x.device(), "gala: head_attn_apply: operands on ",
                    x.device(), ", ", w.device(), ", ", b.device());
        auto out = torch::empty({N, H}, fopts(x));
        check(be(x).head_attn(N, (int32_t)F, (int32_t)H, x.data_ptr<float>(), x.stride(0), w.data_ptr<float>(),
                              b.data_ptr<float>(), out.data_ptr<float>(), stream_of(x)),
              "gala_head_attn_f32");
        ctx->save_for_backward({x, w});
        ctx->saved_data["heads"] = H;
        return out;
    }
    static tensor_list backward(AutogradContext *ctx, tensor_list grad_outputs) {
        auto sv = ctx->get_saved_variables();
        auto x = sv[0], w = sv[1];
        const int heads = (int)ctx->saved_data["heads"].toInt();
        const int64_t N = x.size(0);
        const int32_t F = (int32_t)x.size(1);
        auto g = grad_outputs[0].contiguous();
        auto dX = torch::empty({N, F}, fopts(x));
        check(be(x).head_attn_bwd(N, F, heads, g.data_ptr<float>(), w.data_ptr<float>(), dX.data_ptr<float>(),
                                  dX.stride(0), 0, stream_of(x)),
              "gala_head_attn_bwd_f32");
        torch::Tensor dW, db;
        head_linear_grads(x, g, w, heads, dW, db);
        return {dX, dW, db};
    }
};

torch::Tensor head_attn_apply(torch::Tensor X, torch::Tensor weight, torch::Tensor bias) {
    const int64_t H = bias.numel(), F = weight.numel();
    TORCH_CHECK(X.dim() == 2 && X.size(-1) == F && F % H == 0, "gala: head_attn_apply: X has ", X.size(-1),
                " columns, the attention vectors ", F);
    return HeadAttnFn::apply(X, weight, bias);
}

bool gat_input_layer_eligible(const torch::Tensor &X, const torch::Tensor &W, int64_t li, int64_t heads,
                              int64_t mode) {
    if (!gat_input_enabled() || mode != GALA_SOFTMAX_REF || X.requires_grad() || X.dim() != 2 || W.dim() != 2)
        return false;
    if (X.scalar_type() != torch::kFloat || W.scalar_type() != torch::kFloat || X.device() != W.device()) return false;
    const int64_t fin = X.size(1), F = W.size(0);
    if (heads < 1 || heads > 8 || F % heads != 0 || W.size(1) != fin || fin < 1 || fin > 100) return false;
    const int64_t D = F / heads;
    if (!(D == 4 || D == 8 || D == 16 || D == 32)) return false;
    // the byte saving is the point: the input row narrower than the Linear's output
    if (fin >= F) return false;
    // REF on the undirected graph (slot 2li+1 = slot 2li, the reference's A-not-A^T backward
    // then equals the transposed regrouping), one segment; hub rows run as chunk partials
    // (make_split_plan's 512-edge chunks meet the kernels' multiple-of-64 contract)
    Slot s = slot(2 * li);
    if (!recompute_attention(li, mode) || s.segs != 1 || s.weighted || global_slots().nsamples > 0) return false;
    if (s.off.device() != X.device()) return false;
    return true;
}

torch::Tensor gat_input_layer_apply(torch::Tensor X, torch::Tensor weight, torch::Tensor bias, torch::Tensor attn_l_weight,
                                    torch::Tensor attn_l_bias, torch::Tensor attn_r_weight, torch::Tensor attn_r_bias,
                                    int64_t li, double slope, int64_t mode, bool relu) {
    const int64_t heads = attn_l_bias.numel();
    if (gat_input_layer_eligible(X, weight, li, heads, mode))
        return GatInputLayer::apply(X, weight, bias, attn_l_weight, attn_l_bias, attn_r_weight, attn_r_bias, li,
                                    slope, heads, relu);
    auto v1 = ffn_apply(X, weight, bias);
    auto aL = head_attn_apply(v1, attn_l_weight, attn_l_bias);
    auto y = gat_aggregate_ffn_apply(aL, v1, attn_r_weight, attn_r_bias, li, slope, mode);
    return relu ? torch::relu(y) : y;
}

}  // namespace gala
