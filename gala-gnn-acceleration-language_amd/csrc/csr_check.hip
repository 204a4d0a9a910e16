// csr_check.hip -- gala_csr_is_transpose_i32: is the CSR pattern `at` exactly the transpose of
// the CSR pattern `a`?  One grid-stride pass over a flat index of n rows, at's edges and a's
// edges; every item that fails its test adds one to an int32 count in device memory (zero:
// transpose).  The tests, for square single-segment patterns of the same n and nnz:
//   rows of at:   rowptr[0] = 0, rowptr[n] = nnz, rowptr[c] <= rowptr[c + 1]: the rows of at
//                 partition its nnz slots;
//   edges of at:  column in [0, n), larger than its predecessor's in the same row (strictly
//                 ascending: no duplicates, and the search below is licensed);
//   edges of a:   column c in [0, n), larger than its predecessor's in the same row (a's
//                 edges are distinct), and the edge's row r found by binary search in row c
//                 of at.
// nnz distinct edges of a, each found in one of at's nnz slots, the slots of distinct rows
// disjoint: at holds a's edges transposed and nothing else.  An edge's row comes from a binary
// search of the row offsets, so a hub row's edges are spread over the grid like any others.
// A malformed at counts and does not fault: offsets are clamped to [0, nnz] before they index
// col, columns are tested against n before they index rowptr.
#include <hip/hip_runtime.h>

#include "gala_internal.h"

namespace gala {

constexpr int kCheckMaxBlocks = 1024;  // grid cap: kCheckMaxBlocks * kBlock items per round

struct TransposeCheck {
    const int32_t *a_rp, *a_col, *t_rp, *t_col;
    int64_t n, a_nnz, t_nnz;
    int32_t *count;
};

// the row of edge e: the last r in [0, n) with rp[r] <= e (0 when there is none)
__device__ __forceinline__ int64_t edge_row(const int32_t *rp, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;  // rp[lo] <= e (or lo == 0), rp[hi] > e (or hi == n)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)rp[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t clamp_off(int32_t v, int64_t nnz) {
    return v < 0 ? 0 : ((int64_t)v > nnz ? nnz : (int64_t)v);
}

// edge e of a pattern: column in range and above its predecessor's in the same row
__device__ __forceinline__ bool edge_ascends(const int32_t *rp, const int32_t *col, int64_t n, int64_t nnz,
                                             int64_t e, int64_t &row) {
    row = edge_row(rp, n, e);
    const int32_t c = col[e];
    if (c < 0 || (int64_t)c >= n) return false;
    const int64_t r0 = clamp_off(rp[row], nnz);
    return e <= r0 || col[e - 1] < c;
}

__global__ __launch_bounds__(kBlock) void k_csr_is_transpose(TransposeCheck k) {
    const int64_t total = k.n + k.t_nnz + k.a_nnz;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        if (i < k.n) {
            bool ok = k.t_rp[i] <= k.t_rp[i + 1];
            if (i == 0) ok = ok && k.t_rp[0] == 0 && (int64_t)k.t_rp[k.n] == k.t_nnz && k.a_nnz == k.t_nnz;
            bad += !ok;
        } else if (i < k.n + k.t_nnz) {
            int64_t row;
            bad += !edge_ascends(k.t_rp, k.t_col, k.n, k.t_nnz, i - k.n, row);
        } else {
            int64_t r;
            const int64_t e = i - k.n - k.t_nnz;
            bool ok = edge_ascends(k.a_rp, k.a_col, k.n, k.a_nnz, e, r);
            if (ok) {
                const int64_t c = k.a_col[e];
                int64_t lo = clamp_off(k.t_rp[c], k.t_nnz), hi = clamp_off(k.t_rp[c + 1], k.t_nnz);
                while (lo < hi) {  // the first slot of row c whose column is >= r
                    const int64_t mid = lo + (hi - lo) / 2;
                    if ((int64_t)k.t_col[mid] < r) lo = mid + 1;
                    else hi = mid;
                }
                ok = lo < clamp_off(k.t_rp[c + 1], k.t_nnz) && (int64_t)k.t_col[lo] == r;
            }
            bad += !ok;
        }
    }
    // a thread's share capped so that the count cannot wrap round to zero
    const int32_t cap = (int32_t)((int64_t)INT32_MAX / stride);
    if (bad) atomicAdd(k.count, bad < cap ? bad : cap);
}

}  // namespace gala

using namespace gala;

extern "C" int gala_csr_is_transpose_i32(const gala_csr_t *a, const gala_csr_t *at, int32_t *result, void *stream) {
    int st = check_csr(a);
    if (st) return st;
    if ((st = check_csr(at))) return st;
    if (!result) return GALA_ERR_INVALID_ARG;
    if (a->n_seg != 1 || at->n_seg != 1) return GALA_ERR_INVALID_ARG;
    if (a->n_rows != a->n_cols || at->n_rows != at->n_cols || a->n_rows != at->n_rows) return GALA_ERR_INVALID_ARG;
    hipStream_t hs = (hipStream_t)stream;
    if (hipMemsetAsync(result, 0, sizeof(int32_t), hs) != hipSuccess) return launch_status();
    if (a->n_rows == 0) return GALA_OK;
    TransposeCheck k{a->rowptr, a->col, at->rowptr, at->col, a->n_rows, a->nnz, at->nnz, result};
    const int64_t total = k.n + k.t_nnz + k.a_nnz;
    const int64_t blocks = std::min<int64_t>((total + kBlock - 1) / kBlock, kCheckMaxBlocks);
    hipLaunchKernelGGL(k_csr_is_transpose, dim3((unsigned)blocks), dim3(kBlock), 0, hs, k);
    return launch_status();
}
