// The SpMM's bf16 storage paths (csrc/spmm_bf16.hip), launched by gala_spmm_ex_f32's dispatch
// in csrc/spmm.hip under GALA_SPMM_X_BF16 / GALA_SPMM_Y2_BF16.
#pragma once

#include "gala_internal.h"

namespace gala {

// one launch: one segment, no sampling, no ReLU epilogue (refused on the host)
struct Bf16Params {
    const int32_t *rowptr;
    const int32_t *col;
    const float *val;
    const float *val_rs;
    const void *X;            // bf16 (GALA_SPMM_X_BF16) or fp32 [n_cols, ldx], at the launch's first column
    float *Y;
    const float *src_scale;
    const float *dst_scale;
    int64_t n_rows;
    int64_t ldx;              // in elements of X's type
    int64_t ldy;
    int32_t F;                // columns of this launch
    int32_t f_base;           // the launch's first column (its edge-weight head is (f_base + f) / head_dim)
    int32_t val_heads;
    int32_t head_dim;
    int32_t accum;
    int32_t split_threshold;  // > 0: longer rows are left to the hub kernel
    const int32_t *row_order;
    int32_t xcd_order;
    int32_t dst_deg;
    void *Y2;                 // nullable; bf16 (y2_bf16) or fp32 [n_rows, ldy2]
    int64_t ldy2;             // in elements of Y2's type
    const float *y2_scale;
    int32_t y2_bf16;
};

struct Bf16Hub {
    const int32_t *rows;
    const int32_t *order;
    int64_t n_hub;
    int32_t n_slices;
};

constexpr int kBf16MaxVecs = 256;  // vectors of a row per launch (64 lanes x 4 chunks)

// widest vector (elements per lane and load) the operands allow: 8 / 4 / 2 / 1 bf16 or
// 4 / 2 / 1 fp32 of X, with Y (and an fp32 Y2) in vectors of min(xv, 4) floats
int bf16_pick_vec(bool x_bf16, const void *X, int64_t ldx, const float *Y, int64_t ldy, const void *Y2,
                  int64_t ldy2, bool y2_bf16, int32_t F, int32_t head_dim, bool one_head);
// the rows up to the plan's threshold (all rows without one); L = ceil(F / xv) <= kBf16MaxVecs
int bf16_launch_rows(const Bf16Params &p, bool x_bf16, int xv, hipStream_t st);
// the hub rows in REF order from bf16 X
int bf16_launch_hub(const Bf16Params &p, Bf16Hub hp, int xv, hipStream_t st);
// Y2 = bf16(s2 * Y) of the hub rows, after the fp32 hub kernel wrote their Y
int bf16_launch_hub_y2(const Bf16Params &p, Bf16Hub hp, hipStream_t st);

}  // namespace gala
