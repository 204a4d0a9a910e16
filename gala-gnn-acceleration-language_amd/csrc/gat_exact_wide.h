// gat_exact_wide.h -- entry of the wide-row exact GAT kernels (gat_exact_wide.hip) for the
// dispatcher of gat_exact.hip, and the operand block the two files share.
#pragma once

#include "gat_wide.h"

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

// Shapes of gat_wide_shape, square pattern, no self_col, d.dy_rows == d.dY.  Each returns a
// gala_status (launch_status()).
// The forward: d and x as gala_gat_fwd_stats_exact_ex_f32 fills them (d.aR NULL: recompute).
int gat_exact_wide_fwd(const EdgeParams &p, const GatDev &d, const ExactDev &x, hipStream_t hs);

// The backward: the pre-pass over p's rows, then the gather pass over pt's rows (the same
// pattern, or its transpose); d.aL the rows' aL, d.aR the rows' source logits.
int gat_exact_wide_bwd(const EdgeParams &p, const EdgeParams &pt, const GatDev &d, const ExactDev &x, hipStream_t hs);

}  // namespace gala
