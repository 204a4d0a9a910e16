// gat_headw.h -- entry of the narrow-row fused GAT kernels for head widths that are no power
// of two of float4 vectors (gat_headw.hip: 3 x 40, 5 x 20, 8 x 24, 21 x 12), for the
// dispatchers of gat.hip and gat_fused.hip.
#pragma once

#include "gat_common.h"

namespace gala {

// heads >= 2, D = F / heads a multiple of 4 with D / 4 no power of two, F <= 256, float4
// operands (vec == 4), one segment, a square pattern (n_cols == n_rows: the kernels read row r
// of the column operands X, dY, Y and Ym for every row r), no hub rows in the graph's plan.
bool gat_headw_shape(const gala_csr_t *A, int32_t F, int32_t heads, int vec);

// The forward: mode GALA_SOFTMAX_REF / _FIXED with the source logits recomputed (d.aR NULL),
// kRefStats with either; d as gat_fwd_impl fills it (no partial, no continuation, no
// self_col).  Returns a gala_status (launch_status()).
int gat_headw_fwd(const EdgeParams &p, const GatDev &d, int mode, hipStream_t hs);

// The REF row-statistics backward; d as bwd_stats_impl fills it (no dy_rows; attn_w, the
// Linear-folding form, is served).
int gat_headw_bwd_stats(const EdgeParams &p, const GatDev &d, hipStream_t hs);

}  // namespace gala
