// gat_wide.h -- entry of the wide-row fused GAT kernels (gat_wide.hip) for the dispatchers
// of gat.hip and gat_fused.hip.
#pragma once

#include "gat_common.h"

namespace gala {

// 256 < F <= 1024 floats per row, float4 operands (vec == 4), D = F / heads a multiple of 4,
// at most 32 heads, one segment, no hub rows in the graph's plan.
bool gat_wide_shape(const gala_csr_t *A, int32_t F, int32_t heads, int vec);

// The forward: mode GALA_SOFTMAX_REF / _FIXED / kRefStats; d as gat_fwd_impl fills it (no
// partial, no continuation, no self_col).  Returns a gala_status (launch_status()).
int gat_wide_fwd(const EdgeParams &p, const GatDev &d, int mode, hipStream_t hs);

// The REF row-statistics backward; d as bwd_stats_impl fills it (no dy_rows; attn_w, the
// Linear-folding form, is served).
int gat_wide_bwd_stats(const EdgeParams &p, const GatDev &d, hipStream_t hs);

}  // namespace gala
