// bfloat16 storage helpers shared by the HIP kernels and the host-CPU backend: a bf16 value is
// the upper 16 bits of an fp32, so widening is exact and narrowing is one rounding.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GALA_HD __host__ __device__ __forceinline__
#else
#define GALA_HD inline
#endif

namespace gala {

GALA_HD uint32_t f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}
GALA_HD float bits_f32(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// exact: bf16 bits -> the fp32 with those upper bits
GALA_HD float bf16_widen(uint16_t b) { return bits_f32((uint32_t)b << 16); }

// round to nearest even, as torch.Tensor.to(torch.bfloat16): +-Inf stays, every NaN becomes the
// quiet NaN 0x7FC0
GALA_HD uint16_t bf16_rne(float f) {
    const uint32_t u = f32_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace gala
