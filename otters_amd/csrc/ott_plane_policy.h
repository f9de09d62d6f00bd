// ott_plane_policy.h — the two format decisions of the cascade's planes (ott_planes.hip), free of HIP and of ott_store: plain
// C++17, so that the CPU suite compiles the very code libotters_hip.so ships on its own (tests/test_plane_policy_cpu.py), as it
// does ott_policy.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace ott {

// a row whose measured loss ||x - plane(x)|| / ||x|| is above its plane's figure is marked irregular: always listed, always re-scored exactly
constexpr float I8_REL_FLAG = 0.03125f;        // 2^-5: eight times what a row of ordinary dynamic range measures at dim 768
constexpr float HALF_REL_FLAG = 9.765625e-4f;  // 2^-10: five times what a row of ordinary dynamic range measures

struct HiFormat {
    bool f16;     // IEEE half; else bf16, whose exponent range is f32's
    float scale;  // half only: the ONE power-of-two factor every row is multiplied by before the conversion (bf16: 1)
};
// Format of a hi plane that is built from scratch: IEEE half unless the store asks for bf16 (option hi_fmt = 0).
// min_regular_inv_bits: the float bits of the smallest non-zero inverse norm over the regular rows, i.e. 1 / the largest norm the
// factor has to accommodate (min_regular_inv_kernel; 0x7F800000 = the store has no regular row, which counts as a norm of 1).
inline HiFormat hi_plane_format(int hi_fmt, uint32_t min_regular_inv_bits) {
    if (hi_fmt == 0) return HiFormat{false, 1.0f};
    float min_inv;
    memcpy(&min_inv, &min_regular_inv_bits, 4);
    const float max_norm = (min_regular_inv_bits != 0x7F800000u && min_inv > 0.0f) ? 1.0f / min_inv : 1.0f;
    // factor = 2^-round(log2(max_norm) / 4).  The batch path multiplies its query operands by the RECIPROCAL (so the
    // accumulators need no correction): rows then sit around max_norm^0.75 / sqrt(dim), unit-length (cosine) queries
    // around max_norm^0.25 / sqrt(dim), raw (dot / L2) queries of similar length around max_norm^1.25 / sqrt(dim) — all
    // inside half's normal range for norms from ~1e-3 to a few thousand (cosine: to ~1e6).  Outside that, bf16.
    int e = 0;
    (void)frexpf(max_norm, &e);  // max_norm = m * 2^e, m in [0.5, 1)
    const float scale = ldexpf(1.0f, -(e / 4));
    if (!(scale > 0.0f) || !(scale < __builtin_inff()) || max_norm > 1e6f || max_norm < 1e-3f) return HiFormat{false, 1.0f};
    return HiFormat{true, scale};
}

// A plane built from scratch marked `rows_marked` of its `rows_converted` rows irregular: more than 1 row in 64 means the format
// is the wrong one for this store (half: norms spread over many binades — the plane is built again as bf16; int8: heavy-tailed
// elements — the plane is freed and the cascade starts at the hi pass)
inline bool format_rejected(uint64_t rows_marked, uint64_t rows_converted) { return rows_marked * 64 > rows_converted; }

}  // namespace ott
