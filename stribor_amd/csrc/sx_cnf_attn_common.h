// What the two attention CNF kernel files (sx_cnf_attn.hip: DiffeqSelfAttention under 'compute_set'; sx_cnf_exact_attn.hip:
// DiffeqExactTraceAttention under 'exact') have in common beyond sx_cnf_common.h: the k / v exchange areas' geometry, what a lane
// knows of its place in the workgroup's pass, the scores and P.V products on the matrix pipe, the key mask and the non-finite rule of
// the exchange.  The pieces were sx_cnf_attn.hip's own and moved here as they were.  Internal linkage: two translation units include it.
#pragma once
#include "sx_cnf_common.h"

#define CA_LD 36                                  /* row stride of the exchange areas (floats): 16-byte rows, conflict-free reads */
#define CA_AREA (SX_CNF_ROWS * CA_LD)             /* one k (or v) area */

namespace {

// where a lane stands in its workgroup's pass
struct ca_pos {
    int rho;            // row slot 0 .. SX_CNF_ROWS - 1
    int first;          // the first slot of the row's set (a padding slot: itself)
    int n;              // rows of that set (a padding slot: 1)
    int kt_lo, kt_hi;   // the key tiles that hold rows of the wave's sets (wave-uniform)
};

// scores of the wave's queries (qm: zero outside the head's features [lo, hi)) against the 32 keys at `kb` (the tile's first row + (lane &
// 31) rows + 4 h floats)
__device__ __forceinline__ f32x16 ca_scores(const f32x16 &qm, const float *kb, int lo, int hi) {
    f32x16 acc = {};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (8 * g < hi && 8 * g + 8 > lo) {
            const f32x4 k = *reinterpret_cast<const f32x4 *>(kb + 8 * g);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.x, qm[4 * g + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.y, qm[4 * g + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.z, qm[4 * g + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.w, qm[4 * g + 3], acc, 0, 0, 0);
        }
    }
    return acc;
}

// acc += V^T w over the 32 keys of a tile: `vb` = the tile's first row + 4 h rows + (lane & 31) floats; e_in: the lane's feature is the head's
__device__ __forceinline__ void ca_pv(f32x16 &acc, const f32x16 &w, const float *vb, bool e_in) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = vb[sx_kmap(r, 0) * CA_LD];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(e_in ? v : 0.f, w[r], acc, 0, 0, 0);
    }
}

__device__ __forceinline__ bool ca_valid(const ca_pos &p, int js, bool md) { return js >= p.first && js < p.first + p.n && !(md && js == p.rho); }

__device__ __forceinline__ float ca_finite(float v, bool &bad) {
    const bool ok = fabsf(v) < INFINITY;
    bad = bad || !ok;
    return ok ? v : 0.f;
}

}  // namespace
