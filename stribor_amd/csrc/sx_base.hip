// Base densities with parameters (stribor/dist/normal.py:8-68, dist/uniform.py:8-52): Normal(loc, scale) and Uniform(low, high) with
// vector parameters of the row's width, and MultivariateNormal through the inverse of its lower-triangular factor.
//   * sx_base_logprob        one pass over x, the layouts of the unit_normal_* kernels (sx_elementwise.hip): 8 bf16 or 4 columns per
//                            lane when the row width and the alignment allow ONE 16- / 8-byte access, else one wave per row;
//   * sx_normal_logprob_bwd  dx and the column sums d loc / d scale: per-block partials added in slot order, no atomics;
//   * sx_mvn_logprob         z = Linv (x - loc) on v_mfma_f32_32x32x2_f32 in the fragment layout of sx_cnf_common.h (one wave = 32 rows
//                            on the MFMA column), Linv's lower tiles staged in LDS once per workgroup, z never leaves registers.
#include "sx_stream.h"
#include "sx_cnf_common.h"

namespace {

inline int base_ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// ---- sx_base_logprob ---------------------------------------------------------------------------------------------------------------
// One element's share of the row sum.  Normal: ((x - loc) / scale)^2.  Uniform: 0 inside [low, high), 1 outside, NaN for a NaN --
// the row's sum is then 0 (inside), positive (outside) or NaN.
template <int KIND>
__device__ __forceinline__ float base_term(float x, float p0, float p1) {
    if constexpr (KIND == SX_BASE_NORMAL) {
        const float z = (x - p0) * p1;
        return z * z;
    } else {
        return x != x ? x : ((p0 <= x && x < p1) ? 0.f : 1.f);
    }
}
template <int KIND>
__device__ __forceinline__ float base_finish(float s, float log_norm, float ldj) {
    if constexpr (KIND == SX_BASE_NORMAL) return -0.5f * s + log_norm + ldj;
    else return (s != s ? s : (s > 0.f ? -INFINITY : log_norm)) + ldj;
}

// N = 4 or 8 columns per lane in one access (x and the parameters aligned to it), 2^tpr_log2 lanes per row
template <int KIND, bool BF16, int N>
__global__ __launch_bounds__(256) void base_vec_kernel(const void *__restrict__ x, const float *__restrict__ p0, const float *__restrict__ p1,
                                                       float log_norm, const float *__restrict__ ldj, float *__restrict__ out,
                                                       int64_t n_rows, int dim, int tpr_log2) {
    const int tpr = 1 << tpr_log2;
    const int64_t n_vec = n_rows << tpr_log2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // (the tpr lanes of a row are an aligned lane group and n_vec is a multiple of tpr: a group is in the loop whole or not at all)
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += stride) {
        const int64_t row = v >> tpr_log2;
        const int c = ((int)(v & (tpr - 1))) * N;
        f32x4 xv[N / 4];
        sx_ldv<BF16, N, false>(x, row * dim + c, xv);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < N / 4; ++j) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(p0 + c + 4 * j), b = *reinterpret_cast<const f32x4 *>(p1 + c + 4 * j);
            s += (base_term<KIND>(xv[j].x, a.x, b.x) + base_term<KIND>(xv[j].y, a.y, b.y)) +
                 (base_term<KIND>(xv[j].z, a.z, b.z) + base_term<KIND>(xv[j].w, a.w, b.w));
        }
        s = group_sum_rt(s, tpr);
        if ((v & (tpr - 1)) == 0) out[row] = base_finish<KIND>(s, log_norm, ldj ? ldj[row] : 0.f);
    }
}

// any width, any alignment: one wave per row
template <int KIND, bool BF16>
__global__ __launch_bounds__(256) void base_generic_kernel(const void *__restrict__ x, const float *__restrict__ p0,
                                                           const float *__restrict__ p1, float log_norm, const float *__restrict__ ldj,
                                                           float *__restrict__ out, int64_t n_rows, int dim) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t row = wave; row < n_rows; row += n_waves) {
        float s = 0.f;
        for (int c = lane; c < dim; c += 64) s += base_term<KIND>(sx_ld<BF16>(x, row * dim + c), p0[c], p1[c]);
        s = group_sum<64>(s);
        if (lane == 0) out[row] = base_finish<KIND>(s, log_norm, ldj ? ldj[row] : 0.f);
    }
}

// ---- sx_normal_logprob_bwd ---------------------------------------------------------------------------------------------------------
// A block owns a contiguous slab of rows.  Its 256 threads are `rl` row lanes x `cw` columns (cw = the power of two >= min(dim, 64)):
// consecutive threads read consecutive columns.  Each thread keeps the two column sums of its rows; the row lanes are added through
// LDS in row-lane order and the block's 2 * dim sums go to its slot of `partial` ([block][loc | scale][dim]).
// (four workgroups per CU: with one, a SIMD holds a single wave and nothing runs under its loads)
#ifndef SX_NORMAL_BWD_MAX_BLOCKS
#define SX_NORMAL_BWD_MAX_BLOCKS 1024
#endif

inline int normal_bwd_cw(int dim) { int cw = 1; while (cw < dim && cw < 64) cw <<= 1; return cw; }
inline int64_t normal_bwd_rows_per_block(int64_t n_rows, int dim) {
    const int rl = 256 / normal_bwd_cw(dim);
    int64_t rpb = (n_rows + SX_NORMAL_BWD_MAX_BLOCKS - 1) / SX_NORMAL_BWD_MAX_BLOCKS;
    rpb = (rpb + rl - 1) / rl * rl;
    return rpb < rl ? rl : rpb;
}
inline int normal_bwd_blocks(int64_t n_rows, int dim) {
    const int64_t rpb = normal_bwd_rows_per_block(n_rows, dim);
    return (int)((n_rows + rpb - 1) / rpb);
}

__global__ __launch_bounds__(256) void normal_bwd_kernel(const float *__restrict__ x, const float *__restrict__ g, const float *__restrict__ loc,
                                                         const float *__restrict__ inv_scale, float *__restrict__ gx,
                                                         float *__restrict__ partial, int64_t n_rows, int dim, int cw_log2,
                                                         int64_t rows_per_block) {
    __shared__ float red[2][256];
    const int cw = 1 << cw_log2, rl = 256 >> cw_log2;
    const int col_in = threadIdx.x & (cw - 1), row_lane = threadIdx.x >> cw_log2;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    for (int c0 = 0; c0 < dim; c0 += cw) {
        const int c = c0 + col_in;
        float a_loc = 0.f, a_scale = 0.f;
        if (c < dim) {
            const float m = loc[c], is = inv_scale[c], is2 = is * is;
            for (int64_t r = r0 + row_lane; r < r1; r += rl) {
                const float gr = g[r], d = x[r * dim + c] - m;
                const float t = gr * (d * is2);                     // g (x - loc) / scale^2
                if (gx) gx[r * dim + c] = -t;
                a_loc += t;
                a_scale += t * (d * is) - gr * is;                  // g ((x - loc)^2 / scale^3 - 1 / scale)
            }
        }
        if (partial) {
            red[0][threadIdx.x] = a_loc;
            red[1][threadIdx.x] = a_scale;
            __syncthreads();
            if (threadIdx.x < cw && c < dim) {
                float s0 = 0.f, s1 = 0.f;
                for (int l = 0; l < rl; ++l) { s0 += red[0][(l << cw_log2) + col_in]; s1 += red[1][(l << cw_log2) + col_in]; }
                partial[((int64_t)blockIdx.x * 2 + 0) * dim + c] = s0;
                partial[((int64_t)blockIdx.x * 2 + 1) * dim + c] = s1;
            }
            __syncthreads();
        }
    }
}

// g_loc[c] / g_scale[c] = the blocks' partials: one wave per column, lane l adds the slots l, l + 64, ... in slot order, then the 64
// lanes are added by shuffles -- a fixed order, the same bits on every call
__global__ __launch_bounds__(256) void normal_bwd_reduce_kernel(const float *__restrict__ partial, float *__restrict__ g_loc,
                                                                float *__restrict__ g_scale, int n_blocks, int dim) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= dim) return;                                   // (a whole wave leaves)
    float s0 = 0.f, s1 = 0.f;
    for (int b = lane; b < n_blocks; b += 64) {
        s0 += partial[((int64_t)b * 2 + 0) * dim + c];
        s1 += partial[((int64_t)b * 2 + 1) * dim + c];
    }
    s0 = group_sum<64>(s0);
    s1 = group_sum<64>(s1);
    if (lane == 0) {
        if (g_loc) g_loc[c] = s0;
        if (g_scale) g_scale[c] = s1;
    }
}

// ---- sx_mvn_logprob ----------------------------------------------------------------------------------------------------------------
struct mvn_args {
    const void *x;
    const float *loc, *linv, *ldj;
    float *out;
    int64_t n_rows;
    int dim;
    float log_norm;
};

__host__ __device__ constexpr int mvn_tiles(int dim) { return (dim + 31) / 32; }
__host__ __device__ constexpr int mvn_tri(int m, int c) { return m * (m + 1) / 2 + c; }          // lower tile (m, c), c <= m
__host__ __device__ constexpr int mvn_lds_floats(int T) { return mvn_tri(T, 0) * 1024 + 32 * T; }

// T tiles of 32 columns; BF16 rows; VEC: a lane's four consecutive columns in one access (dim % 4 == 0, x aligned to the access)
template <int T, bool BF16, bool VEC>
__global__ __launch_bounds__(SX_CNF_THREADS) void mvn_kernel(mvn_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const int D = a.dim;
    // the lower tiles of Linv in A-fragment order (cnf_stage's layout per tile), then loc padded with zeros
    for (int e = threadIdx.x; e < mvn_tri(T, 0) * 1024; e += SX_CNF_THREADS) {
        const int tile = e >> 10, rem = e & 1023;
        int m = 0;
        while (mvn_tri(m + 1, 0) <= tile) ++m;
        const int c = tile - mvn_tri(m, 0);
        const int g = rem >> 8, ln = (rem >> 2) & 63, j = rem & 3;
        const int row = 32 * m + (ln & 31), col = 32 * c + sx_kmap(4 * g + j, ln >> 5);
        cnf_smem[e] = (row < D && col < D && col <= row) ? a.linv[(int64_t)row * D + col] : 0.f;
    }
    float *locs = cnf_smem + mvn_tri(T, 0) * 1024;
    for (int i = threadIdx.x; i < 32 * T; i += SX_CNF_THREADS) locs[i] = i < D ? a.loc[i] : 0.f;
    __syncthreads();
    const int64_t n_pass = (a.n_rows + SX_CNF_ROWS - 1) / SX_CNF_ROWS;
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        // the A fragments are read from LDS in every pass: hoisted out of the loop they would stay in registers (10 tiles = 160
        // registers at T = 4) and leave one wave per SIMD, with nothing to run under its loads -- the offset is opaque per pass
        int lane_off = lane * 4;
        asm volatile("" : "+v"(lane_off));
        const float *wb = cnf_smem + lane_off;
        const int64_t row = pass * SX_CNF_ROWS + wave * 32 + (lane & 31);
        const bool valid = row < a.n_rows;
        cnf_tile<T> d;                                  // x - loc, feature 32c + kmap(r, h) in register r of tile c
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = 32 * c + 8 * g + 4 * h;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if constexpr (VEC) {
                    if (valid && col < D) sx_ldv<BF16, 4, false>(a.x, row * D + col, &v);
                } else {
                    if (valid) {
                        if (col + 0 < D) v.x = sx_ld<BF16>(a.x, row * D + col + 0);
                        if (col + 1 < D) v.y = sx_ld<BF16>(a.x, row * D + col + 1);
                        if (col + 2 < D) v.z = sx_ld<BF16>(a.x, row * D + col + 2);
                        if (col + 3 < D) v.w = sx_ld<BF16>(a.x, row * D + col + 3);
                    }
                }
                const f32x4 m = *reinterpret_cast<const f32x4 *>(locs + col);
                d.v[c][4 * g + 0] = v.x - m.x;
                d.v[c][4 * g + 1] = v.y - m.y;
                d.v[c][4 * g + 2] = v.z - m.z;
                d.v[c][4 * g + 3] = v.w - m.w;
            }
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < T; ++m) {
            f32x16 acc = {};
#pragma unroll
            for (int c = 0; c <= m; ++c) {              // the tiles above the diagonal are zero: skipped
                const cnf_tile<1> in = {{d.v[c]}};
                cnf_mma<1>(acc, in, wb + mvn_tri(m, c) * 1024);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s += acc[r] * acc[r];
        }
        s += __shfl_xor(s, 32, 64);                     // the two lane halves hold the two halves of a row's features
        if (valid && h == 0) a.out[row] = -0.5f * s + a.log_norm + (a.ldj ? a.ldj[row] : 0.f);
    }
}

template <int T>
int mvn_launch(const mvn_args &a, bool bf16, bool vec, void *stream) {
    const size_t lds = (size_t)mvn_lds_floats(T) * sizeof(float);
    const int64_t want = cnf_row_blocks(a.n_rows);
    int rc = SX_OK;
    sx_dispatch(bf16, vec, [&](auto BF, auto VEC) { rc = cnf_launch<mvn_kernel<T, BF(), VEC()>>("sx_mvn_logprob", a, lds, want, stream); });
    return rc;
}

}  // namespace

extern "C" int sx_base_logprob(const void *x, const float *p0, const float *p1, float log_norm, const float *ldj, float *out,
                               int64_t n_rows, int32_t dim, int32_t dtype, int32_t kind, void *stream) {
    SX_REQUIRE(x && p0 && p1 && out, "sx_base_logprob: null pointer");
    SX_REQUIRE(dim > 0 && n_rows >= 0, "sx_base_logprob: bad sizes");
    SX_REQUIRE(dtype == SX_F32 || dtype == SX_BF16, "sx_base_logprob: bad dtype");
    SX_REQUIRE(kind == SX_BASE_NORMAL || kind == SX_BASE_UNIFORM, "sx_base_logprob: kind must be SX_BASE_NORMAL or SX_BASE_UNIFORM, got %d", kind);
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const bool aligned = ((((uintptr_t)x) | ((uintptr_t)p0) | ((uintptr_t)p1)) & 15) == 0;
    const bool by8 = dtype == SX_BF16 && dim % 8 == 0 && sx_pow2(dim / 8) && dim / 8 <= 64 && aligned;
    const bool by4 = dim % 4 == 0 && sx_pow2(dim / 4) && dim / 4 <= 64 && aligned;
    sx_dispatch(kind == SX_BASE_UNIFORM, dtype == SX_BF16, [&](auto UNI, auto BF) {
        constexpr int KIND = UNI() ? SX_BASE_UNIFORM : SX_BASE_NORMAL;
        if (by8) {
            if constexpr (BF()) {
                const int tl = base_ilog2(dim / 8);
                hipLaunchKernelGGL((base_vec_kernel<KIND, true, 8>), dim3(grid_for(n_rows << tl, 256)), dim3(256), 0, st, x, p0, p1, log_norm,
                                   ldj, out, n_rows, dim, tl);
            }
        } else if (by4) {
            const int tl = base_ilog2(dim / 4);
            hipLaunchKernelGGL((base_vec_kernel<KIND, BF(), 4>), dim3(grid_for(n_rows << tl, 256)), dim3(256), 0, st, x, p0, p1, log_norm, ldj,
                               out, n_rows, dim, tl);
        } else {
            hipLaunchKernelGGL((base_generic_kernel<KIND, BF()>), dim3(grid_for(n_rows * 64, 256)), dim3(256), 0, st, x, p0, p1, log_norm, ldj,
                               out, n_rows, dim);
        }
    });
    SX_LAUNCH_CHECK();
    return SX_OK;
}

extern "C" size_t sx_normal_bwd_partial_floats(int64_t n_rows, int32_t dim) {
    if (n_rows <= 0 || dim <= 0) return 0;
    return (size_t)2 * dim * normal_bwd_blocks(n_rows, dim);
}

extern "C" int sx_normal_logprob_bwd(const float *x, const float *g, const float *loc, const float *inv_scale, float *gx, float *g_loc,
                                     float *g_scale, float *partial, int64_t n_rows, int32_t dim, void *stream) {
    SX_REQUIRE(x && g && loc && inv_scale, "sx_normal_logprob_bwd: null pointer");
    SX_REQUIRE(dim > 0 && n_rows >= 0, "sx_normal_logprob_bwd: bad sizes");
    const bool sums = g_loc || g_scale;
    SX_REQUIRE(!sums || n_rows == 0 || partial, "sx_normal_logprob_bwd: the partial buffer is missing (sx_normal_bwd_partial_floats)");
    hipStream_t st = sx_stream(stream);
    if (n_rows == 0) {
        // no rows: the column sums are zero
        for (float *p : {g_loc, g_scale})
            if (p) {
                hipError_t e = hipMemsetAsync(p, 0, (size_t)dim * sizeof(float), st);
                if (e != hipSuccess) { sx_set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
            }
        return SX_OK;
    }
    if (!sums && !gx) return SX_OK;
    const int n_blocks = normal_bwd_blocks(n_rows, dim);
    hipLaunchKernelGGL(normal_bwd_kernel, dim3(n_blocks), dim3(256), 0, st, x, g, loc, inv_scale, gx, sums ? partial : (float *)nullptr, n_rows,
                       dim, base_ilog2(normal_bwd_cw(dim)), normal_bwd_rows_per_block(n_rows, dim));
    SX_LAUNCH_CHECK();
    if (sums) {
        hipLaunchKernelGGL(normal_bwd_reduce_kernel, dim3((dim + 3) / 4), dim3(256), 0, st, partial, g_loc, g_scale, n_blocks, dim);
        SX_LAUNCH_CHECK();
    }
    return SX_OK;
}

extern "C" size_t sx_mvn_lds_bytes(int32_t dim) {
    if (dim < 1 || dim > SX_MVN_MAX_DIM) return 0;
    return (size_t)mvn_lds_floats(mvn_tiles(dim)) * sizeof(float);
}

extern "C" int sx_mvn_logprob(const void *x, const float *loc, const float *linv, float log_norm, const float *ldj, float *out,
                              int64_t n_rows, int32_t dim, int32_t dtype, void *stream) {
    SX_REQUIRE(x && loc && linv && out, "sx_mvn_logprob: null pointer");
    SX_REQUIRE(dim > 0 && n_rows >= 0, "sx_mvn_logprob: bad sizes");
    SX_REQUIRE(dim <= SX_MVN_MAX_DIM, "sx_mvn_logprob: dim %d beyond SX_MVN_MAX_DIM (%d)", dim, SX_MVN_MAX_DIM);
    SX_REQUIRE(dtype == SX_F32 || dtype == SX_BF16, "sx_mvn_logprob: bad dtype");
    if (n_rows == 0) return SX_OK;
    const mvn_args a{x, loc, linv, ldj, out, n_rows, dim, log_norm};
    const bool bf16 = dtype == SX_BF16;
    const bool vec = dim % 4 == 0 && (((uintptr_t)x) & (bf16 ? 7 : 15)) == 0;
    switch (mvn_tiles(dim)) {
        case 1: return mvn_launch<1>(a, bf16, vec, stream);
        case 2: return mvn_launch<2>(a, bf16, vec, stream);
        case 3: return mvn_launch<3>(a, bf16, vec, stream);
        default: return mvn_launch<4>(a, bf16, vec, stream);
    }
}
