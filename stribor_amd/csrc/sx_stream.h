// What the stream kernels (sx_elementwise.hip, sx_pointwise.hip, sx_rqs.hip) have in common.  They are the unfused tier: parameters
// already in HBM, one lane per element (or per 4 / 8 consecutive elements of a row):
//   * element access in a storage type (fp32 or bf16; all arithmetic is fp32): scalar, and 4- / 8-wide as ONE 8- or 16-byte access,
//     plain or streaming (non-temporal).  A launcher issues only accesses as wide as the alignment it checked;
//   * sx_row_ldj, the per-row log-det sum: fixed-order shuffle sums, no atomics -- aligned lane groups for power-of-two widths <= 64
//     (ldj_mode 1), the row-aligned units of sx_common.h for every other width (ldj_mode 2);
//   * on the host: the ldj_mode rule, the grid cap, the dispatch of runtime bools to template arguments, and the launch plan of the
//     two spline kernels (pass-through copy, LDS slices per wave, grid).
// Everything here has internal linkage: three translation units include it.
#pragma once
#include "sx_common.h"
#include <type_traits>

namespace {

// ---- element access ------------------------------------------------------------------------------------------------------
template <int N> using sx_u16v = uint16_t __attribute__((ext_vector_type(N)));

// NT: streaming (non-temporal) access -- for data touched exactly once
template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void st_stream(T *p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// element `off` of an array stored as bf16 or fp32
template <bool BF16>
__device__ __forceinline__ float sx_ld(const void *p, int64_t off) {
    if constexpr (BF16) return bf16_to_f32(reinterpret_cast<const uint16_t *>(p)[off]);
    else return reinterpret_cast<const float *>(p)[off];
}
template <bool BF16>
__device__ __forceinline__ void sx_st(void *p, int64_t off, float v) {
    if constexpr (BF16) reinterpret_cast<uint16_t *>(p)[off] = f32_to_bf16(v);
    else reinterpret_cast<float *>(p)[off] = v;
}

// the N consecutive elements from `off` on as N / 4 f32x4, in ONE access: bf16 N = 4 (8 bytes) or 8 (16 bytes), fp32 N = 4 (16 bytes)
template <bool BF16, int N, bool NT>
__device__ __forceinline__ void sx_ldv(const void *p, int64_t off, f32x4 *v) {
    if constexpr (BF16) {
        const sx_u16v<N> q = ld_stream<NT>(reinterpret_cast<const sx_u16v<N> *>(reinterpret_cast<const uint16_t *>(p) + off));
#pragma unroll
        for (int j = 0; j < N / 4; ++j)
            v[j] = f32x4{bf16_to_f32(q[4 * j]), bf16_to_f32(q[4 * j + 1]), bf16_to_f32(q[4 * j + 2]), bf16_to_f32(q[4 * j + 3])};
    } else {
        static_assert(N == 4, "fp32: one 16-byte access");
        v[0] = ld_stream<NT>(reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(p) + off));
    }
}
template <bool BF16, int N, bool NT>
__device__ __forceinline__ void sx_stv(void *p, int64_t off, const f32x4 *v) {
    if constexpr (BF16) {
        sx_u16v<N> o;
#pragma unroll
        for (int j = 0; j < N / 4; ++j) {
            o[4 * j] = f32_to_bf16(v[j].x); o[4 * j + 1] = f32_to_bf16(v[j].y);
            o[4 * j + 2] = f32_to_bf16(v[j].z); o[4 * j + 3] = f32_to_bf16(v[j].w);
        }
        st_stream<NT>(reinterpret_cast<sx_u16v<N> *>(reinterpret_cast<uint16_t *>(p) + off), o);
    } else {
        static_assert(N == 4, "fp32: one 16-byte access");
        st_stream<NT>(reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(p) + off), v[0]);
    }
}

// ---- per-row log-det sums --------------------------------------------------------------------------------------------------
// One object per work unit.  ldj[r] = (acc ? ldj[r] : 0) + scale * s, in exactly this order (a kernel without a scale passes 1).
struct sx_row_ldj {
    float *ldj;
    int acc;
    float scale;
    float row_acc = 0.f;        // ldj_mode 2, rows wider than a wave: the row's sum over its chunks

    __device__ __forceinline__ void put(int64_t r, float s) const { ldj[r] = (acc ? ldj[r] : 0.f) + scale * s; }
    // ldj_mode 1 (width a power of two <= 64: rows are aligned lane groups, a row never leaves the wave).  Every lane of the wave
    // calls it; s = the lane's part (0 for a lane without an element), first = the lane holds the first element of `row`
    __device__ __forceinline__ void group(float s, int width, bool first, int64_t row) const {
        s = group_sum_rt(s, width);
        if (first) put(row, s);
    }
    // ldj_mode 2 (row-aligned units), after each chunk of a unit: s0 as above, pos = the element's index in `row`
    __device__ __forceinline__ void chunk(const sx_units &units, float s0, int pos, int width, bool valid, int64_t row) {
        if (units.chunks == 1) {
            const float s = segment_sum_rt(s0, pos, width);
            if (valid && pos == 0) put(row, s);
        } else {
            row_acc += s0;
        }
    }
    // ... and after the unit's last chunk (rows wider than a wave: unit = row)
    __device__ __forceinline__ void finish(const sx_units &units, int lane, int64_t unit) const {
        if (units.chunks > 1) {
            const float s = group_sum<64>(row_acc);
            if (lane == 0) put(unit, s);
        }
    }
};

// ---- host ------------------------------------------------------------------------------------------------------------------
inline bool sx_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// how a kernel sums a row's `width` lanes into ldj: 0 no ldj, 1 aligned lane groups, 2 row-aligned units
inline int sx_ldj_mode(const float *ldj, int width) { return ldj ? (sx_pow2(width) && width <= 64 ? 1 : 2) : 0; }

inline int grid_for(int64_t work_items, int block, int max_blocks = 256 * 8) {
    int64_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// runtime bools -> template arguments: f(std::bool_constant<a>{}, ...); inside f, `A()` is a constant expression
template <class F>
inline void sx_dispatch(bool a, F &&f) {
    if (a) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
inline void sx_dispatch(bool a, bool b, F &&f) {
    sx_dispatch(a, [&](auto A) { sx_dispatch(b, [&](auto B) { f(A, B); }); });
}
template <class F>
inline void sx_dispatch(bool a, bool b, bool c, F &&f) {
    sx_dispatch(a, b, [&](auto A, auto B) { sx_dispatch(c, [&](auto C) { f(A, B, C); }); });
}

// One LDS slice of 64 * stride floats per wave (the wave's 64 elements' parameters): 4 waves per workgroup while that fits 64 KiB,
// else one.  The grid is capped at the workgroups resident at once (at most 8 per CU); the waves stride over the units.
struct sx_slice_plan {
    int block;
    size_t lds;
    int grid(int64_t n_units) const {
        const int wpb = block / 64;
        const int64_t per_cu = (160 * 1024) / (int64_t)lds > 8 ? 8 : (160 * 1024) / (int64_t)lds;
        int64_t g = (n_units + wpb - 1) / wpb;
        if (g > 256 * per_cu) g = 256 * per_cu;
        if (g < 1) g = 1;
        return (int)g;
    }
};
inline sx_slice_plan sx_plan_slices(int stride) {
    sx_slice_plan p{256, (size_t)4 * 64 * stride * sizeof(float)};
    if (p.lds > 64 * 1024) p = sx_slice_plan{64, (size_t)64 * stride * sizeof(float)};
    return p;
}

// copies the pass-through (mask == 1) columns: y = T(x)*(1-m) + x*m (coupling.py:78)
template <bool BF16>
__global__ __launch_bounds__(256) void rqs_copy_passthrough_kernel(const void *__restrict__ x, void *__restrict__ y,
                                                                   float *__restrict__ ldiag,
                                                                   const int32_t *__restrict__ live_idx, int l0,
                                                                   int n_live, int64_t n_rows, int dim, int copy_x) {
    extern __shared__ __attribute__((aligned(16))) char cp_smem[];
    int *is_live = reinterpret_cast<int *>(cp_smem);
    for (int c = threadIdx.x; c < dim; c += blockDim.x) is_live[c] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n_live; i += blockDim.x) is_live[live_idx ? live_idx[i] : l0 + i] = 1;
    __syncthreads();
    const int64_t total = n_rows * dim;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % dim);
        if (!is_live[c]) {
            if (copy_x) sx_st<BF16>(y, i, sx_ld<BF16>(x, i));
            if (ldiag) ldiag[i] = 0.f;
        }
    }
}

// What sx_rqs_coupling and sx_cubic_coupling (`who`) do before their own launch: the LDS slices of `stride` floats per element, the
// pass-through columns (and their zero log-diag entries), ldj of a layer without live columns, ldj_mode, the grid, and -- slices
// above 48 KiB -- the dynamic-LDS limit of every kernel kernel_of(bf16, inverse, aligned) names.  grid == 0: nothing left to launch.
struct sx_spline_plan {
    sx_slice_plan sl;
    int grid, ldj_mode;
};
template <class KernelOf>
inline int sx_plan_spline(const char *who, const void *x, void *y, float *ldj, float *ldiag, const int32_t *live_idx,
                          int32_t live_start, int32_t n_live, int32_t n_bins, int stride, int64_t n_rows, int32_t dim, int32_t dtype,
                          int32_t ldj_accumulate, hipStream_t st, KernelOf kernel_of, sx_spline_plan *plan) {
    *plan = sx_spline_plan{sx_plan_slices(stride), 0, 0};
    const size_t lds = plan->sl.lds;
    SX_REQUIRE(lds <= 160 * 1024, "%s: n_bins %d needs %zu B of LDS per wave", who, n_bins, lds);
    if (n_live < dim && (x != y || ldiag)) {
        sx_dispatch(dtype == SX_BF16, [&](auto BF) {
            hipLaunchKernelGGL(rqs_copy_passthrough_kernel<BF()>, dim3(grid_for(n_rows * dim, 256)), dim3(256), dim * sizeof(int), st,
                               x, y, ldiag, live_idx, live_start, n_live, n_rows, dim, x != y);
        });
        SX_LAUNCH_CHECK();
    }
    if (n_live == 0) {
        if (ldj && !ldj_accumulate) {
            hipError_t e = hipMemsetAsync(ldj, 0, n_rows * sizeof(float), st);
            if (e != hipSuccess) { sx_set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        }
        return SX_OK;
    }
    plan->ldj_mode = sx_ldj_mode(ldj, n_live);
    plan->grid = plan->sl.grid(sx_make_units(n_rows, n_live, plan->ldj_mode == 2).n_units);
    if (lds > 48 * 1024)
        for (int m = 0; m < 8; ++m)
            sx_dispatch(m & 1, m & 2, m & 4, [&](auto BF, auto INV, auto AL) {
                (void)hipFuncSetAttribute(kernel_of(BF, INV, AL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            });
    return SX_OK;
}

}  // namespace
