// Time-dependent element-wise flows of the reference (stribor/flows/activations.py:125-196): ContinuousTanh, the solution of
// dx/dt = tanh x in both directions, and ContinuousActivation, x (1 - w) + act(x) w with w = tanh(temperature t) for act = tanh / sigmoid /
// relu.  One time per row.
//
// Forward: one pass over HBM in sx_pointwise's shape -- read x (and one t per row), write y and, when asked, the per-element log-derivative
// and / or its row sum; one lane = 1, 4 or 8 consecutive elements of a row (16-byte accesses when the row length and the pointers allow).
// Backward: gx per element, the time gradient as a row sum, the temperature gradient as fixed-order partials (one per wave, fp64) and one
// ordered reduce; no atomics anywhere.
#include "sx_stream.h"

#include "sx_pointwise_time_core.h"

template <bool BF16, int VEC, bool ALIGNED>
__global__ __launch_bounds__(256) void pointwise_time_kernel(const void *__restrict__ x, const float *__restrict__ t, void *__restrict__ y,
                                                             float *__restrict__ ldj, float *__restrict__ ldiag, int64_t n_rows, int dim,
                                                             int kind, float param, int ldj_mode, int ldj_acc) {
    const int gdim = dim / VEC;                         // lanes per row
    const int64_t total = n_rows * gdim;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int row_shift = 31 - __builtin_clz(gdim);     // used when gdim is a power of two
    const bool flow = pwt_is_flow(kind);
    // one lane = VEC consecutive elements of row `row` at (vector) index i; returns the lane's log-det part
    auto body = [&](int64_t i, int64_t row) -> float {
        const float rp = pwt_row(kind, param, t[row]);
        float ld_sum = 0.f;
        float xv[VEC], out[VEC], ld[VEC];
        if constexpr (VEC >= 4) {
            f32x4 v[VEC / 4];
            sx_ldv<BF16, VEC, true>(x, VEC * i, v);                 // streaming: every byte is touched once
#pragma unroll
            for (int c = 0; c < VEC; ++c) xv[c] = v[c / 4][c % 4];
        } else xv[0] = sx_ld<BF16>(x, i);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            if (flow) {
                const pwt_flow_out o = pwt_tanh_flow(rp, xv[c]);
                out[c] = o.y; ld[c] = o.ld;
            } else {
                out[c] = pwt_mix(kind, rp, xv[c]); ld[c] = 0.f;
            }
            ld_sum += ld[c];
        }
        if (y) {
            if constexpr (VEC >= 4) {
                f32x4 o[VEC / 4];
#pragma unroll
                for (int c = 0; c < VEC; ++c) o[c / 4][c % 4] = out[c];
                sx_stv<BF16, VEC, true>(y, VEC * i, o);
            } else sx_st<BF16>(y, i, out[0]);
        }
        if (ldiag) {
            if constexpr (VEC >= 4) {
#pragma unroll
                for (int c = 0; c < VEC; c += 4)
                    __builtin_nontemporal_store(f32x4{ld[c], ld[c + 1], ld[c + 2], ld[c + 3]}, reinterpret_cast<f32x4 *>(ldiag + VEC * i + c));
            } else ldiag[i] = ld[0];
        }
        return ld_sum;
    };
    if constexpr (ALIGNED) {
        // row sums for any row length without atomics: row-aligned units (sx_common.h), fixed-order sums
        const int lane = threadIdx.x & 63;
        const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = stride >> 6;
        const sx_units units = sx_make_units(n_rows, gdim, true);
        for (int64_t u = wave; u < units.n_units; u += n_waves) {
            sx_row_ldj rl{ldj, ldj_acc, 1.f};
            for (int chunk = 0; chunk < units.chunks; ++chunk) {
                int64_t e0;
                int n_here;
                sx_unit_span(units, u, chunk, n_rows, gdim, &e0, &n_here);
                const bool valid = lane < n_here;
                const int64_t row = (e0 + lane) / gdim;
                rl.chunk(units, valid ? body(e0 + lane, row) : 0.f, (int)((e0 + lane) - row * gdim), gdim, valid, row);
            }
            rl.finish(units, lane, u);
        }
        return;
    }
    const bool pow2 = (gdim & (gdim - 1)) == 0;
    // the loop bound is rounded up to whole waves so that every lane of a wave reaches the shuffle sum
    const int64_t total_up = (total + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_up; i += stride) {
        const bool valid = i < total;
        const int64_t row = pow2 ? i >> row_shift : i / gdim;
        const float ld_sum = valid ? body(i, row) : 0.f;
        if (ldj_mode == 1) sx_row_ldj{ldj, ldj_acc, 1.f}.group(ld_sum, gdim, valid && (i & (gdim - 1)) == 0, row);
    }
}

// ---- backward (training, layer-wise path) --------------------------------------------------------------------------------------------
// A row takes W = min(64, dim rounded up to a power of two) consecutive lanes of a wave (64 / W rows per wave and pass; rows wider than
// a wave are walked 64 columns at a time).  gx per element; the row's sum of dL/d(row time) by a butterfly over its lanes; the
// temperature gradient is summed per lane over the lane's rows in fp64, then over the wave, one partial per wave.
__global__ __launch_bounds__(256) void pointwise_time_bwd_kernel(const float *__restrict__ x, const float *__restrict__ t,
                                                                 const float *__restrict__ gy, const float *__restrict__ gldj,
                                                                 const float *__restrict__ gldiag, float *__restrict__ gx,
                                                                 float *__restrict__ gt, double *__restrict__ partial, int64_t n_rows,
                                                                 int dim, int kind, float param, int W) {
    const int lane = threadIdx.x & 63;
    const int rpw = 64 / W, sub = lane / W, pos = lane - sub * W;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_groups = (n_rows + rpw - 1) / rpw;
    const bool flow = pwt_is_flow(kind);
    double tp = 0.0;
    for (int64_t g = wave; g < n_groups; g += n_waves) {
        const int64_t row = g * rpw + sub;
        const bool live = row < n_rows;
        float rsum = 0.f, tr = 0.f, rp = 0.f;
        if (live) {
            tr = t[row];
            rp = pwt_row(kind, param, tr);
            const float gl_row = gldj ? gldj[row] : 0.f;
            for (int c = pos; c < dim; c += W) {
                const int64_t i = row * dim + c;
                const float xv = x[i], g_y = gy ? gy[i] : 0.f;
                if (flow) {
                    const float gl = gl_row + (gldiag ? gldiag[i] : 0.f);
                    const pwt_flow_out o = pwt_tanh_flow(rp, xv);
                    const float dydx = expf(o.ld);
                    gx[i] = g_y * dydx + gl * (o.tanh_x - o.tanh_y * dydx);
                    rsum += g_y * o.tanh_y + gl * o.sech2_y;
                } else {
                    float dact;
                    const float av = pwt_act(kind, xv, dact);
                    gx[i] = g_y * ((1.f - rp) + dact * rp);
                    rsum += g_y * (av - xv);
                }
            }
        }
        rsum = group_sum_rt(rsum, W);
        if (live && pos == 0) {
            if (flow) {
                // d tau / dt: the direction's sign, and 1 / (1 + t) under log_time
                float dtau = kind == SX_PWT_TANH_FLOW_INV ? -1.f : 1.f;
                if (param != 0.f) dtau /= (1.f + tr);
                if (gt) gt[row] = rsum * dtau;
            } else {
                const float dw = rsum * (1.f - rp * rp);        // dL/dw (1 - w^2)
                if (gt) gt[row] = dw * param;
                tp += (double)dw * (double)tr;
            }
        }
    }
    if (partial) {
        tp = wave_sum_f64(tp);
        if (lane == 0) partial[wave] = tp;
    }
}

// the ordered reduce: one wave, lane l sums partials l, l + 64, ... in that order, then the butterfly
__global__ __launch_bounds__(64) void pointwise_time_reduce_kernel(const double *__restrict__ partial, int n, float *__restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s += partial[i];
    s = wave_sum_f64(s);
    if (threadIdx.x == 0) out[0] = (float)s;
}

static bool pwt_kind_ok(int kind) { return kind >= SX_PWT_TANH_FLOW && kind <= SX_PWT_MIX_RELU; }

extern "C" int sx_pointwise_time_bwd(const float *x, const float *t, const float *gy, const float *gldj, const float *gldiag, float *gx,
                                     float *gt, float *gparam, double *partial, int64_t n_rows, int32_t dim, int32_t kind, float param,
                                     void *stream) {
    SX_REQUIRE(x && t && gx, "sx_pointwise_time_bwd: null pointer");
    SX_REQUIRE(dim > 0 && n_rows >= 0, "sx_pointwise_time_bwd: bad sizes");
    SX_REQUIRE(pwt_kind_ok(kind), "sx_pointwise_time_bwd: unknown kind %d", kind);
    const bool flow = kind <= SX_PWT_TANH_FLOW_INV;
    SX_REQUIRE(flow || (gldj == nullptr && gldiag == nullptr), "sx_pointwise_time_bwd: the mix kinds have no log-derivative");
    SX_REQUIRE(gy || gldj || gldiag, "sx_pointwise_time_bwd: no incoming adjoint");
    SX_REQUIRE(gparam == nullptr || (!flow && partial != nullptr && ((uintptr_t)partial & 7) == 0),
               "sx_pointwise_time_bwd: the temperature gradient belongs to the mix kinds and needs the partial buffer (8-byte aligned)");
    hipStream_t st = sx_stream(stream);
    if (n_rows == 0) {
        if (gparam) {
            hipError_t e = hipMemsetAsync(gparam, 0, sizeof(float), st);
            if (e != hipSuccess) { sx_set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        }
        return SX_OK;
    }
    int W = 1;
    while (W < dim && W < 64) W <<= 1;
    const int64_t n_groups = (n_rows + (64 / W) - 1) / (64 / W);
    const int g = grid_for(n_groups * 64, 256, SX_PWT_PARTIALS / 4);     // 4 waves per workgroup, one partial per wave
    hipLaunchKernelGGL(pointwise_time_bwd_kernel, dim3(g), dim3(256), 0, st, x, t, gy, gldj, gldiag, gx, gt, gparam ? partial : nullptr,
                       n_rows, dim, kind, param, W);
    SX_LAUNCH_CHECK();
    if (gparam) {
        hipLaunchKernelGGL(pointwise_time_reduce_kernel, dim3(1), dim3(64), 0, st, partial, g * 4, gparam);
        SX_LAUNCH_CHECK();
    }
    return SX_OK;
}

extern "C" int sx_pointwise_time(const void *x, const float *t, void *y, float *ldj, float *ldiag, int64_t n_rows, int32_t dim,
                                 int32_t dtype, int32_t kind, float param, int32_t ldj_accumulate, void *stream) {
    SX_REQUIRE(x != nullptr && t != nullptr, "sx_pointwise_time: null x / t");
    SX_REQUIRE(dim > 0 && n_rows >= 0, "sx_pointwise_time: bad sizes");
    SX_REQUIRE(dtype == SX_F32 || dtype == SX_BF16, "sx_pointwise_time: bad dtype");
    SX_REQUIRE(pwt_kind_ok(kind), "sx_pointwise_time: unknown kind %d", kind);
    SX_REQUIRE(kind <= SX_PWT_TANH_FLOW_INV || (ldj == nullptr && ldiag == nullptr),
               "sx_pointwise_time: the mix kinds have no log-derivative (activations.py:155-159)");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const size_t esz = dtype == SX_BF16 ? 2 : 4;
    auto fits = [&](int v) {
        return (dim % v == 0) && (((uintptr_t)x % (v * esz)) == 0) && (y == nullptr || ((uintptr_t)y % (v * esz)) == 0) &&
               (ldiag == nullptr || ((uintptr_t)ldiag % 16) == 0);
    };
    const int vec = (dtype == SX_BF16 && fits(8)) ? 8 : fits(4) ? 4 : 1;
    const int gdim = dim / vec;
    const int ldj_mode = sx_ldj_mode(ldj, gdim);
    const int g = grid_for(ldj_mode == 2 ? sx_make_units(n_rows, gdim, true).n_units * 64 : n_rows * gdim, 256);
#define PWT_GO(BF, V, AL) hipLaunchKernelGGL((pointwise_time_kernel<BF, V, AL>), dim3(g), dim3(256), 0, st, x, t, y, ldj, ldiag, n_rows, dim, \
                                             kind, param, ldj_mode, ldj_accumulate)
    sx_dispatch(ldj_mode == 2, [&](auto AL) {
        if (vec == 8) PWT_GO(true, 8, AL());
        else if (dtype == SX_BF16) { if (vec == 4) PWT_GO(true, 4, AL()); else PWT_GO(true, 1, AL()); }
        else { if (vec == 4) PWT_GO(false, 4, AL()); else PWT_GO(false, 1, AL()); }
    });
#undef PWT_GO
    SX_LAUNCH_CHECK();
    return SX_OK;
}
