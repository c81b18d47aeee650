// Exact-trace continuous normalizing flow (ContinuousTransform with divergence='exact' over net.DiffeqExactTraceMLP; reference:
// stribor/net/diffeq_exact_trace.py:48-72, diffeq_zero_trace.py:14-56, made.py, diagjac.py) on a fixed grid, in one launch per call.
//
// sx_cnf_exact_flow -- the solve dx/dt = f(t, x, latent) with
//     h     = MADE_1(x) + MADE_2(x)                   the exclusive net: d_h values per dimension, dh_i/dx_i = 0
//     f_i   = g(t, x_i, h_i, latent)                  the dimwise net g: one MLP shared by every dimension
//     jac_i = dg/dx_i at fixed h_i                    = df_i/dx_i exactly, because the Jacobian of h is hollow
// from t0 to t1 by euler / midpoint / rk4 (the 3/8 rule) over the grid of sx_cnf_flow, with the log-det = the integral of
// sum_i jac_i under the same tableau.  The solver, its order of roundings and the exact-fp32 MFMA product are sx_cnf_common.h's:
//   * one wave = 32 rows on the MFMA column (lane & 31); the state, the stage vectors, h, every activation and the per-row log-det
//     stay in registers for the whole grid;
//   * the caller hands over ONE image of everything the kernel keeps in LDS (sx_cnf_exact_net.image): mask * weight of both MADEs,
//     the dimwise weights, the biases -- already in A-fragment order (the tile image of sx_cnf_common.h's cnf_stage) and already in the
//     kernel's feature POSITIONS, so staging is a straight copy and the kernel never sees a mask or an index table:
//       state      dimension i            at position kmap(i, 0): register i of the lower lane half (the upper half stays 0)
//       h          (slot kk, dimension i) at tile kk >> 1, position kmap(i, kk & 1): register i holds the slot pair (2c, 2c + 1) of
//                                         dimension i in the two lane halves -- one MFMA k-pair of the dimwise first layer
//       dimwise in x_i at k-pair 0 (lower half), slots (2c, 2c + 1) at k-pair 1 + c
//     so "dimension i of a tile" is register i of that tile: a select chain on the wave-uniform i, no LDS transpose, no shuffle;
//   * per evaluation: both MADEs (their last layers accumulate into the same h tiles), then a loop over the dimensions i < D: the
//     dimwise MLP on [x_i, h_i] with the tangent d/dx_i beside the value (tau_1 = act'(z_1) * W1[:, x], tau_2 = act'(z_2) * (W2
//     tau_1): the same A fragments, a second B operand), the one-row last layer as a dot product on the VALU;
//   * time is uniform over rows (b1 + t_stage * W1[:, 0]); the latent columns' share of the dimwise first layer is the same for every
//     dimension and every stage: one GEMM per row group before the grid loop, A fragments from global memory;
//   * a call without a log-det (want_ldj == 0) skips the tangent.
//
// The MADE, the dimwise loop, the solve of a row group, the plan pieces and the host checks are sx_cnf_exact_common.h's, shared with
// sx_cnf_exact_set.hip; this file keeps the evaluation (two MADEs, then the dimwise net), the kernel's row groups and the entry points.
//
// Coverage: dim <= 16, d_h <= 8, latent_dim <= 64, one or two hidden layers of <= 64 units (the same widths in the two MADEs and the
// dimwise net), activations Identity .. LeakyReLU.  The largest image (two hidden layers of 64, d_h = 8) is 137 KiB.
#include "sx_cnf_exact_common.h"

namespace {

// the LDS image: float offsets (sx_cnf_exact_net.image is laid out in this order; net/diffeq_exact_trace.py builds it)
struct cx_plan {
    cnf_exact_made made[2];
    cnf_exact_dimwise dw;
    int total;
};

__host__ __device__ constexpr cx_plan cx_make_plan(int HT, int NH, int OT) {
    cx_plan p{};
    int off = 0;
    p.made[0] = cnf_exact_plan_made(off, HT, NH, OT);
    p.made[1] = cnf_exact_plan_made(off, HT, NH, OT);
    p.dw = cnf_exact_plan_dimwise(off, HT, NH);
    p.total = off;
    return p;
}

struct cx_args : cnf_exact_args<sx_cnf_exact_net> {};

// f(t, x) -> k (dimension i at register i of the lower lane half) and -- when `want` -- tr = sum_i jac_i, for the wave's 32 rows
template <int HT, int NH, int OT>
__device__ __forceinline__ void cx_eval(const cx_args &a, const f32x16 &xin, float t, const cnf_tile<HT> &lat, f32x16 &k, bool want, float &tr,
                                        int lane) {
    constexpr cx_plan p = cx_make_plan(HT, NH, OT);
    const int act = a.net.act;
    // the image never changes: without this the compiler hoists its loads out of the step loop and holds matrices in registers
    asm volatile("" ::: "memory");
    // ---- the exclusive net: both MADEs, their last layers summed into `raw` ----
    cnf_tile<OT> raw;
#pragma unroll
    for (int m = 0; m < OT; ++m) raw.v[m] = f32x16{};
    cnf_tile<1> xi;
    xi.v[0] = xin;
    cnf_exact_made_eval<HT, NH, OT>(p.made[0], xi, raw, act, lane);
    cnf_exact_made_eval<HT, NH, OT>(p.made[1], xi, raw, act, lane);
    // ---- the dimwise net, one dimension at a time ----
    cnf_exact_dimwise_eval<HT, NH, OT>(p.dw, act, a.net.dim, xin, raw, t, lat, k, want, tr, lane);
}

template <int HT, int NH, int OT>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_exact_kernel(const cx_args a) {
    constexpr cx_plan p = cx_make_plan(HT, NH, OT);
    cnf_stage_image(a.net.image, p.total);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, D = a.net.dim, L = a.net.latent_dim;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_CNF_WAVES + (threadIdx.x >> 6); grp < n_groups;
         grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        CNF_EXACT_SOLVE_ROWS(HT, a, row, live, h, D, L, want, sgn, lane, cx_eval<HT, NH, OT>(a, xs.v[0], ts, lat, k.v[0], want, q, lane))
    }
}

int cx_check_net(const sx_cnf_exact_net *net_host) {
    return cnf_exact_check_net("sx_cnf_exact_flow", net_host, SX_CNF_EXACT_MAX_DIM, SX_CNF_EXACT_MAX_DH, SX_CNF_EXACT_MAX_LATENT,
                               SX_CNF_EXACT_MAX_HIDDEN);
}

}  // namespace

extern "C" size_t sx_cnf_exact_lds_bytes(const sx_cnf_exact_net *net_host) {
    if (cx_check_net(net_host) != SX_OK) return 0;
    int HT, OT;
    cnf_exact_shape(*net_host, &HT, &OT);
    return (size_t)cx_make_plan(HT, net_host->n_hidden, OT).total * 4;
}

extern "C" int sx_cnf_exact_flow(const sx_cnf_exact_net *net_host, const float *x, const float *latent, float *y, float *ldj, int64_t n_rows,
                                 int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj, void *stream) {
    const char *fn = "sx_cnf_exact_flow";
    int rc = cx_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_net &net = *net_host;
    rc = cnf_check_call(fn, solver, n_rows, 1, n_steps, step_size, x, y);
    if (rc != SX_OK) return rc;
    int HT, OT;
    cnf_exact_shape(net, &HT, &OT);
    const int NH = net.n_hidden;
    const size_t image = (size_t)cx_make_plan(HT, NH, OT).total, lds = image * 4;
    rc = cnf_exact_check_flow(fn, net, latent, ldj, want_ldj, image, lds, "the image needs");
    if (rc != SX_OK || n_rows == 0) return rc;
    const cx_args a = cnf_exact_fill<cx_args>(net, x, latent, y, ldj, n_rows, solver, n_steps, t0, t1, step_size, want_ldj);
    CNF_EXACT_DISPATCH(cnf_exact_kernel, fn, HT, NH, OT, a, lds, cnf_row_blocks(n_rows), stream);
}
