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
// Coverage: dim <= 16, d_h <= 8, latent_dim <= 64, one or two hidden layers of <= 64 units (the same widths in the two MADEs and the
// dimwise net), activations Identity .. LeakyReLU.  The largest image (two hidden layers of 64, d_h = 8) is 137 KiB.
#include "sx_cnf_common.h"

namespace {

// the LDS image: float offsets (sx_cnf_exact_net.image is laid out in this order; net/diffeq_exact_trace.py builds it)
struct cx_plan {
    int ew[2][3], eb[2][3];       // MADE e: first layer, (second hidden layer,) last layer -- images and biases
    int dw1, db1, dw0, dwx;       // dimwise first layer: image, bias, the time column, the x column (the tangent's seed)
    int dw2, db2;                 // two hidden layers: the second
    int dwl, dbl;                 // the last layer as a vector over the hidden positions; its bias (1 float, padded to 32)
    int total;
};

__host__ __device__ constexpr cx_plan cx_make_plan(int HT, int NH, int OT) {
    cx_plan p{};
    int off = 0;
    for (int e = 0; e < 2; ++e) {
        p.ew[e][0] = off; off += HT * 1024;
        p.eb[e][0] = off; off += HT * 32;
        if (NH == 2) {
            p.ew[e][1] = off; off += HT * HT * 1024;
            p.eb[e][1] = off; off += HT * 32;
        }
        p.ew[e][2] = off; off += OT * HT * 1024;
        p.eb[e][2] = off; off += OT * 32;
    }
    p.dw1 = off; off += HT * 1024;
    p.db1 = off; off += HT * 32;
    p.dw0 = off; off += HT * 32;
    p.dwx = off; off += HT * 32;
    if (NH == 2) {
        p.dw2 = off; off += HT * HT * 1024;
        p.db2 = off; off += HT * 32;
    }
    p.dwl = off; off += HT * 32;
    p.dbl = off; off += 32;
    p.total = off;
    return p;
}

struct cx_args {
    sx_cnf_exact_net net;
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int64_t n_rows;
    int solver, n_steps, want_ldj;
    float t0, t1, step_size;
};

// MADE E of the exclusive net: raw += W_last . hidden(x) + b_last
template <int HT, int NH, int OT, int E>
__device__ __forceinline__ void cx_made(const cnf_tile<1> &xi, cnf_tile<OT> &raw, int act, int lane) {
    constexpr cx_plan p = cx_make_plan(HT, NH, OT);
    const int h = lane >> 5;
    cnf_tile<HT> h1;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        h1.v[m] = f32x16{};
        cnf_mma<1>(h1.v[m], xi, cnf_smem + p.ew[E][0] + m * 1024 + lane * 4);
    }
    cnf_add_vec<HT>(h1, cnf_smem + p.eb[E][0] + 4 * h);
    cnf_act_all<HT>(h1, act);
    if (NH == 2) {
        cnf_tile<HT> h2;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            h2.v[m] = f32x16{};
            cnf_mma<HT>(h2.v[m], h1, cnf_smem + p.ew[E][1] + m * HT * 1024 + lane * 4);
        }
        cnf_add_vec<HT>(h2, cnf_smem + p.eb[E][1] + 4 * h);
        cnf_act_all<HT>(h2, act);
        h1 = h2;
    }
#pragma unroll
    for (int m = 0; m < OT; ++m) cnf_mma<HT>(raw.v[m], h1, cnf_smem + p.ew[E][2] + m * HT * 1024 + lane * 4);
    cnf_add_vec<OT>(raw, cnf_smem + p.eb[E][2] + 4 * h);
    asm volatile("" ::: "memory");
}

// f(t, x) -> k (dimension i at register i of the lower lane half) and -- when `want` -- tr = sum_i jac_i, for the wave's 32 rows
template <int HT, int NH, int OT>
__device__ __forceinline__ void cx_eval(const cx_args &a, const f32x16 &xin, float t, const cnf_tile<HT> &lat, f32x16 &k, bool want, float &tr,
                                        int lane) {
    constexpr cx_plan p = cx_make_plan(HT, NH, OT);
    const int h = lane >> 5, act = a.net.act, D = a.net.dim;
    // the image never changes: without this the compiler hoists its loads out of the step loop and holds matrices in registers
    asm volatile("" ::: "memory");
    // ---- the exclusive net: both MADEs, their last layers summed into `raw` ----
    cnf_tile<OT> raw;
#pragma unroll
    for (int m = 0; m < OT; ++m) raw.v[m] = f32x16{};
    cnf_tile<1> xi;
    xi.v[0] = xin;
    cx_made<HT, NH, OT, 0>(xi, raw, act, lane);
    cx_made<HT, NH, OT, 1>(xi, raw, act, lane);
    // ---- the dimwise net, one dimension at a time ----
    const float *b1 = cnf_smem + p.db1 + 4 * h, *w0 = cnf_smem + p.dw0 + 4 * h, *wx = cnf_smem + p.dwx + 4 * h;
    const float *wl = cnf_smem + p.dwl + 4 * h;
    const float bl = cnf_smem[p.dbl];
    float s = 0.f;
    k = f32x16{};
#pragma unroll 1
    for (int i = 0; i < D; ++i) {
        asm volatile("" ::: "memory");
        const float x_i = cnf_pick(xin, i);
        float hs[OT];
#pragma unroll
        for (int c = 0; c < OT; ++c) hs[c] = cnf_pick(raw.v[c], i);
        cnf_tile<HT> a1;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            const float *wb = cnf_smem + p.dw1 + m * 1024 + lane * 4;
            const f32x4 w = *reinterpret_cast<const f32x4 *>(wb);
            f32x16 acc = {};
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, x_i, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, hs[0], acc, 0, 0, 0);
            if (OT > 1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, hs[OT > 1 ? 1 : 0], acc, 0, 0, 0);
            if (OT > 2) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, hs[OT > 2 ? 2 : 0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[256], hs[OT > 2 ? 3 : 0], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = (acc[r] + lat.v[m][r]) + (cnf_vec(b1, m, r) + t * cnf_vec(w0, m, r));
            a1.v[m] = acc;
        }
        cnf_act_all<HT>(a1, act);
        float f = 0.f, j = 0.f;
        if (NH == 1) {
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float w = cnf_vec(wl, m, r);
                    f += w * a1.v[m][r];
                    if (want) j += w * (cnf_dact(a1.v[m][r], act) * cnf_vec(wx, m, r));
                }
        } else {
            const float *b2 = cnf_smem + p.db2 + 4 * h;
            cnf_tile<HT> a2;
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                a2.v[m] = f32x16{};
                cnf_mma<HT>(a2.v[m], a1, cnf_smem + p.dw2 + m * HT * 1024 + lane * 4);
            }
            cnf_add_vec<HT>(a2, b2);
            cnf_act_all<HT>(a2, act);
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) f += cnf_vec(wl, m, r) * a2.v[m][r];
            if (want) {
                // a1 <- tau_1, u = W2 tau_1 one tile at a time, consumed at once: j += w_last . (act'(z_2) * u)
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) a1.v[m][r] = cnf_dact(a1.v[m][r], act) * cnf_vec(wx, m, r);
#pragma unroll
                for (int m = 0; m < HT; ++m) {
                    f32x16 u = {};
                    cnf_mma<HT>(u, a1, cnf_smem + p.dw2 + m * HT * 1024 + lane * 4);
#pragma unroll
                    for (int r = 0; r < 16; ++r) j += cnf_vec(wl, m, r) * (cnf_dact(a2.v[m][r], act) * u[r]);
                }
            }
        }
        // the two lane halves hold the two halves of the hidden positions of a row
        f = (f + __shfl_xor(f, 32, 64)) + bl;
        if (want) s += j + __shfl_xor(j, 32, 64);
        const float fi = h == 0 ? f : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) k[r] = (i == r) ? fi : k[r];
    }
    if (want) tr = s;
}

template <int HT, int NH, int OT>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_exact_kernel(const cx_args a) {
    const sx_cnf_exact_net &net = a.net;
    constexpr cx_plan p = cx_make_plan(HT, NH, OT);
    cnf_stage_image(net.image, p.total);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, D = net.dim, L = net.latent_dim;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_CNF_WAVES + (threadIdx.x >> 6); grp < n_groups;
         grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        cnf_tile<1> y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y.v[0][r] = (live && h == 0 && r < D) ? a.x[row * D + r] : 0.f;
        cnf_tile<HT> lat;
        cnf_latent_packed<HT>(lat, net.w_latent, a.latent, row, live, L, lane);
        float l = 0.f;
        const int n_stages = cnf_stages(a.solver);
        const float third = 1.f / 3.f, two_thirds = 2.f / 3.f;
        for (int i = 0; i < a.n_steps; ++i) {
            float ta, tb;
            cnf_grid(a, sgn, i, ta, tb);
            const float dt = tb - ta, half = 0.5f * dt;
            cnf_tile<1> k1, k2, xs = y;
            float q1 = 0.f, q2 = 0.f, ts = ta;
            // one copy of the network's code serves every stage: the stage index is wave-uniform
            for (int st = 0; st < n_stages; ++st) {
                cnf_tile<1> k;
                float q = 0.f;
                cx_eval<HT, NH, OT>(a, xs.v[0], ts, lat, k.v[0], want, q, lane);
                cnf_tableau<1>(a.solver, st, ta, tb, dt, half, third, two_thirds, k, q, k1, k2, q1, q2, xs, ts, y, l);
            }
        }
        if (live && h == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (r < D) a.y[row * D + r] = y.v[0][r];
            if (want) a.ldj[row] = l;
        }
    }
}

int cx_check_net(const sx_cnf_exact_net *net_host) {
    SX_REQUIRE(net_host != nullptr, "sx_cnf_exact_flow: null network");
    const sx_cnf_exact_net &net = *net_host;
    SX_REQUIRE(net.n_hidden == 1 || net.n_hidden == 2, "sx_cnf_exact_flow: one or two hidden layers (got %d)", net.n_hidden);
    SX_REQUIRE(net.dim >= 1 && net.dim <= SX_CNF_EXACT_MAX_DIM, "sx_cnf_exact_flow: dim must be in 1..%d (got %d)", SX_CNF_EXACT_MAX_DIM, net.dim);
    SX_REQUIRE(net.d_h >= 1 && net.d_h <= SX_CNF_EXACT_MAX_DH, "sx_cnf_exact_flow: d_h must be in 1..%d (got %d)", SX_CNF_EXACT_MAX_DH, net.d_h);
    SX_REQUIRE(net.latent_dim >= 0 && net.latent_dim <= SX_CNF_EXACT_MAX_LATENT, "sx_cnf_exact_flow: latent_dim must be in 0..%d (got %d)",
               SX_CNF_EXACT_MAX_LATENT, net.latent_dim);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "sx_cnf_exact_flow: activation %d has no in-kernel derivative", net.act);
    for (int l = 0; l < net.n_hidden; ++l)
        SX_REQUIRE(net.hidden[l] >= 1 && net.hidden[l] <= SX_CNF_EXACT_MAX_HIDDEN, "sx_cnf_exact_flow: hidden layer %d must have 1..%d units (got %d)",
                   l, SX_CNF_EXACT_MAX_HIDDEN, net.hidden[l]);
    return SX_OK;
}

inline void cx_shape(const sx_cnf_exact_net &net, int *HT, int *OT) {
    int ht = cnf_tiles(net.hidden[0]);
    if (net.n_hidden == 2 && cnf_tiles(net.hidden[1]) > ht) ht = cnf_tiles(net.hidden[1]);
    *HT = ht;
    *OT = cnf_out_tiles(net.d_h);
}

}  // namespace

extern "C" size_t sx_cnf_exact_lds_bytes(const sx_cnf_exact_net *net_host) {
    if (cx_check_net(net_host) != SX_OK) return 0;
    int HT, OT;
    cx_shape(*net_host, &HT, &OT);
    return (size_t)cx_make_plan(HT, net_host->n_hidden, OT).total * 4;
}

extern "C" int sx_cnf_exact_flow(const sx_cnf_exact_net *net_host, const float *x, const float *latent, float *y, float *ldj, int64_t n_rows,
                                 int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj, void *stream) {
    const int rc = cx_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_net &net = *net_host;
    const int rc_call = cnf_check_call("sx_cnf_exact_flow", solver, n_rows, 1, n_steps, step_size, x, y);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || (latent != nullptr && net.w_latent != nullptr), "sx_cnf_exact_flow: latent rows / latent weights missing");
    SX_REQUIRE(!want_ldj || ldj != nullptr, "sx_cnf_exact_flow: want_ldj needs ldj");
    int HT, OT;
    cx_shape(net, &HT, &OT);
    const int NH = net.n_hidden;
    const size_t lds = (size_t)cx_make_plan(HT, NH, OT).total * 4;
    SX_REQUIRE(net.image != nullptr && (size_t)net.image_floats * 4 == lds, "sx_cnf_exact_flow: the image holds %d floats, the kernel's plan %zu",
               net.image_floats, lds / 4);
    SX_REQUIRE(((uintptr_t)net.image & 15) == 0 && ((uintptr_t)net.w_latent & 15) == 0, "sx_cnf_exact_flow: image / w_latent must be 16-byte aligned");
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_exact_flow: the image needs %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    cx_args a{};
    a.net = net;
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.want_ldj = want_ldj ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    const int64_t want = cnf_row_blocks(n_rows);
#define CX_CASE(H_, O_)                                                                                \
    if (HT == H_ && OT == O_)                                                                            \
        return NH == 1 ? cnf_launch<cnf_exact_kernel<H_, 1, O_>>("sx_cnf_exact_flow", a, lds, want, stream) \
                       : cnf_launch<cnf_exact_kernel<H_, 2, O_>>("sx_cnf_exact_flow", a, lds, want, stream);
    CX_CASE(1, 1) CX_CASE(1, 2) CX_CASE(1, 4) CX_CASE(2, 1) CX_CASE(2, 2) CX_CASE(2, 4)
#undef CX_CASE
    sx_set_error("sx_cnf_exact_flow: no kernel for %d hidden x %d output tiles", HT, OT);
    return SX_E_BADARG;
}
