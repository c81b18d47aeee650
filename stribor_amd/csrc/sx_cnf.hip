// Continuous normalizing flow (ContinuousTransform, stribor/flows/cnf.py:13-262, with net/diffeq.py's DiffeqMLP) on a fixed grid,
// in one launch per call.
//
// sx_cnf_flow -- the solve dx/dt = f(t, x, latent), f = MLP([t, x, latent]) with one or two hidden layers and no final
// activation, from t0 to t1 by euler / midpoint / rk4 (the 3/8 rule) over the grid of DESIGN.md "CNF", together with the exact
// divergence tr df/dx and its integral (the log-det):
//   * one wave = 32 rows, laid out as in sx_resnet.hip: rows on the MFMA column (lane & 31), features on the C rows, a 32-feature
//     tile of a row = one f32x16 C fragment = the B operand of the next GEMM.  The state, every stage vector, the hidden
//     activations and the per-row log-det accumulator stay in registers for the whole grid;
//   * the x columns of W1 and the later layers are staged into LDS once per workgroup (A-fragment order, zero-padded to tiles of
//     32, the layer image of sx_resnet.hip); the workgroup then walks its 32-row groups;
//   * time is uniform over rows: per stage the first layer's bias is b1 + t_stage * W1[:, 0];
//   * the latent columns are constant along the solve: W1[:, latent] . latent_row is one GEMM per row group before the loop (its
//     A fragments come straight from global memory: once per group, no LDS spent on it);
//   * the trace (d_l = act'(hidden layer l), W1x = the x columns of W1):
//       one hidden layer   tr J = sum_j d1_j c_j,           c_j = sum_i W2[i, j] W1x[j, i]
//       two hidden layers  tr J = d2^T C d1,                 C[k, j] = W2[k, j] (W1x W3)[j, k]     (one extra H2 x H1 GEMM)
//     c / C depend on the weights only and are passed in (fp32, derived in fp64 by the caller).  c and -- where the LDS budget
//     allows -- C sit in LDS beside the weights; a C that does not fit (two hidden layers of 128 units) is read from global
//     memory (L2-resident: 64 KiB shared by every wave);
//   * arithmetic: exact fp32, v_mfma_f32_32x32x2_f32, library tanhf / expf; unfused multiply-adds in the tableau (the file is
//     compiled with -ffp-contract=off) so a step is the reference solver's sequence of roundings.  set_gemm_precision is ignored.
//
// Coverage: dim <= 64 (<= 32 with two hidden layers wider than 64 units: that kernel would spill), 1 + dim + latent_dim <= 128,
// one or two hidden layers of <= 128 units, activations Identity / Tanh /
// ReLU / Sigmoid / ELU / Softplus / LeakyReLU (the ones whose derivative is a function of the activation's OUTPUT).
//
// The hidden layers, the output layer, the activation sweep, the network validator and the plan of the forward images are
// sx_cnf_dense.h's, shared with sx_cnf_train.hip; this file's own are the trace and its constants in LDS.  The staging, the row load
// and store and the latent GEMM are written out in cnf_flow_kernel, not taken from that header's functions, and the hidden and
// output layers are expanded as its macros: cnf_flow_kernel<1, 4, 2> uses every register there is, any other form of these
// statements allocates it differently, and each form tried cost dim 32 / [128, 128] 0.2 .. 0.8 % (29.18 ms for 29.01, 18.73 for 18.58).
#include "sx_cnf_dense.h"

namespace {

struct cn_args : cnf_dense_args {
    int base_tr;            // LDS float offset of c (one hidden layer) or C (two, when c_in_lds)
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int64_t n_rows;
    int solver, n_steps, want_ldj, c_in_lds;
    float t0, t1, step_size;
};

// f(t, x) and -- when `want` -- tr = tr df/dx for the wave's 32 rows
template <int DT, int HT, int NH>
__device__ __forceinline__ void cn_eval(const cn_args &a, const cnf_tile<DT> &xin, float t, const cnf_tile<HT> &lat, cnf_tile<DT> &k, bool want, float &tr,
                                        int lane) {
    const int h = lane >> 5, act = a.net.act;
    cnf_tile<HT> h1;
    CNF_DENSE_H1(DT, HT, false, a, xin, t, lat, h1, lane, h, act);
    float s = 0.f;
    if (NH == 1) {
        if (want) {
            const float *cv = cnf_smem + a.base_tr + 4 * h;
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                f32x16 d = h1.v[m];
                if (act != SX_ACT_IDENTITY) cnf_dact_tile(d, act);
                else d = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
#pragma unroll
                for (int r = 0; r < 16; ++r) s += d[r] * cnf_vec(cv, m, r);
            }
        }
        CNF_DENSE_OUT(DT, HT, 1, a, h1, k, lane, h);
    } else {
        cnf_tile<HT> h2;
        CNF_DENSE_H2(HT, false, a, h1, h2, lane, h, act);
        if (want) {
            // h1 <- d1, v = C d1, s = d2 . v
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                if (act != SX_ACT_IDENTITY) cnf_dact_tile(h1.v[m], act);
                else h1.v[m] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
            }
            // v = C d1 one 32-row tile at a time, consumed at once: s += d2 . v
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                f32x16 v = {};
                if (a.c_in_lds) cnf_mma<HT>(v, h1, cnf_smem + a.base_tr + m * HT * 1024 + lane * 4);
                else cnf_mma_global<HT>(v, h1, a.net.trace + (int64_t)m * 32 * (HT * 32), lane);
                f32x16 d = h2.v[m];
                if (act != SX_ACT_IDENTITY) cnf_dact_tile(d, act);
                else d = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
#pragma unroll
                for (int r = 0; r < 16; ++r) s += d[r] * v[r];
            }
        }
        asm volatile("" ::: "memory");
        CNF_DENSE_OUT(DT, HT, 2, a, h2, k, lane, h);
    }
    if (want) tr = s + __shfl_xor(s, 32, 64);          // the two lane halves hold the two feature halves of a row
}

template <int DT, int HT, int NH>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_flow_kernel(const cn_args a) {
    const sx_cnf_net &net = a.net;
    const int D = net.dim, L = net.latent_dim, in_dim = 1 + D + L, H1 = net.layer[0].out_dim;
    cnf_stage(net.layer[0].W, H1, D, in_dim, 1, HT, DT, a.base_w[0]);
    cnf_stage_vec(net.layer[0].b, H1, 1, HT * 32, a.base_b[0]);
    cnf_stage_vec(net.layer[0].W, H1, in_dim, HT * 32, a.base_w0);
    if (NH == 1) {
        cnf_stage(net.layer[1].W, D, H1, H1, 0, DT, HT, a.base_w[1]);
        cnf_stage_vec(net.layer[1].b, D, 1, DT * 32, a.base_b[1]);
        cnf_stage_vec(a.want_ldj ? net.trace : nullptr, H1, 1, HT * 32, a.base_tr);
    } else {
        const int H2 = net.layer[1].out_dim;
        cnf_stage(net.layer[1].W, H2, H1, H1, 0, HT, HT, a.base_w[1]);
        cnf_stage_vec(net.layer[1].b, H2, 1, HT * 32, a.base_b[1]);
        cnf_stage(net.layer[2].W, D, H2, H2, 0, DT, HT, a.base_w[2]);
        cnf_stage_vec(net.layer[2].b, D, 1, DT * 32, a.base_b[2]);
        if (a.want_ldj && a.c_in_lds) cnf_stage(net.trace, HT * 32, HT * 32, HT * 32, 0, HT, HT, a.base_tr);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_CNF_WAVES + (threadIdx.x >> 6); grp < n_groups;
         grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        cnf_tile<DT> y;
#pragma unroll
        for (int c = 0; c < DT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * c + sx_kmap(r, h);
                y.v[c][r] = (live && f < D) ? a.x[row * D + f] : 0.f;
            }
        // the latent share of the first layer: W1[:, 1 + D ..] . latent_row, once per row
        cnf_tile<HT> lat;
#pragma unroll
        for (int m = 0; m < HT; ++m) lat.v[m] = f32x16{};
        if (L > 0) {
            const float *W1 = net.layer[0].W;
            for (int c = 0; c < (L + 31) >> 5; ++c) {
                f32x16 lb;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * c + sx_kmap(r, h);
                    lb[r] = (live && f < L) ? a.latent[row * L + f] : 0.f;
                }
#pragma unroll
                for (int m = 0; m < HT; ++m) {
                    const int wr = 32 * m + (lane & 31);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int f = 32 * c + sx_kmap(q, h);
                        const float av = (wr < H1 && f < L) ? W1[(int64_t)wr * in_dim + 1 + D + f] : 0.f;
                        lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, lb[q], lat.v[m], 0, 0, 0);
                    }
                }
            }
        }
        float l = 0.f;
        const int n_stages = cnf_stages(a.solver);
        const float third = 1.f / 3.f, two_thirds = 2.f / 3.f;
        for (int i = 0; i < a.n_steps; ++i) {
            float ta, tb;
            cnf_grid(a, sgn, i, ta, tb);
            const float dt = tb - ta, half = 0.5f * dt;
            cnf_tile<DT> k1, k2, xs = y;          // (rk4: after stage 3, k1 holds k1 + 3 (k2 + k3))
            float q1 = 0.f, q2 = 0.f, ts = ta;
            // one copy of the network's code serves every stage: the stage index is wave-uniform
            for (int st = 0; st < n_stages; ++st) {
                cnf_tile<DT> k;
                float q = 0.f;
                cn_eval<DT, HT, NH>(a, xs, ts, lat, k, want, q, lane);
                cnf_tableau<DT>(a.solver, st, ta, tb, dt, half, third, two_thirds, k, q, k1, k2, q1, q2, xs, ts, y, l);
            }
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * c + sx_kmap(r, h);
                    if (f < D) a.y[row * D + f] = y.v[c][r];
                }
            if (want && h == 0) a.ldj[row] = l;
        }
    }
}

// the LDS plan: the forward images, then c / C.  C goes into LDS when it fits beside the rest.  -> floats used
size_t cn_plan(const sx_cnf_net &net, int want_ldj, cn_args &a) {
    const int NH = net.n_layers - 1, HT = cnf_dense_hidden_tiles(net);
    size_t off = cnf_dense_plan(net, a);
    a.base_tr = (int)off;
    a.c_in_lds = 1;
    if (NH == 1) off += (size_t)HT * 32;
    else if (want_ldj) {
        const size_t c_floats = (size_t)HT * HT * 1024;
        if ((off + c_floats) * 4 <= SX_CNF_LDS_BYTES) off += c_floats;
        else a.c_in_lds = 0;
    }
    return off;
}

int cn_check_net(const sx_cnf_net *net_host) {
    const int rc = cnf_dense_check_net("sx_cnf_flow", net_host, SX_CNF_MAX_DIM, 128, 128);
    if (rc != SX_OK) return rc;
    const sx_cnf_net &net = *net_host;
    // two hidden layers of four tiles beside a two-tile state do not fit the register file (the build would spill): not offered
    SX_REQUIRE(!(net.n_layers == 3 && net.dim > 32 && (net.layer[0].out_dim > 64 || net.layer[1].out_dim > 64)),
               "sx_cnf_flow: two hidden layers wider than 64 units need dim <= 32 (got dim %d)", net.dim);
    return SX_OK;
}

}  // namespace

extern "C" size_t sx_cnf_lds_bytes(const sx_cnf_net *net_host, int32_t want_ldj) {
    if (cn_check_net(net_host) != SX_OK) return 0;
    cn_args a{};
    return cn_plan(*net_host, want_ldj, a) * 4;
}

extern "C" int sx_cnf_flow(const sx_cnf_net *net_host, const float *x, const float *latent, float *y, float *ldj, int64_t n_rows,
                           int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj, void *stream) {
    const int rc = cn_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_net &net = *net_host;
    const int rc_call = cnf_check_call("sx_cnf_flow", solver, n_rows, 1, n_steps, step_size, x, y);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "sx_cnf_flow: latent rows missing");
    SX_REQUIRE(!want_ldj || (ldj != nullptr && net.trace != nullptr), "sx_cnf_flow: want_ldj needs ldj and the trace constants");
    cn_args a{};
    a.net = net;
    const size_t lds = cn_plan(net, want_ldj ? 1 : 0, a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_flow: the padded weights need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.want_ldj = want_ldj ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    const int DT = cnf_tiles(net.dim), NH = net.n_layers - 1, HT = cnf_dense_hidden_tiles(net);
    const int64_t want = cnf_row_blocks(n_rows);
#define CN_CASE(D_, H_)                                                                                  \
    if (DT == D_ && HT == H_)                                                                            \
        return NH == 1 ? cnf_launch<cnf_flow_kernel<D_, H_, 1>>("sx_cnf_flow", a, lds, want, stream)     \
                       : cnf_launch<cnf_flow_kernel<D_, H_, 2>>("sx_cnf_flow", a, lds, want, stream);
    CN_CASE(1, 1) CN_CASE(1, 2) CN_CASE(1, 4) CN_CASE(2, 1) CN_CASE(2, 2)
#undef CN_CASE
    if (DT == 2 && HT == 4 && NH == 1) return cnf_launch<cnf_flow_kernel<2, 4, 1>>("sx_cnf_flow", a, lds, want, stream);
    sx_set_error("sx_cnf_flow: no kernel for %d x %d tiles", DT, HT);
    return SX_E_BADARG;
}
