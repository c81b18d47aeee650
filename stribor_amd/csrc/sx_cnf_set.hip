// Continuous normalizing flow over SETS (ContinuousTransform with set_data / 'compute_set', stribor/flows/cnf.py:13-262, over
// net/diffeq.py:78-94's DiffeqDeepset = DiffeqConcat around net/equivariant.py's EquivariantNet) on a fixed grid, in one launch.
//
// sx_cnf_set_flow -- rows are set elements, the N = set_size elements of a set contiguous.  Layer l of the net is
//     z_l,i = A_l h_i + G_l sum_j h_j + bias_l,     G_l = B_l / N,  bias_l = a_l + b_l / N     (A = l1, B = l2; j over the set)
// and the divergence of the whole set's dynamics, per element, has the closed form of DESIGN.md "CNF on sets" (d_l = act'(hidden
// layer l), s_l = sum_j d_l,j):
//     one hidden layer   tr_i = d1_i . c_d + sum_j d1_j . c_s
//     two hidden layers  tr_i = d2_i^T (C_abd d1_i + C_c s1) + s2^T (C_f d1_i + C_g s1) + sum_j d2_j^T C_e d1_j
// with weight-only constants passed in (fp32, derived in fp64 by the caller).
//   * the conventions of sx_cnf_common.h: one wave = 32 rows on the MFMA column, features on the C rows, exact fp32
//     (v_mfma_f32_32x32x2_f32), weights in LDS in A-fragment order, state / stage vectors / log-det in registers for the whole grid,
//     the same solvers, grid, tableau roundings (-ffp-contract=off) and activations;
//   * a workgroup of 4 waves owns 128 row slots and takes floor(128 / N) WHOLE sets per pass: sets never straddle workgroups, they
//     may straddle waves.  Slots past the last set are padding: they compute on zeros and are never stored;
//   * a set sum is sx_cnf_common.h's cnf_setsum through an LDS scratch [128][32 HT + 4], its additions in row order.  Every wave
//     reaches its three barriers (padding waves included) because the pass loop, the stage loop and `want` are uniform over the
//     workgroup;
//   * per evaluation the sums taken are: x, h1(, h2) for the l2 branches, and for the trace d1 and d2 (two hidden layers; the scalar
//     sum_j d2_j^T C_e d1_j rides with d2) or one scalar riding with h1 (one hidden layer);
//   * time: per stage the first layer's bias is bias_1 + t_stage (A1[:, 0] + B1[:, 0]); the latent columns of A1 and G1 are constant
//     along the solve: one GEMM pair per pass before the loop, A fragments straight from global memory;
//   * LDS: A and G images of every layer, the small vectors, the scratch, and as many of the five C matrices (order abd, c, e, f, g)
//     as still fit SX_CNF_LDS_BYTES; the others are read from global memory (row-major, zero-padded: 16 KiB each, L2-resident).
//
// Coverage: 1 <= N <= 128, dim <= 32, 1 + dim + latent_dim <= 64, one or two hidden layers of <= 64 units, the seven activations of
// sx_cnf_common.h, no final activation, no mask.
#include "sx_cnf_common.h"

namespace {

struct cs_args {
    sx_cnf_set_net net;
    int base_a[3], base_g[3], base_b[3];          // LDS float offsets of the A / G images and the biases
    int base_w0;                                  // ... of the time column
    int base_tr;                                  // ... of c_d, c_s (one hidden layer) or the first n_c_lds C images (two)
    int base_x;                                   // ... of the exchange scratch [SX_CNF_ROWS][32 HT + 4]
    int n_c_lds;
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int64_t n_rows;
    int solver, n_steps, want_ldj;
    float t0, t1, step_size;
};

// acc += (rows 32m .. 32m + 31 of C matrix `ci`) . in
template <int HT>
__device__ __forceinline__ void cs_mma_c(f32x16 &acc, const cnf_tile<HT> &in, const cs_args &a, int ci, int m, int lane) {
    if (ci < a.n_c_lds) cnf_mma<HT>(acc, in, cnf_smem + a.base_tr + (ci * HT + m) * HT * 1024 + lane * 4);
    else cnf_mma_global<HT>(acc, in, a.net.trace + ((int64_t)ci * HT + m) * 32 * (HT * 32), lane);
}

__device__ __forceinline__ float cs_dot(const f32x16 &p, const f32x16 &q) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += p[r] * q[r];
    return s;
}

// f(t, x) and -- when `want` -- tr = the row's share of the set's divergence, for the wave's 32 rows
template <int HT, int NH>
__device__ __forceinline__ void cs_eval(const cs_args &a, const cnf_set_pos &p, const f32x16 &xin, float t, const cnf_tile<HT> &lat, f32x16 &k, bool want,
                                        float &tr, int lane) {
    constexpr int LD = 32 * HT + 4;
    const int h = lane >> 5, act = a.net.act;
    // (keeps the loop-invariant LDS weight loads inside the step loop: without it the compiler holds whole matrices in registers)
    asm volatile("" ::: "memory");
    float unused;
    cnf_tile<1> xi, mx;
    xi.v[0] = xin;
    cnf_setsum<1, LD>(a.base_x, a.net.set_size, p, xi, mx, 0.f, unused, lane);
    const float *b1 = cnf_smem + a.base_b[0] + 4 * h, *w0 = cnf_smem + a.base_w0 + 4 * h;
    cnf_tile<HT> h1, m1;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        f32x16 acc = {};
        cnf_mma<1>(acc, xi, cnf_smem + a.base_a[0] + m * 1024 + lane * 4);
        cnf_mma<1>(acc, mx, cnf_smem + a.base_g[0] + m * 1024 + lane * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) h1.v[m][r] = (acc[r] + lat.v[m][r]) + (cnf_vec(b1, m, r) + t * cnf_vec(w0, m, r));
    }
    cnf_act_all<HT>(h1, act);
    if (NH == 1) {
        float s = 0.f, e = 0.f, e_set = 0.f;
        if (want) {
            const float *cd = cnf_smem + a.base_tr + 4 * h, *cv = cnf_smem + a.base_tr + HT * 32 + 4 * h;
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d = cnf_dact(h1.v[m][r], act);
                    s += d * cnf_vec(cd, m, r);
                    e += d * cnf_vec(cv, m, r);
                }
            e = e + __shfl_xor(e, 32, 64);
        }
        cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h1, m1, e, e_set, lane);
        f32x16 acc = {};
        cnf_mma<HT>(acc, h1, cnf_smem + a.base_a[1] + lane * 4);
        cnf_mma<HT>(acc, m1, cnf_smem + a.base_g[1] + lane * 4);
        const float *b2 = cnf_smem + a.base_b[1] + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) k[r] = acc[r] + cnf_vec(b2, 0, r);
        if (want) tr = (s + __shfl_xor(s, 32, 64)) + e_set;
    } else {
        cnf_tile<HT> h2, m2;
        cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h1, m1, 0.f, unused, lane);
        const float *b2 = cnf_smem + a.base_b[1] + 4 * h;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            f32x16 acc = {};
            cnf_mma<HT>(acc, h1, cnf_smem + a.base_a[1] + m * HT * 1024 + lane * 4);
            cnf_mma<HT>(acc, m1, cnf_smem + a.base_g[1] + m * HT * 1024 + lane * 4);
#pragma unroll
            for (int r = 0; r < 16; ++r) h2.v[m][r] = acc[r] + cnf_vec(b2, m, r);
        }
        cnf_act_all<HT>(h2, act);
        cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h2, m2, 0.f, unused, lane);
        {
            f32x16 acc = {};
            cnf_mma<HT>(acc, h2, cnf_smem + a.base_a[2] + lane * 4);
            cnf_mma<HT>(acc, m2, cnf_smem + a.base_g[2] + lane * 4);
            const float *b3 = cnf_smem + a.base_b[2] + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) k[r] = acc[r] + cnf_vec(b3, 0, r);
        }
        if (want) {
            // h1 <- d1, m1 <- s1, h2 <- d2, m2 <- s2
            cnf_dact_all<HT>(h1, act);
            cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h1, m1, 0.f, unused, lane);
            cnf_dact_all<HT>(h2, act);
            float s = 0.f, e = 0.f, e_set = 0.f;
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                f32x16 u = {}, v = {};
                cs_mma_c<HT>(u, h1, a, 2, m, lane);          // C_e d1
                e += cs_dot(h2.v[m], u);
                cs_mma_c<HT>(v, h1, a, 0, m, lane);          // C_abd d1 + C_c s1
                cs_mma_c<HT>(v, m1, a, 1, m, lane);
                s += cs_dot(h2.v[m], v);
            }
            e = e + __shfl_xor(e, 32, 64);
            cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h2, m2, e, e_set, lane);
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                f32x16 w = {};
                cs_mma_c<HT>(w, h1, a, 3, m, lane);          // C_f d1 + C_g s1
                cs_mma_c<HT>(w, m1, a, 4, m, lane);
                s += cs_dot(m2.v[m], w);
            }
            tr = (s + __shfl_xor(s, 32, 64)) + e_set;
        }
    }
}

template <int HT, int NH>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_set_flow_kernel(const cs_args a) {
    constexpr int LD = 32 * HT + 4;
    const sx_cnf_set_net &net = a.net;
    const int D = net.dim, L = net.latent_dim, in_dim = 1 + D + L, H1 = net.out_dim[0], N = net.set_size;
    cnf_stage(net.A[0], H1, D, in_dim, 1, HT, 1, a.base_a[0]);
    cnf_stage(net.G[0], H1, D, in_dim, 1, HT, 1, a.base_g[0]);
    cnf_stage_vec(net.bias[0], H1, 1, HT * 32, a.base_b[0]);
    cnf_stage_vec(net.w0, H1, 1, HT * 32, a.base_w0);
    if (NH == 1) {
        cnf_stage(net.A[1], D, H1, H1, 0, 1, HT, a.base_a[1]);
        cnf_stage(net.G[1], D, H1, H1, 0, 1, HT, a.base_g[1]);
        cnf_stage_vec(net.bias[1], D, 1, 32, a.base_b[1]);
        cnf_stage_vec(a.want_ldj ? net.trace : nullptr, H1, 1, HT * 32, a.base_tr);
        cnf_stage_vec(a.want_ldj ? net.trace + H1 : nullptr, H1, 1, HT * 32, a.base_tr + HT * 32);
    } else {
        const int H2 = net.out_dim[1];
        cnf_stage(net.A[1], H2, H1, H1, 0, HT, HT, a.base_a[1]);
        cnf_stage(net.G[1], H2, H1, H1, 0, HT, HT, a.base_g[1]);
        cnf_stage_vec(net.bias[1], H2, 1, HT * 32, a.base_b[1]);
        cnf_stage(net.A[2], D, H2, H2, 0, 1, HT, a.base_a[2]);
        cnf_stage(net.G[2], D, H2, H2, 0, 1, HT, a.base_g[2]);
        cnf_stage_vec(net.bias[2], D, 1, 32, a.base_b[2]);
        if (a.want_ldj)
            for (int ci = 0; ci < a.n_c_lds; ++ci)
                cnf_stage(net.trace + (int64_t)ci * (HT * 32) * (HT * 32), HT * 32, HT * 32, HT * 32, 0, HT, HT, a.base_tr + ci * HT * HT * 1024);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_passes = cnf_set_passes(N, a.n_rows);
    cnf_set_pos p;
    p.rho = cnf_set_slot(lane);
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        cnf_set_pass(p, pass, N, a.n_rows);
        const bool live = p.live;
        const int64_t row = p.row;
        // (the row loads and the store are written out: through cnf_load_row / cnf_store_row all four kernels are allocated differently)
        cnf_tile<1> y;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = sx_kmap(r, h);
            y.v[0][r] = (live && f < D) ? a.x[row * D + f] : 0.f;
        }
        // the latent share of the first layer: A1[:, latent] . latent_row + G1[:, latent] . (the set's latent sum), once per pass
        cnf_tile<HT> lat;
#pragma unroll
        for (int m = 0; m < HT; ++m) lat.v[m] = f32x16{};
        for (int c = 0; c < (L + 31) >> 5; ++c) {
            cnf_tile<1> lb, ml;
            float unused;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * c + sx_kmap(r, h);
                lb.v[0][r] = (live && f < L) ? a.latent[row * L + f] : 0.f;
            }
            cnf_setsum<1, LD>(a.base_x, a.net.set_size, p, lb, ml, 0.f, unused, lane);
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                const int wr = 32 * m + (lane & 31);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int f = 32 * c + sx_kmap(q, h);
                    const bool in = wr < H1 && f < L;
                    const float av = in ? net.A[0][(int64_t)wr * in_dim + 1 + D + f] : 0.f;
                    const float gv = in ? net.G[0][(int64_t)wr * in_dim + 1 + D + f] : 0.f;
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, lb.v[0][q], lat.v[m], 0, 0, 0);
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, ml.v[0][q], lat.v[m], 0, 0, 0);
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
            cnf_tile<1> k1 = {}, k2 = {}, xs = y;
            float q1 = 0.f, q2 = 0.f, ts = ta;
            for (int st = 0; st < n_stages; ++st) {
                cnf_tile<1> k;
                float q = 0.f;
                cs_eval<HT, NH>(a, p, xs.v[0], ts, lat, k.v[0], want, q, lane);
                cnf_tableau<1>(a.solver, st, ta, tb, dt, half, third, two_thirds, k, q, k1, k2, q1, q2, xs, ts, y, l);
            }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = sx_kmap(r, h);
                if (f < D) a.y[row * D + f] = y.v[0][r];
            }
            if (want && h == 0) a.ldj[row] = l;
        }
    }
}

inline int cs_hidden_tiles(const sx_cnf_set_net &net) {
    int HT = 1;
    for (int l = 0; l + 1 < net.n_layers; ++l) HT = cnf_tiles(net.out_dim[l]) > HT ? cnf_tiles(net.out_dim[l]) : HT;
    return HT;
}

// the LDS plan: float offsets into `a` (may be null), -> floats used.  The C matrices go into LDS while they fit beside the rest.
size_t cs_plan(const sx_cnf_set_net &net, int want_ldj, cs_args *a) {
    const int NH = net.n_layers - 1, HT = cs_hidden_tiles(net);
    size_t off = 0;
    int ba[3] = {0, 0, 0}, bg[3] = {0, 0, 0}, bb[3] = {0, 0, 0};
    for (int l = 0; l <= NH; ++l) {
        const int KT = l == 0 ? 1 : HT, MT = l == NH ? 1 : HT;
        ba[l] = (int)off; off += (size_t)MT * KT * 1024;
        bg[l] = (int)off; off += (size_t)MT * KT * 1024;
        bb[l] = (int)off; off += (size_t)MT * 32;
    }
    const int base_w0 = (int)off; off += (size_t)HT * 32;
    const int base_x = (int)off; off += (size_t)SX_CNF_ROWS * (32 * HT + 4);
    const int base_tr = (int)off;
    int n_c_lds = 0;
    if (NH == 1) off += (size_t)2 * HT * 32;
    else if (want_ldj) {
        const size_t c_floats = (size_t)HT * HT * 1024;
        while (n_c_lds < 5 && (off + c_floats) * 4 <= SX_CNF_LDS_BYTES) { off += c_floats; ++n_c_lds; }
    }
    if (a) {
        for (int l = 0; l < 3; ++l) { a->base_a[l] = ba[l]; a->base_g[l] = bg[l]; a->base_b[l] = bb[l]; }
        a->base_w0 = base_w0; a->base_x = base_x; a->base_tr = base_tr; a->n_c_lds = n_c_lds;
    }
    return off;
}

// the shape of the network alone (no pointer is read)
int cs_check_shape(const sx_cnf_set_net *net_host) {
    SX_REQUIRE(net_host != nullptr, "sx_cnf_set_flow: null network");
    const sx_cnf_set_net &net = *net_host;
    SX_REQUIRE(net.n_layers == 2 || net.n_layers == 3, "sx_cnf_set_flow: one or two hidden layers (got %d equivariant layers)", net.n_layers);
    SX_REQUIRE(net.dim >= 1 && net.dim <= SX_CNF_SET_MAX_DIM, "sx_cnf_set_flow: dim must be in 1..%d (got %d)", SX_CNF_SET_MAX_DIM, net.dim);
    SX_REQUIRE(net.latent_dim >= 0 && 1 + net.dim + net.latent_dim <= SX_CNF_SET_MAX_IN,
               "sx_cnf_set_flow: 1 + dim + latent_dim must be <= %d", SX_CNF_SET_MAX_IN);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "sx_cnf_set_flow: activation %d has no in-kernel derivative", net.act);
    SX_REQUIRE(net.set_size >= 1 && net.set_size <= SX_CNF_SET_MAX_SIZE, "sx_cnf_set_flow: set_size must be in 1..%d (got %d)",
               SX_CNF_SET_MAX_SIZE, net.set_size);
    for (int l = 0; l + 1 < net.n_layers; ++l)
        SX_REQUIRE(net.out_dim[l] >= 1 && net.out_dim[l] <= SX_CNF_SET_MAX_HIDDEN, "sx_cnf_set_flow: hidden layer %d must have 1..%d units (got %d)",
                   l, SX_CNF_SET_MAX_HIDDEN, net.out_dim[l]);
    SX_REQUIRE(net.out_dim[net.n_layers - 1] == net.dim, "sx_cnf_set_flow: the last layer must map back to dim");
    return SX_OK;
}

}  // namespace

extern "C" size_t sx_cnf_set_lds_bytes(const sx_cnf_set_net *net_host, int32_t want_ldj) {
    if (cs_check_shape(net_host) != SX_OK) return 0;
    return cs_plan(*net_host, want_ldj ? 1 : 0, nullptr) * 4;
}

extern "C" int sx_cnf_set_flow(const sx_cnf_set_net *net_host, const float *x, const float *latent, float *y, float *ldj, int64_t n_rows,
                               int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj, void *stream) {
    const int rc = cs_check_shape(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_set_net &net = *net_host;
    for (int l = 0; l < net.n_layers; ++l)
        SX_REQUIRE(net.A[l] != nullptr && net.G[l] != nullptr && net.bias[l] != nullptr, "sx_cnf_set_flow: layer %d lacks A, G or bias", l);
    SX_REQUIRE(net.w0 != nullptr, "sx_cnf_set_flow: the time column w0 is missing");
    const int rc_call = cnf_check_call("sx_cnf_set_flow", solver, n_rows, net.set_size, n_steps, step_size, x, y);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "sx_cnf_set_flow: latent rows missing");
    SX_REQUIRE(!want_ldj || (ldj != nullptr && net.trace != nullptr), "sx_cnf_set_flow: want_ldj needs ldj and the trace constants");
    SX_REQUIRE(!want_ldj || net.n_layers == 2 || ((uintptr_t)net.trace & 15) == 0, "sx_cnf_set_flow: the C matrices must be 16-byte aligned");
    cs_args a{};
    a.net = net;
    const size_t lds = cs_plan(net, want_ldj ? 1 : 0, &a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_set_flow: the padded weights need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.want_ldj = want_ldj ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    const int NH = net.n_layers - 1, HT = cs_hidden_tiles(net);
    const int64_t want = cnf_set_blocks(n_rows, net.set_size);
    const char *fn = "sx_cnf_set_flow";
    if (HT == 1) return NH == 1 ? cnf_launch<cnf_set_flow_kernel<1, 1>>(fn, a, lds, want, stream) : cnf_launch<cnf_set_flow_kernel<1, 2>>(fn, a, lds, want, stream);
    return NH == 1 ? cnf_launch<cnf_set_flow_kernel<2, 1>>(fn, a, lds, want, stream) : cnf_launch<cnf_set_flow_kernel<2, 2>>(fn, a, lds, want, stream);
}
