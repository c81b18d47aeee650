// Exact-trace continuous normalizing flow over SETS (ContinuousTransform with divergence='exact' over net.DiffeqExactTraceDeepSet;
// reference: stribor/net/diffeq_exact_trace.py:75-101, diffeq_zero_trace.py:59-176, made.py, diagjac.py) on a fixed grid, in one launch.
//
// sx_cnf_exact_set_flow -- rows are set elements, the N = set_size elements of a set contiguous.  For element i and dimension d
//     e_j      = set_emb([t, x_j])                    an MLP, d_h columns
//     p_i      = pool over j != i of e_j              sum | mean | max, the same for every d
//     h_i[d,:] = MADE(x_i)[d,:] + p_i                 d_h values per dimension; neither term depends on x_i[d]
//     f_i[d]   = g(t, x_i[d], h_i[d,:], latent_i)     the dimwise net g: one MLP shared by every dimension
//     jac_i[d] = dg/dx at fixed h                     = df_i[d]/dx_i[d] exactly
// The two halves are those of sx_cnf_exact.hip (the MADE, the dimwise loop with its forward-mode tangent, the image in A-fragment
// order and in feature POSITIONS) and of sx_cnf_set.hip (the set layout and its ordered exchange through LDS); their conventions hold:
// one wave = 32 rows on the MFMA column, exact fp32 (v_mfma_f32_32x32x2_f32), -ffp-contract=off, the same solvers, grid and tableau,
// state / stage vectors / h / log-det in registers for the whole grid, time as b1 + t * W1[:, 0].
//   * a workgroup of 4 waves owns 128 row slots and takes floor(128 / N) WHOLE sets per pass: sets never straddle workgroups, they
//     may straddle waves.  Slots past the last set are padding: they compute on zeros and are never stored.  The pass loop, the stage
//     loop and `want` are uniform over the workgroup, so every wave reaches every barrier;
//   * the embedding's last layer puts slot kk at position kmap(kk >> 1, kk & 1): register c of lane half hh holds slot 2c + hh of the
//     row -- the slot pair the MADE output keeps in tile c (register d, the two lane halves), so p is added to a tile's registers
//     without a shuffle;
//   * one exchange per evaluation (xs_pool; barriers as cs_setsum's): every lane writes its slots to a scratch [128][16], one thread
//     per (set, slot) walks the set's rows IN ELEMENT ORDER -- sum / mean: adds them into the set's first row; max: keeps the two
//     largest values, duplicates counted -- and every lane reads its set's first row back: sum - own (mean: / max(N - 1, 1), a true
//     division), or own == first ? second : first.  The order depends on the position inside the set only, so a set's result does not
//     depend on its slot or on its neighbours.  N = 1 needs no exchange (p = 0);
//   * the latent columns' share of the dimwise first layer: one GEMM per pass before the grid loop, A fragments from global memory.
//
// Coverage: 1 <= N <= 128, dim <= 16, d_h <= 8, latent_dim <= 64, one or two hidden layers of <= 64 units (the same widths in the three
// nets), activations Identity .. LeakyReLU.  The largest image (two hidden layers of 64, d_h = 8) is 115 KiB, the exchange 8 KiB.
#include "sx_cnf_common.h"

#define SX_XS_LD 16          /* floats per row of the exchange scratch: slots 0..7, and for max pooling the second values at 8..15 */

namespace {

// the LDS image: float offsets (sx_cnf_exact_set_net.image is laid out in this order; net/diffeq_exact_trace.py builds it); the
// exchange scratch follows it
struct xs_plan {
    int mw[3], mb[3];             // the MADE: first layer, (second hidden layer,) last layer -- images and biases
    int sw[3], sb[3], st0;        // the set embedding: the same, and the time column of its first layer
    int dw1, db1, dw0, dwx;       // dimwise first layer: image, bias, the time column, the x column (the tangent's seed)
    int dw2, db2;                 // two hidden layers: the second
    int dwl, dbl;                 // the last layer as a vector over the hidden positions; its bias (1 float, padded to 32)
    int total;                    // floats of the image = the offset of the exchange scratch [SX_CNF_ROWS][SX_XS_LD]
};

__host__ __device__ constexpr xs_plan xs_make_plan(int HT, int NH, int OT) {
    xs_plan p{};
    int off = 0;
    p.mw[0] = off; off += HT * 1024;
    p.mb[0] = off; off += HT * 32;
    if (NH == 2) {
        p.mw[1] = off; off += HT * HT * 1024;
        p.mb[1] = off; off += HT * 32;
    }
    p.mw[2] = off; off += OT * HT * 1024;
    p.mb[2] = off; off += OT * 32;
    p.sw[0] = off; off += HT * 1024;
    p.sb[0] = off; off += HT * 32;
    p.st0 = off; off += HT * 32;
    if (NH == 2) {
        p.sw[1] = off; off += HT * HT * 1024;
        p.sb[1] = off; off += HT * 32;
    }
    p.sw[2] = off; off += HT * 1024;
    p.sb[2] = off; off += 32;
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

struct xs_args {
    sx_cnf_exact_set_net net;
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int64_t n_rows;
    int solver, n_steps, want_ldj;
    float t0, t1, step_size;
};

// where a lane stands in its workgroup's pass
struct xs_pos {
    int rho;            // row slot 0 .. SX_CNF_ROWS - 1
    int first;          // the first slot of the row's set (a padding slot: itself)
    int n_sets;         // whole sets of this pass
    bool live;          // the slot holds a row
};

// out[c] = the pooling over the OTHER rows of the lane's set of slot 2c + (lane >> 5), from the lane's own e[c].  `xs`: the exchange
// scratch.  Uniform over the workgroup: every thread must call it.
template <int OT>
__device__ __forceinline__ void xs_pool(const xs_args &a, const xs_pos &p, float *xs, const float (&e)[OT], float (&out)[OT], int lane) {
    const int N = a.net.set_size, pooling = a.net.pooling, h = lane >> 5;
    if (N == 1) {
#pragma unroll
        for (int c = 0; c < OT; ++c) out[c] = 0.f;
        return;
    }
    __syncthreads();                    // the reads of the previous exchange are over
#pragma unroll
    for (int c = 0; c < OT; ++c) xs[p.rho * SX_XS_LD + 2 * c + h] = e[c];
    __syncthreads();
    const int n_pairs = p.n_sets * (2 * OT);
    for (int q = threadIdx.x; q < n_pairs; q += SX_CNF_THREADS) {
        const int s = q / (2 * OT), f = q - s * (2 * OT);
        float *col = xs + (s * N) * SX_XS_LD + f;
        if (pooling == SX_POOL_MAX) {
            float first = col[0], second = -INFINITY;
            for (int j = 1; j < N; ++j) {
                const float v = col[j * SX_XS_LD];
                if (v > first) { second = first; first = v; }
                else if (v > second) second = v;
            }
            col[0] = first;
            col[8] = second;
        } else {
            float acc = col[0];
            for (int j = 1; j < N; ++j) acc = acc + col[j * SX_XS_LD];
            col[0] = acc;
        }
    }
    __syncthreads();
    const float *src = xs + p.first * SX_XS_LD + h;
    const float div = (float)(N - 1);
#pragma unroll
    for (int c = 0; c < OT; ++c) {
        float v;
        if (pooling == SX_POOL_MAX) {
            const float first = src[2 * c], second = src[2 * c + 8];
            v = e[c] == first ? second : first;
        } else {
            v = src[2 * c] - e[c];
            if (pooling == SX_POOL_MEAN) v = v / div;
        }
        out[c] = p.live ? v : 0.f;
    }
}

// the MADE of the exclusive net: raw += W_last . hidden(x) + b_last
template <int HT, int NH, int OT>
__device__ __forceinline__ void xs_made(const cnf_tile<1> &xi, cnf_tile<OT> &raw, int act, int lane) {
    constexpr xs_plan p = xs_make_plan(HT, NH, OT);
    const int h = lane >> 5;
    cnf_tile<HT> h1;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        h1.v[m] = f32x16{};
        cnf_mma<1>(h1.v[m], xi, cnf_smem + p.mw[0] + m * 1024 + lane * 4);
    }
    cnf_add_vec<HT>(h1, cnf_smem + p.mb[0] + 4 * h);
    cnf_act_all<HT>(h1, act);
    if (NH == 2) {
        cnf_tile<HT> h2;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            h2.v[m] = f32x16{};
            cnf_mma<HT>(h2.v[m], h1, cnf_smem + p.mw[1] + m * HT * 1024 + lane * 4);
        }
        cnf_add_vec<HT>(h2, cnf_smem + p.mb[1] + 4 * h);
        cnf_act_all<HT>(h2, act);
        h1 = h2;
    }
#pragma unroll
    for (int m = 0; m < OT; ++m) cnf_mma<HT>(raw.v[m], h1, cnf_smem + p.mw[2] + m * HT * 1024 + lane * 4);
    cnf_add_vec<OT>(raw, cnf_smem + p.mb[2] + 4 * h);
    asm volatile("" ::: "memory");
}

// the set embedding of the wave's rows: e[c] = slot 2c + (lane >> 5) of set_emb([t, x])
template <int HT, int NH, int OT>
__device__ __forceinline__ void xs_embed(const cnf_tile<1> &xi, float t, float (&e)[OT], int act, int lane) {
    constexpr xs_plan p = xs_make_plan(HT, NH, OT);
    const int h = lane >> 5;
    const float *b1 = cnf_smem + p.sb[0] + 4 * h, *w0 = cnf_smem + p.st0 + 4 * h;
    cnf_tile<HT> h1;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        f32x16 acc = {};
        cnf_mma<1>(acc, xi, cnf_smem + p.sw[0] + m * 1024 + lane * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] + (cnf_vec(b1, m, r) + t * cnf_vec(w0, m, r));
        h1.v[m] = acc;
    }
    cnf_act_all<HT>(h1, act);
    if (NH == 2) {
        cnf_tile<HT> h2;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            h2.v[m] = f32x16{};
            cnf_mma<HT>(h2.v[m], h1, cnf_smem + p.sw[1] + m * HT * 1024 + lane * 4);
        }
        cnf_add_vec<HT>(h2, cnf_smem + p.sb[1] + 4 * h);
        cnf_act_all<HT>(h2, act);
        h1 = h2;
    }
    f32x16 out = {};
    cnf_mma<HT>(out, h1, cnf_smem + p.sw[2] + lane * 4);
    const float *b3 = cnf_smem + p.sb[2] + 4 * h;
#pragma unroll
    for (int c = 0; c < OT; ++c) e[c] = out[c] + cnf_vec(b3, 0, c);
    asm volatile("" ::: "memory");
}

// f(t, x) -> k (dimension i at register i of the lower lane half) and -- when `want` -- tr = sum_i jac_i, for the wave's 32 rows
template <int HT, int NH, int OT>
__device__ __forceinline__ void xs_eval(const xs_args &a, const xs_pos &pos, const f32x16 &xin, float t, const cnf_tile<HT> &lat, f32x16 &k, bool want, float &tr,
                                        int lane) {
    constexpr xs_plan p = xs_make_plan(HT, NH, OT);
    const int h = lane >> 5, act = a.net.act, D = a.net.dim;
    // the image never changes: without this the compiler hoists its loads out of the step loop and holds matrices in registers
    asm volatile("" ::: "memory");
    // ---- the exclusive net: the MADE of the row, plus the pooled embeddings of the set's other rows in every dimension ----
    cnf_tile<OT> raw;
#pragma unroll
    for (int m = 0; m < OT; ++m) raw.v[m] = f32x16{};
    cnf_tile<1> xi;
    xi.v[0] = xin;
    xs_made<HT, NH, OT>(xi, raw, act, lane);
    {
        float e[OT], pool[OT];
        xs_embed<HT, NH, OT>(xi, t, e, act, lane);
        xs_pool<OT>(a, pos, cnf_smem + p.total, e, pool, lane);
#pragma unroll
        for (int m = 0; m < OT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) raw.v[m][r] = raw.v[m][r] + pool[m];
    }
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
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_exact_set_kernel(const xs_args a) {
    const sx_cnf_exact_set_net &net = a.net;
    constexpr xs_plan pl = xs_make_plan(HT, NH, OT);
    cnf_stage_image(net.image, pl.total);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, D = net.dim, L = net.latent_dim, N = net.set_size;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int rows_per_pass = cnf_rows_per_pass(N);
    const int64_t n_passes = (a.n_rows + rows_per_pass - 1) / rows_per_pass;
    xs_pos p;
    p.rho = (threadIdx.x >> 6) * 32 + (lane & 31);
    // (every bound of this loop is uniform over the workgroup: all four waves make every pass and meet at every barrier)
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        const int64_t base = pass * rows_per_pass, left = a.n_rows - base;
        const int n_here = left < rows_per_pass ? (int)left : rows_per_pass;
        const bool live = p.rho < n_here;
        const int64_t row = base + p.rho;
        p.live = live;
        p.first = live ? (p.rho / N) * N : p.rho;
        p.n_sets = n_here / N;
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
                xs_eval<HT, NH, OT>(a, p, xs.v[0], ts, lat, k.v[0], want, q, lane);
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

int xs_check_net(const sx_cnf_exact_set_net *net_host) {
    SX_REQUIRE(net_host != nullptr, "sx_cnf_exact_set_flow: null network");
    const sx_cnf_exact_set_net &net = *net_host;
    SX_REQUIRE(net.n_hidden == 1 || net.n_hidden == 2, "sx_cnf_exact_set_flow: one or two hidden layers (got %d)", net.n_hidden);
    SX_REQUIRE(net.dim >= 1 && net.dim <= SX_CNF_EXACT_SET_MAX_DIM, "sx_cnf_exact_set_flow: dim must be in 1..%d (got %d)",
               SX_CNF_EXACT_SET_MAX_DIM, net.dim);
    SX_REQUIRE(net.d_h >= 1 && net.d_h <= SX_CNF_EXACT_SET_MAX_DH, "sx_cnf_exact_set_flow: d_h must be in 1..%d (got %d)",
               SX_CNF_EXACT_SET_MAX_DH, net.d_h);
    SX_REQUIRE(net.latent_dim >= 0 && net.latent_dim <= SX_CNF_EXACT_SET_MAX_LATENT, "sx_cnf_exact_set_flow: latent_dim must be in 0..%d (got %d)",
               SX_CNF_EXACT_SET_MAX_LATENT, net.latent_dim);
    SX_REQUIRE(net.set_size >= 1 && net.set_size <= SX_CNF_EXACT_SET_MAX_SIZE, "sx_cnf_exact_set_flow: set_size must be in 1..%d (got %d)",
               SX_CNF_EXACT_SET_MAX_SIZE, net.set_size);
    SX_REQUIRE(net.pooling >= SX_POOL_SUM && net.pooling <= SX_POOL_MAX, "sx_cnf_exact_set_flow: pooling must be sum (0), mean (1) or max (2), got %d",
               net.pooling);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "sx_cnf_exact_set_flow: activation %d has no in-kernel derivative", net.act);
    for (int l = 0; l < net.n_hidden; ++l)
        SX_REQUIRE(net.hidden[l] >= 1 && net.hidden[l] <= SX_CNF_EXACT_SET_MAX_HIDDEN,
                   "sx_cnf_exact_set_flow: hidden layer %d must have 1..%d units (got %d)", l, SX_CNF_EXACT_SET_MAX_HIDDEN, net.hidden[l]);
    return SX_OK;
}

inline void xs_shape(const sx_cnf_exact_set_net &net, int *HT, int *OT) {
    int ht = cnf_tiles(net.hidden[0]);
    if (net.n_hidden == 2 && cnf_tiles(net.hidden[1]) > ht) ht = cnf_tiles(net.hidden[1]);
    *HT = ht;
    *OT = cnf_out_tiles(net.d_h);
}

inline size_t xs_lds_floats(const sx_cnf_exact_set_net &net) {
    int HT, OT;
    xs_shape(net, &HT, &OT);
    return (size_t)xs_make_plan(HT, net.n_hidden, OT).total + SX_CNF_ROWS * SX_XS_LD;
}

}  // namespace

extern "C" size_t sx_cnf_exact_set_lds_bytes(const sx_cnf_exact_set_net *net_host) {
    if (xs_check_net(net_host) != SX_OK) return 0;
    const size_t lds = xs_lds_floats(*net_host) * 4;
    return lds <= SX_CNF_LDS_BYTES ? lds : 0;
}

extern "C" int sx_cnf_exact_set_flow(const sx_cnf_exact_set_net *net_host, const float *x, const float *latent, float *y, float *ldj,
                                     int64_t n_rows, int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj,
                                     void *stream) {
    const int rc = xs_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_set_net &net = *net_host;
    const int rc_call = cnf_check_call("sx_cnf_exact_set_flow", solver, n_rows, net.set_size, n_steps, step_size, x, y);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || (latent != nullptr && net.w_latent != nullptr), "sx_cnf_exact_set_flow: latent rows / latent weights missing");
    SX_REQUIRE(!want_ldj || ldj != nullptr, "sx_cnf_exact_set_flow: want_ldj needs ldj");
    int HT, OT;
    xs_shape(net, &HT, &OT);
    const int NH = net.n_hidden;
    const size_t image = (size_t)xs_make_plan(HT, NH, OT).total, lds = xs_lds_floats(net) * 4;
    SX_REQUIRE(net.image != nullptr && (size_t)net.image_floats == image, "sx_cnf_exact_set_flow: the image holds %d floats, the kernel's plan %zu",
               net.image_floats, image);
    SX_REQUIRE(((uintptr_t)net.image & 15) == 0 && ((uintptr_t)net.w_latent & 15) == 0, "sx_cnf_exact_set_flow: image / w_latent must be 16-byte aligned");
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_exact_set_flow: the image and the exchange need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    xs_args a{};
    a.net = net;
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.want_ldj = want_ldj ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    const int64_t want = cnf_set_blocks(n_rows, net.set_size);
#define XS_CASE(H_, O_)                                                                                \
    if (HT == H_ && OT == O_)                                                                            \
        return NH == 1 ? cnf_launch<cnf_exact_set_kernel<H_, 1, O_>>("sx_cnf_exact_set_flow", a, lds, want, stream) \
                       : cnf_launch<cnf_exact_set_kernel<H_, 2, O_>>("sx_cnf_exact_set_flow", a, lds, want, stream);
    XS_CASE(1, 1) XS_CASE(1, 2) XS_CASE(1, 4) XS_CASE(2, 1) XS_CASE(2, 2) XS_CASE(2, 4)
#undef XS_CASE
    sx_set_error("sx_cnf_exact_set_flow: no kernel for %d hidden x %d output tiles", HT, OT);
    return SX_E_BADARG;
}
