// Exact-trace continuous normalizing flow over SETS (ContinuousTransform with divergence='exact' over net.DiffeqExactTraceDeepSet;
// reference: stribor/net/diffeq_exact_trace.py:75-101, diffeq_zero_trace.py:59-176, made.py, diagjac.py) on a fixed grid, in one launch.
//
// sx_cnf_exact_set_flow -- rows are set elements, the N = set_size elements of a set contiguous.  For element i and dimension d
//     e_j      = set_emb([t, x_j])                    an MLP, d_h columns
//     p_i      = pool over j != i of e_j              sum | mean | max, the same for every d
//     h_i[d,:] = MADE(x_i)[d,:] + p_i                 d_h values per dimension; neither term depends on x_i[d]
//     f_i[d]   = g(t, x_i[d], h_i[d,:], latent_i)     the dimwise net g: one MLP shared by every dimension
//     jac_i[d] = dg/dx at fixed h                     = df_i[d]/dx_i[d] exactly
// One half is sx_cnf_exact.hip's, and is the same code: the MADE, the dimwise loop with its forward-mode tangent, the solve of a row
// group, the plan pieces of the image (A-fragment order, feature POSITIONS) and the host checks come from sx_cnf_exact_common.h.  The
// other half follows sx_cnf_set.hip (the set layout and its ordered exchange through LDS) and is this file's own; the conventions hold:
// one wave = 32 rows on the MFMA column, exact fp32 (v_mfma_f32_32x32x2_f32), -ffp-contract=off, the same solvers, grid and tableau,
// state / stage vectors / h / log-det in registers for the whole grid, time as b1 + t * W1[:, 0].
//   * a workgroup of 4 waves owns 128 row slots and takes floor(128 / N) WHOLE sets per pass: sets never straddle workgroups, they
//     may straddle waves.  Slots past the last set are padding: they compute on zeros and are never stored.  The pass loop, the stage
//     loop and `want` are uniform over the workgroup, so every wave reaches every barrier;
//   * the embedding's last layer puts slot kk at position kmap(kk >> 1, kk & 1): register c of lane half hh holds slot 2c + hh of the
//     row -- the slot pair the MADE output keeps in tile c (register d, the two lane halves), so p is added to a tile's registers
//     without a shuffle;
//   * one exchange per evaluation (xs_pool; barriers as cnf_setsum's): every lane writes its slots to a scratch [128][16], one thread
//     per (set, slot) walks the set's rows IN ELEMENT ORDER -- sum / mean: adds them into the set's first row; max: keeps the two
//     largest values, duplicates counted -- and every lane reads its set's first row back: sum - own (mean: / max(N - 1, 1), a true
//     division), or own == first ? second : first.  The order depends on the position inside the set only, so a set's result does not
//     depend on its slot or on its neighbours.  N = 1 needs no exchange (p = 0);
//   * the latent columns' share of the dimwise first layer: one GEMM per pass before the grid loop, A fragments from global memory.
//
// Coverage: 1 <= N <= 128, dim <= 16, d_h <= 8, latent_dim <= 64, one or two hidden layers of <= 64 units (the same widths in the three
// nets), activations Identity .. LeakyReLU.  The largest image (two hidden layers of 64, d_h = 8) is 115 KiB, the exchange 8 KiB.
#include "sx_cnf_exact_common.h"

#define SX_XS_LD 16          /* floats per row of the exchange scratch: slots 0..7, and for max pooling the second values at 8..15 */

namespace {

// the LDS image: float offsets (sx_cnf_exact_set_net.image is laid out in this order; net/diffeq_exact_trace.py builds it); the
// exchange scratch follows it
struct xs_plan {
    cnf_exact_made made;
    int sw[3], sb[3], st0;        // the set embedding: the same (one output tile), and the time column of its first layer
    cnf_exact_dimwise dw;
    int total;                    // floats of the image = the offset of the exchange scratch [SX_CNF_ROWS][SX_XS_LD]
};

__host__ __device__ constexpr xs_plan xs_make_plan(int HT, int NH, int OT) {
    xs_plan p{};
    int off = 0;
    p.made = cnf_exact_plan_made(off, HT, NH, OT);
    p.sw[0] = off; off += HT * 1024;
    p.sb[0] = off; off += HT * 32;
    p.st0 = off; off += HT * 32;
    if (NH == 2) {
        p.sw[1] = off; off += HT * HT * 1024;
        p.sb[1] = off; off += HT * 32;
    }
    p.sw[2] = off; off += HT * 1024;
    p.sb[2] = off; off += 32;
    p.dw = cnf_exact_plan_dimwise(off, HT, NH);
    p.total = off;
    return p;
}

struct xs_args : cnf_exact_args<sx_cnf_exact_set_net> {};

// out[c] = the pooling over the OTHER rows of the lane's set of slot 2c + (lane >> 5), from the lane's own e[c].  `xs`: the exchange
// scratch.  Uniform over the workgroup: every thread must call it.
template <int OT>
__device__ __forceinline__ void xs_pool(const xs_args &a, const cnf_set_pos &p, float *xs, const float (&e)[OT], float (&out)[OT], int lane) {
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
__device__ __forceinline__ void xs_eval(const xs_args &a, const cnf_set_pos &pos, const f32x16 &xin, float t, const cnf_tile<HT> &lat, f32x16 &k, bool want, float &tr,
                                        int lane) {
    constexpr xs_plan p = xs_make_plan(HT, NH, OT);
    const int act = a.net.act;
    // the image never changes: without this the compiler hoists its loads out of the step loop and holds matrices in registers
    asm volatile("" ::: "memory");
    // ---- the exclusive net: the MADE of the row, plus the pooled embeddings of the set's other rows in every dimension ----
    cnf_tile<OT> raw;
#pragma unroll
    for (int m = 0; m < OT; ++m) raw.v[m] = f32x16{};
    cnf_tile<1> xi;
    xi.v[0] = xin;
    cnf_exact_made_eval<HT, NH, OT>(p.made, xi, raw, act, lane);
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
    cnf_exact_dimwise_eval<HT, NH, OT>(p.dw, act, a.net.dim, xin, raw, t, lat, k, want, tr, lane);
}

template <int HT, int NH, int OT>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_exact_set_kernel(const xs_args a) {
    constexpr xs_plan pl = xs_make_plan(HT, NH, OT);
    cnf_stage_image(a.net.image, pl.total);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, D = a.net.dim, L = a.net.latent_dim, N = a.net.set_size;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_passes = cnf_set_passes(N, a.n_rows);
    cnf_set_pos p;
    p.rho = cnf_set_slot(lane);
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        cnf_set_pass(p, pass, N, a.n_rows);
        const bool live = p.live;
        const int64_t row = p.row;
        CNF_EXACT_SOLVE_ROWS(HT, a, row, live, h, D, L, want, sgn, lane, xs_eval<HT, NH, OT>(a, p, xs.v[0], ts, lat, k.v[0], want, q, lane))
    }
}

int xs_check_net(const sx_cnf_exact_set_net *net_host) {
    const char *fn = "sx_cnf_exact_set_flow";
    const int rc = cnf_exact_check_net(fn, net_host, SX_CNF_EXACT_SET_MAX_DIM, SX_CNF_EXACT_SET_MAX_DH, SX_CNF_EXACT_SET_MAX_LATENT,
                                       SX_CNF_EXACT_SET_MAX_HIDDEN);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_set_net &net = *net_host;
    SX_REQUIRE(net.set_size >= 1 && net.set_size <= SX_CNF_EXACT_SET_MAX_SIZE, "%s: set_size must be in 1..%d (got %d)", fn,
               SX_CNF_EXACT_SET_MAX_SIZE, net.set_size);
    SX_REQUIRE(net.pooling >= SX_POOL_SUM && net.pooling <= SX_POOL_MAX, "%s: pooling must be sum (0), mean (1) or max (2), got %d", fn, net.pooling);
    return SX_OK;
}

// floats of the image, by the kernel's plan; the exchange scratch follows them
inline size_t xs_image_floats(const sx_cnf_exact_set_net &net) {
    int HT, OT;
    cnf_exact_shape(net, &HT, &OT);
    return (size_t)xs_make_plan(HT, net.n_hidden, OT).total;
}

}  // namespace

extern "C" size_t sx_cnf_exact_set_lds_bytes(const sx_cnf_exact_set_net *net_host) {
    if (xs_check_net(net_host) != SX_OK) return 0;
    const size_t lds = (xs_image_floats(*net_host) + SX_CNF_ROWS * SX_XS_LD) * 4;
    return lds <= SX_CNF_LDS_BYTES ? lds : 0;
}

extern "C" int sx_cnf_exact_set_flow(const sx_cnf_exact_set_net *net_host, const float *x, const float *latent, float *y, float *ldj,
                                     int64_t n_rows, int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj,
                                     void *stream) {
    const char *fn = "sx_cnf_exact_set_flow";
    int rc = xs_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_set_net &net = *net_host;
    rc = cnf_check_call(fn, solver, n_rows, net.set_size, n_steps, step_size, x, y);
    if (rc != SX_OK) return rc;
    int HT, OT;
    cnf_exact_shape(net, &HT, &OT);
    const int NH = net.n_hidden;
    const size_t image = xs_image_floats(net), lds = (image + SX_CNF_ROWS * SX_XS_LD) * 4;
    rc = cnf_exact_check_flow(fn, net, latent, ldj, want_ldj, image, lds, "the image and the exchange need");
    if (rc != SX_OK || n_rows == 0) return rc;
    const xs_args a = cnf_exact_fill<xs_args>(net, x, latent, y, ldj, n_rows, solver, n_steps, t0, t1, step_size, want_ldj);
    CNF_EXACT_DISPATCH(cnf_exact_set_kernel, fn, HT, NH, OT, a, lds, cnf_set_blocks(n_rows, net.set_size), stream);
}
