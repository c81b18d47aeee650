// What the two exact-trace CNF kernel files (sx_cnf_exact.hip: rows; sx_cnf_exact_set.hip: sets) have in common beyond
// sx_cnf_common.h -- everything that depends only on the fields the two network structs share and on the LDS layout of a MADE and of
// the dimwise net, written once, so that the dimwise arithmetic (the seeded MFMA chain, the forward-mode tangent, the half-wave fold)
// is one piece of code:
//   * the LDS plan in pieces, each laid out from a running float offset: a MADE block, the dimwise block (a file's plan is a sequence
//     of them: MADE, MADE, dimwise / MADE, set embedding, dimwise);
//   * device: the MADE evaluator, the dimwise evaluator, and the solve of one row group (a macro that both kernels expand: see there);
//   * host: the range checks of the shared network fields (the entry point's name and the limits are arguments), the tile counts, the
//     image / alignment / LDS-budget checks of a flow call, the argument struct with its fill, and the dispatch over (HT, NH, OT).
// The evaluators are __forceinline__ and take their plan piece by value from the caller's constexpr plan: after inlining the offsets
// are the immediates they were when each file had its own copy, and every kernel compiles to the instructions it compiled to then.
// Internal linkage: two translation units include it.
#pragma once
#include "sx_cnf_common.h"

namespace {

// ---- the LDS plan, in pieces (float offsets) -------------------------------------------------------------------------------------------
struct cnf_exact_made {
    int w[3], b[3];               // first layer, (second hidden layer,) last layer -- images and biases
};

struct cnf_exact_dimwise {
    int dw1, db1, dw0, dwx;       // first layer: image, bias, the time column, the x column (the tangent's seed)
    int dw2, db2;                 // two hidden layers: the second
    int dwl, dbl;                 // the last layer as a vector over the hidden positions; its bias (1 float, padded to 32)
};

// a MADE whose last layer has OT row tiles, from `off` on; -> `off` behind it
__host__ __device__ constexpr cnf_exact_made cnf_exact_plan_made(int &off, int HT, int NH, int OT) {
    cnf_exact_made p{};
    p.w[0] = off; off += HT * 1024;
    p.b[0] = off; off += HT * 32;
    if (NH == 2) {
        p.w[1] = off; off += HT * HT * 1024;
        p.b[1] = off; off += HT * 32;
    }
    p.w[2] = off; off += OT * HT * 1024;
    p.b[2] = off; off += OT * 32;
    return p;
}

__host__ __device__ constexpr cnf_exact_dimwise cnf_exact_plan_dimwise(int &off, int HT, int NH) {
    cnf_exact_dimwise p{};
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
    return p;
}

// a flow call's arguments (NET: sx_cnf_exact_net or sx_cnf_exact_set_net); each file derives its own struct from it, so that its
// kernels keep their names
template <class NET>
struct cnf_exact_args {
    NET net;
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int64_t n_rows;
    int solver, n_steps, want_ldj;
    float t0, t1, step_size;
};

// ---- device ----------------------------------------------------------------------------------------------------------------------------
// a MADE of the exclusive net: raw += W_last . hidden(x) + b_last
template <int HT, int NH, int OT>
__device__ __forceinline__ void cnf_exact_made_eval(const cnf_exact_made p, const cnf_tile<1> &xi, cnf_tile<OT> &raw, int act, int lane) {
    const int h = lane >> 5;
    cnf_tile<HT> h1;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        h1.v[m] = f32x16{};
        cnf_mma<1>(h1.v[m], xi, cnf_smem + p.w[0] + m * 1024 + lane * 4);
    }
    cnf_add_vec<HT>(h1, cnf_smem + p.b[0] + 4 * h);
    cnf_act_all<HT>(h1, act);
    if (NH == 2) {
        cnf_tile<HT> h2;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            h2.v[m] = f32x16{};
            cnf_mma<HT>(h2.v[m], h1, cnf_smem + p.w[1] + m * HT * 1024 + lane * 4);
        }
        cnf_add_vec<HT>(h2, cnf_smem + p.b[1] + 4 * h);
        cnf_act_all<HT>(h2, act);
        h1 = h2;
    }
#pragma unroll
    for (int m = 0; m < OT; ++m) cnf_mma<HT>(raw.v[m], h1, cnf_smem + p.w[2] + m * HT * 1024 + lane * 4);
    cnf_add_vec<OT>(raw, cnf_smem + p.b[2] + 4 * h);
    asm volatile("" ::: "memory");
}

// the dimwise net, one dimension at a time, on [x_i, h_i] (h: `raw`, slot pair c of dimension i in register i of tile c) -> k
// (dimension i at register i of the lower lane half) and -- when `want` -- tr = sum_i jac_i, for the wave's 32 rows.  The
// parenthesisation is the sequence of roundings the tests pin; the fences keep the image's loads inside the loops.
template <int HT, int NH, int OT>
__device__ __forceinline__ void cnf_exact_dimwise_eval(const cnf_exact_dimwise p, int act, int D, const f32x16 &xin, const cnf_tile<OT> &raw,
                                                       float t, const cnf_tile<HT> &lat, f32x16 &k, bool want, float &tr, int lane) {
    const int h = lane >> 5;
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

// The solve of the wave's 32 rows -- row `row` of x (<= 16 features, the lower lane half) and its latent share, the grid, the stages,
// y / ldj stored for the `live` rows -- is TEXT, not a function: both kernels expand it in their row-group loop, where they had these
// statements, and compile to the code they compiled to before they shared them.  As a function template over an evaluator callable
// (the same statements, __forceinline__) all 24 instantiations are allocated and scheduled differently -- no scratch, the same
// occupancy, registers equal or lower -- and sx_cnf_exact_flow at dim 8 / d_h 4 / [64, 64], 2^18 rows, rk4 x 16 with the log-det
// measured 97.11 ms for 96.50 (+0.6 %, the parent's four rounds span 0.38 ms).  These kernels are 75 .. 285 KB of code, and where
// it lands in the library moves them by as much, so that figure does not condemn the function; the text is kept
// because it alone reproduces the instructions, which makes "nothing changed" a comparison of two files and not a measurement.
// h = lane >> 5, D / L = a.net.dim / latent_dim, want = a.want_ldj != 0, sgn = the grid's direction.  The trailing argument is the
// evaluation k.v[0], q <- f(ts, xs.v[0]) with the latent share `lat`, written over these names of the expansion.  The set kernel's
// evaluation holds __syncthreads(): a.n_steps, the stage count and `want` are uniform over the workgroup, so every wave reaches every
// barrier -- whatever replaces this text must keep that and must be inlined into the kernel's own loop nest.
#define CNF_EXACT_SOLVE_ROWS(HT, a, row, live, h, D, L, want, sgn, lane, ...)                                                     \
    {                                                                                                                             \
        cnf_tile<1> y;                                                                                                            \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) y.v[0][r] = ((live) && (h) == 0 && r < (D)) ? (a).x[(row) * (D) + r] : 0.f; \
        cnf_tile<HT> lat;                                                                                                         \
        cnf_latent_packed<HT>(lat, (a).net.w_latent, (a).latent, row, live, L, lane);                                             \
        float l = 0.f;                                                                                                            \
        const int n_stages = cnf_stages((a).solver);                                                                              \
        const float third = 1.f / 3.f, two_thirds = 2.f / 3.f;                                                                    \
        for (int i = 0; i < (a).n_steps; ++i) {                                                                                   \
            float ta, tb;                                                                                                         \
            cnf_grid(a, sgn, i, ta, tb);                                                                                          \
            const float dt = tb - ta, half = 0.5f * dt;                                                                           \
            cnf_tile<1> k1, k2, xs = y;                                                                                           \
            float q1 = 0.f, q2 = 0.f, ts = ta;                                                                                    \
            /* one copy of the network's code serves every stage: the stage index is wave-uniform */                             \
            for (int st = 0; st < n_stages; ++st) {                                                                               \
                cnf_tile<1> k;                                                                                                    \
                float q = 0.f;                                                                                                    \
                __VA_ARGS__;                                                                                                      \
                cnf_tableau<1>((a).solver, st, ta, tb, dt, half, third, two_thirds, k, q, k1, k2, q1, q2, xs, ts, y, l);          \
            }                                                                                                                     \
        }                                                                                                                         \
        if ((live) && (h) == 0) {                                                                                                 \
            _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                        \
                if (r < (D)) (a).y[(row) * (D) + r] = y.v[0][r];                                                                  \
            if (want) (a).ldj[row] = l;                                                                                           \
        }                                                                                                                         \
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// the fields the two network structs share; `fn`: the prefix of the messages
template <class NET>
inline int cnf_exact_check_net(const char *fn, const NET *net_host, int max_dim, int max_dh, int max_latent, int max_hidden) {
    SX_REQUIRE(net_host != nullptr, "%s: null network", fn);
    const NET &net = *net_host;
    SX_REQUIRE(net.n_hidden == 1 || net.n_hidden == 2, "%s: one or two hidden layers (got %d)", fn, net.n_hidden);
    SX_REQUIRE(net.dim >= 1 && net.dim <= max_dim, "%s: dim must be in 1..%d (got %d)", fn, max_dim, net.dim);
    SX_REQUIRE(net.d_h >= 1 && net.d_h <= max_dh, "%s: d_h must be in 1..%d (got %d)", fn, max_dh, net.d_h);
    SX_REQUIRE(net.latent_dim >= 0 && net.latent_dim <= max_latent, "%s: latent_dim must be in 0..%d (got %d)", fn, max_latent, net.latent_dim);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "%s: activation %d has no in-kernel derivative", fn, net.act);
    for (int l = 0; l < net.n_hidden; ++l)
        SX_REQUIRE(net.hidden[l] >= 1 && net.hidden[l] <= max_hidden, "%s: hidden layer %d must have 1..%d units (got %d)", fn, l, max_hidden,
                   net.hidden[l]);
    return SX_OK;
}

// tiles of the widest hidden layer, tiles of the d_h slots
template <class NET>
inline void cnf_exact_shape(const NET &net, int *HT, int *OT) {
    int ht = cnf_tiles(net.hidden[0]);
    if (net.n_hidden == 2 && cnf_tiles(net.hidden[1]) > ht) ht = cnf_tiles(net.hidden[1]);
    *HT = ht;
    *OT = cnf_out_tiles(net.d_h);
}

// what a flow call checks beyond cnf_check_call: the latent and log-det pointers, the image against the kernel's plan (`image`
// floats), its alignment, and the launch's `lds` bytes (`needs`: the subject of the budget message) against the budget
template <class NET>
inline int cnf_exact_check_flow(const char *fn, const NET &net, const float *latent, const float *ldj, int want_ldj, size_t image, size_t lds,
                                const char *needs) {
    SX_REQUIRE(net.latent_dim == 0 || (latent != nullptr && net.w_latent != nullptr), "%s: latent rows / latent weights missing", fn);
    SX_REQUIRE(!want_ldj || ldj != nullptr, "%s: want_ldj needs ldj", fn);
    SX_REQUIRE(net.image != nullptr && (size_t)net.image_floats == image, "%s: the image holds %d floats, the kernel's plan %zu", fn,
               net.image_floats, image);
    SX_REQUIRE(((uintptr_t)net.image & 15) == 0 && ((uintptr_t)net.w_latent & 15) == 0, "%s: image / w_latent must be 16-byte aligned", fn);
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "%s: %s %zu bytes of LDS (budget %d)", fn, needs, lds, SX_CNF_LDS_BYTES);
    return SX_OK;
}

// the arguments of a flow call; A: a file's argument struct (cnf_exact_args<its network struct>, under the file's own name)
template <class A, class NET>
inline A cnf_exact_fill(const NET &net, const float *x, const float *latent, float *y, float *ldj, int64_t n_rows, int solver, int n_steps,
                        float t0, float t1, float step_size, int want_ldj) {
    A a{};
    a.net = net;
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.want_ldj = want_ldj ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    return a;
}

// the end of an entry point `fn`: return cnf_launch<KERN<HT, NH, OT>>(fn, ...: the arguments, lds, workgroups, stream) for the
// network's tile counts, or the error that there is no such kernel
#define CNF_EXACT_CASE(KERN, H_, O_, fn, HT, NH, OT, ...)                                                                              \
    if ((HT) == H_ && (OT) == O_)                                                                                                      \
        return (NH) == 1 ? cnf_launch<KERN<H_, 1, O_>>(fn, __VA_ARGS__) : cnf_launch<KERN<H_, 2, O_>>(fn, __VA_ARGS__);
#define CNF_EXACT_DISPATCH(KERN, fn, HT, NH, OT, ...)                                                                                  \
    CNF_EXACT_CASE(KERN, 1, 1, fn, HT, NH, OT, __VA_ARGS__) CNF_EXACT_CASE(KERN, 1, 2, fn, HT, NH, OT, __VA_ARGS__)                    \
    CNF_EXACT_CASE(KERN, 1, 4, fn, HT, NH, OT, __VA_ARGS__) CNF_EXACT_CASE(KERN, 2, 1, fn, HT, NH, OT, __VA_ARGS__)                    \
    CNF_EXACT_CASE(KERN, 2, 2, fn, HT, NH, OT, __VA_ARGS__) CNF_EXACT_CASE(KERN, 2, 4, fn, HT, NH, OT, __VA_ARGS__)                    \
    sx_set_error("%s: no kernel for %d hidden x %d output tiles", fn, HT, OT);                                                         \
    return SX_E_BADARG

}  // namespace
