// Continuous normalizing flow over a DiffeqMLP (ContinuousTransform, stribor/flows/cnf.py:13-262) under the PER-SAMPLE adaptive solver
// 'dopri5_per_sample' of DESIGN.md "CNF", in one launch per call.
//
// sx_cnf_adaptive_flow -- Dormand-Prince 5(4) with FSAL, one step-size controller per ROW:
//   * layout, staging and arithmetic are sx_cnf.hip's (one wave = 32 rows on the MFMA column, weights and the trace constants in
//     LDS once per workgroup, exact fp32 v_mfma_f32_32x32x2_f32, -ffp-contract=off); the layers are sx_cnf_dense.h's macros;
//   * time is PER ROW: in DiffeqMLP it is the first input column, so the first layer's time term is t_row * W1[:, 0] with t_row a
//     per-lane value (CNF_DENSE_H1 takes it as written: its `t` is an expression inside a per-lane product);
//   * every row carries its own s (the time integrated so far), dt, attempt counters and done flag; the two lane halves of a row
//     compute them from the same bits.  The wave attempts steps while any of its rows is live (a ballot): finished rows attempt a
//     step of 0 and keep their state, rejected rows keep theirs, both by selects -- there is no divergent branch around an MFMA;
//   * one copy of the network's code serves the six evaluations of an attempt: the stage index is wave-uniform and indexes the
//     coefficient table; the seven stage vectors of the one-tile state stay in registers (7 x 16 of the 512);
//   * the loop ends: every trip either finishes a row or counts an attempt against max_num_steps.
// A row that fails (step cap, step-size underflow, non-finite error ratio) ends as NaN with a status code; nothing else is touched.
//
// Coverage: dim <= 32, 1 + dim + latent_dim <= 128, one or two hidden layers of <= 64 units, the activations of sx_cnf_flow.
//
// The trace (ad_eval) restates cn_eval of sx_cnf.hip with C always in LDS: that function stays in its file because moving it
// changes the register allocation of cnf_flow_kernel<1, 4, 2> (see the header of sx_cnf.hip).
#include "sx_cnf_dense.h"

#define SX_CNF_ADAPTIVE_MAX_DIM    32
#define SX_CNF_ADAPTIVE_MAX_HIDDEN 64
#define SX_CNF_ADAPTIVE_MAX_STEPS  (1 << 20)

namespace {

// The tableau (DESIGN.md "CNF").  Row st = the weights of k1 .. k6 in the input of stage st + 1; row 6 is b (a7 = b: FSAL), so the
// input of the seventh evaluation is the step itself.  Each entry is the fp32 rounding of the fp64 quotient.
#define F(x) ((float)(x))
__device__ const float ad_a[7][6] = {
    {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {F(1.0 / 5.0), 0.f, 0.f, 0.f, 0.f, 0.f},
    {F(3.0 / 40.0), F(9.0 / 40.0), 0.f, 0.f, 0.f, 0.f},
    {F(44.0 / 45.0), F(-56.0 / 15.0), F(32.0 / 9.0), 0.f, 0.f, 0.f},
    {F(19372.0 / 6561.0), F(-25360.0 / 2187.0), F(64448.0 / 6561.0), F(-212.0 / 729.0), 0.f, 0.f},
    {F(9017.0 / 3168.0), F(-355.0 / 33.0), F(46732.0 / 5247.0), F(49.0 / 176.0), F(-5103.0 / 18656.0), 0.f},
    {F(35.0 / 384.0), 0.f, F(500.0 / 1113.0), F(125.0 / 192.0), F(-2187.0 / 6784.0), F(11.0 / 84.0)},
};
__device__ const float ad_c[7] = {0.f, F(1.0 / 5.0), F(3.0 / 10.0), F(4.0 / 5.0), F(8.0 / 9.0), 1.f, 1.f};
// e = b - b*: the weights of k1 .. k7 in the error estimate
__device__ const float ad_e[7] = {F(35.0 / 384.0 - 5179.0 / 57600.0), 0.f, F(500.0 / 1113.0 - 7571.0 / 16695.0), F(125.0 / 192.0 - 393.0 / 640.0),
                                  F(-2187.0 / 6784.0 + 92097.0 / 339200.0), F(11.0 / 84.0 - 187.0 / 2100.0), F(-1.0 / 40.0)};
#undef F

struct ad_args : cnf_dense_args {
    int base_tr;            // LDS float offset of c (one hidden layer) or C (two)
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int32_t *stats;
    int64_t n_rows;
    int max_steps, want_trace;
    float t0, t1, rtol, atol, first_step;
};

// max / min that keep a NaN (fmaxf / fminf drop it): a row whose error ratio is not a number must fail, not pass
__device__ __forceinline__ float ad_nmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float ad_nmin(float a, float b) { return (a < b || a != a) ? a : b; }

// k = sgn f(t, xin) and -- when `want` -- tr = sgn tr df/dx for the wave's 32 rows, t PER LANE (cn_eval of sx_cnf.hip otherwise)
template <int DT, int HT, int NH>
__device__ __forceinline__ void ad_eval(const ad_args &a, const cnf_tile<DT> &xin, float t, const cnf_tile<HT> &lat, float sgn, cnf_tile<DT> &k,
                                        bool want, float &tr, int lane) {
    const int h = lane >> 5, act = a.net.act;
    const f32x16 ones = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
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
                else d = ones;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += d[r] * cnf_vec(cv, m, r);
            }
        }
        CNF_DENSE_OUT(DT, HT, 1, a, h1, k, lane, h);
    } else {
        cnf_tile<HT> h2;
        CNF_DENSE_H2(HT, false, a, h1, h2, lane, h, act);
        if (want) {
            // h1 <- d1, then v = C d1 one 32-row tile at a time, consumed at once: s += d2 . v
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                if (act != SX_ACT_IDENTITY) cnf_dact_tile(h1.v[m], act);
                else h1.v[m] = ones;
            }
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                f32x16 v = {};
                cnf_mma<HT>(v, h1, cnf_smem + a.base_tr + m * HT * 1024 + lane * 4);
                f32x16 d = h2.v[m];
                if (act != SX_ACT_IDENTITY) cnf_dact_tile(d, act);
                else d = ones;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += d[r] * v[r];
            }
        }
        asm volatile("" ::: "memory");
        CNF_DENSE_OUT(DT, HT, 2, a, h2, k, lane, h);
    }
#pragma unroll
    for (int c = 0; c < DT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) k.v[c][r] = sgn * k.v[c][r];
    tr = want ? sgn * (s + __shfl_xor(s, 32, 64)) : 0.f;          // the two lane halves hold the two feature halves of a row
}

// rms over the row's D features of num / den (the padded features stay out; both lane halves of a row get the same bits)
template <int DT>
__device__ __forceinline__ float ad_rms(const cnf_tile<DT> &num, const cnf_tile<DT> &den, int D, int h) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float q = num.v[c][r] / den.v[c][r];
            s = s + ((32 * c + sx_kmap(r, h) < D) ? q * q : 0.f);
        }
    s = s + __shfl_xor(s, 32, 64);
    return sqrtf(s / (float)D);
}

template <int DT, int HT, int NH>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_adaptive_kernel(const ad_args a) {
    const sx_cnf_net &net = a.net;
    const int D = net.dim, H1 = net.layer[0].out_dim;
    cnf_dense_stage<DT, HT, NH>(a);
    if (NH == 1) cnf_stage_vec(a.want_trace ? net.trace : nullptr, H1, 1, HT * 32, a.base_tr);
    else if (a.want_trace) cnf_stage(net.trace, HT * 32, HT * 32, HT * 32, 0, HT, HT, a.base_tr);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const bool want = a.want_trace != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f, T = fabsf(a.t1 - a.t0), rtol = a.rtol, atol = a.atol;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_CNF_WAVES + (threadIdx.x >> 6); grp < n_groups;
         grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        cnf_tile<DT> y, xs, k, K[7];
        cnf_tile<HT> lat;
        cnf_load_row<DT>(y, a.x, row, D, live, h);
        cnf_dense_latent<HT>(a, lat, a.latent, row, live, lane);
        float Q[7], q = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            Q[j] = 0.f;
#pragma unroll
            for (int c = 0; c < DT; ++c) K[j].v[c] = f32x16{};
        }
        ad_eval<DT, HT, NH>(a, y, a.t0, lat, sgn, K[0], want, Q[0], lane);
        float l = 0.f, s = 0.f, dt = a.first_step;
        if (!(a.first_step > 0.f)) {
            // the first step by Hairer's rule: scale = atol + rtol |y0| (the trace share starts at 0: its scale is atol)
            cnf_tile<DT> sc;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc.v[c][r] = atol + rtol * fabsf(y.v[c][r]);
            const float d0 = ad_rms<DT>(y, sc, D, h);
            const float d1 = ad_nmax(ad_rms<DT>(K[0], sc, D, h), want ? fabsf(Q[0]) / atol : 0.f);
            const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) xs.v[c][r] = y.v[c][r] + h0 * K[0].v[c][r];
            ad_eval<DT, HT, NH>(a, xs, a.t0 + sgn * h0, lat, sgn, k, want, q, lane);
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) k.v[c][r] = k.v[c][r] - K[0].v[c][r];
            const float d2 = ad_nmax(ad_rms<DT>(k, sc, D, h), want ? fabsf(q - Q[0]) / atol : 0.f) / h0;
            const float h1 = (d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, 1e-3f * h0) : powf(0.01f / ad_nmax(d1, d2), 0.2f);
            dt = ad_nmin(100.f * h0, h1);
        }
        int n_att = 0, n_acc = 0, n_rej = 0, status = 0;
        bool done = !live || !(T > 0.f);
        while (true) {
            const float rem = T - s;
            const bool last = dt >= rem;
            float hs = last ? rem : dt;
            if (!done && n_att >= a.max_steps) { status = 1; done = true; }
            if (!done && s + hs == s) { status = 2; done = true; }
            if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
            const bool act = !done;
            if (!act) hs = 0.f;
            n_att += act ? 1 : 0;
            // one copy of the network's code serves the six evaluations: the stage index is wave-uniform
#pragma nounroll
            for (int st = 1; st < 7; ++st) {
#pragma unroll
                for (int c = 0; c < DT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float acc = ad_a[st][0] * K[0].v[c][r];
#pragma unroll
                        for (int j = 1; j < 6; ++j) acc = acc + ad_a[st][j] * K[j].v[c][r];
                        xs.v[c][r] = y.v[c][r] + hs * acc;
                    }
                ad_eval<DT, HT, NH>(a, xs, a.t0 + sgn * (s + ad_c[st] * hs), lat, sgn, k, want, q, lane);
#pragma unroll
                for (int j = 1; j < 7; ++j)
                    if (st == j) { K[j] = k; Q[j] = q; }
            }
            // xs is the step (row 6 of the table is b); the trace's step, the error estimate and its ratio to the tolerance
            float qa = ad_a[6][0] * Q[0], qe = ad_e[0] * Q[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) qa = qa + ad_a[6][j] * Q[j];
#pragma unroll
            for (int j = 1; j < 7; ++j) qe = qe + ad_e[j] * Q[j];
            const float l1 = l + hs * qa, err_a = hs * qe;
            cnf_tile<DT> tol;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float acc = ad_e[0] * K[0].v[c][r];
#pragma unroll
                    for (int j = 1; j < 7; ++j) acc = acc + ad_e[j] * K[j].v[c][r];
                    k.v[c][r] = hs * acc;
                    tol.v[c][r] = atol + rtol * fmaxf(fabsf(y.v[c][r]), fabsf(xs.v[c][r]));
                }
            const float ra = want ? fabsf(err_a) / (atol + rtol * fmaxf(fabsf(l), fabsf(l1))) : 0.f;
            const float ratio = ad_nmax(ad_rms<DT>(k, tol, D, h), ra);
            const bool finite = ratio - ratio == 0.f;
            const bool accept = act && finite && ratio <= 1.f;
            float factor = 10.f;
            if (ratio != 0.f) factor = fminf(10.f, fmaxf(0.9f * powf(ratio, -0.2f), ratio < 1.f ? 1.f : 0.2f));
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    y.v[c][r] = accept ? xs.v[c][r] : y.v[c][r];
                    K[0].v[c][r] = accept ? K[6].v[c][r] : K[0].v[c][r];
                }
            Q[0] = accept ? Q[6] : Q[0];
            l = accept ? l1 : l;
            s = accept ? (last ? T : s + hs) : s;
            n_acc += accept ? 1 : 0;
            n_rej += (act && !accept) ? 1 : 0;
            if (act && !finite) { status = 2; done = true; }
            if (accept && last) done = true;
            dt = act ? hs * factor : dt;
        }
        if (status != 0) {
            l = __builtin_nanf("");
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) y.v[c][r] = __builtin_nanf("");
        }
        cnf_store_row<DT>(a.y, y, row, D, live, h);
        if (live && h == 0) {
            if (want) a.ldj[row] = l;
            a.stats[row * 3 + 0] = n_acc;
            a.stats[row * 3 + 1] = n_rej;
            a.stats[row * 3 + 2] = status;
        }
    }
}

// the LDS plan: the forward images, then c / C (always in LDS: at most 64 x 64 floats).  -> floats used
size_t ad_plan(const sx_cnf_net &net, ad_args &a) {
    const int NH = net.n_layers - 1, HT = cnf_dense_hidden_tiles(net);
    size_t off = cnf_dense_plan(net, a);
    a.base_tr = (int)off;
    off += NH == 1 ? (size_t)HT * 32 : (size_t)HT * HT * 1024;
    return off;
}

int ad_check_net(const sx_cnf_net *net_host) {
    return cnf_dense_check_net("sx_cnf_adaptive_flow", net_host, SX_CNF_ADAPTIVE_MAX_DIM, 128, SX_CNF_ADAPTIVE_MAX_HIDDEN);
}

}  // namespace

extern "C" size_t sx_cnf_adaptive_lds_bytes(const sx_cnf_net *net_host) {
    if (ad_check_net(net_host) != SX_OK) return 0;
    ad_args a{};
    return ad_plan(*net_host, a) * 4;
}

extern "C" int sx_cnf_adaptive_flow(const sx_cnf_net *net_host, const float *x, const float *latent, float *y, float *ldj, int32_t *stats,
                                    int64_t n_rows, float t0, float t1, float rtol, float atol, float first_step, int32_t max_num_steps,
                                    int32_t want_trace, void *stream) {
    const int rc = ad_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_net &net = *net_host;
    SX_REQUIRE(n_rows >= 0, "sx_cnf_adaptive_flow: negative n_rows");
    SX_REQUIRE(x != nullptr && y != nullptr && stats != nullptr, "sx_cnf_adaptive_flow: null input / output / stats");
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "sx_cnf_adaptive_flow: latent rows missing");
    SX_REQUIRE(!want_trace || (ldj != nullptr && net.trace != nullptr), "sx_cnf_adaptive_flow: want_trace needs ldj and the trace constants");
    SX_REQUIRE(t0 - t0 == 0.f && t1 - t1 == 0.f, "sx_cnf_adaptive_flow: t0 and t1 must be finite");
    SX_REQUIRE(rtol >= 0.f && atol >= 0.f && rtol - rtol == 0.f && atol - atol == 0.f, "sx_cnf_adaptive_flow: rtol and atol must be finite and >= 0");
    SX_REQUIRE(first_step == first_step, "sx_cnf_adaptive_flow: first_step is not a number");
    SX_REQUIRE(max_num_steps >= 1 && max_num_steps <= SX_CNF_ADAPTIVE_MAX_STEPS, "sx_cnf_adaptive_flow: max_num_steps must be in 1..%d (got %d)",
               SX_CNF_ADAPTIVE_MAX_STEPS, max_num_steps);
    ad_args a{};
    a.net = net;
    const size_t lds = ad_plan(net, a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_adaptive_flow: the padded weights need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.stats = stats; a.n_rows = n_rows;
    a.max_steps = max_num_steps; a.want_trace = want_trace ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.rtol = rtol; a.atol = atol; a.first_step = first_step;
    const int NH = net.n_layers - 1, HT = cnf_dense_hidden_tiles(net);
    const int64_t want = cnf_row_blocks(n_rows);
    if (HT == 1)
        return NH == 1 ? cnf_launch<cnf_adaptive_kernel<1, 1, 1>>("sx_cnf_adaptive_flow", a, lds, want, stream)
                       : cnf_launch<cnf_adaptive_kernel<1, 1, 2>>("sx_cnf_adaptive_flow", a, lds, want, stream);
    return NH == 1 ? cnf_launch<cnf_adaptive_kernel<1, 2, 1>>("sx_cnf_adaptive_flow", a, lds, want, stream)
                   : cnf_launch<cnf_adaptive_kernel<1, 2, 2>>("sx_cnf_adaptive_flow", a, lds, want, stream);
}
