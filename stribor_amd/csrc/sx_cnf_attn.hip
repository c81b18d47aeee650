// Continuous normalizing flow over SETS with self attention (ContinuousTransform with set_data / 'compute_set', stribor/flows/cnf.py:13-262,
// over net/diffeq.py:97-113's DiffeqSelfAttention = DiffeqConcat around net/attention.py's SelfAttention) on a fixed grid, in one launch.
//
// sx_cnf_attn_flow -- rows are set elements, the N = set_size elements of a set contiguous.  With u_i = [t, x_i, latent_i], the three
// embeddings q, k, v (one Linear, or Linear - act - Linear, E outputs), H heads of width dh = E / H, scale = dh^-1/2, per head
//     s_ij = scale q_i . k_j   (mask_diagonal: s_ii = -inf),   p_i = safe_softmax_j(s_ij),   o_i = sum_j p_ij v_j,   f_i = P o_i + b
// and the divergence of the whole set's dynamics, per element, has the closed form of DESIGN.md "CNF on sets with attention": for a
// coordinate d the forward tangent (qd, kd, vd) of x_i[d] through element i's own embeddings gives
//     sd_ij = scale qd_i . k_j + [i == j] scale q_i . kd_i        (the second term is absent under mask_diagonal, where p_ii = 0)
//     od_i  = sum_j p_ij sd_ij v_j - (sum_m p_im sd_im) o_i + p_ii vd_i,        tr_i += P[d, :] . od_i.
//   * the conventions of sx_cnf_common.h: one wave = 32 rows on the MFMA column, features on the C rows, exact fp32
//     (v_mfma_f32_32x32x2_f32), weights in LDS in A-fragment order, state / stage vectors / log-det in registers for the whole grid,
//     the same solvers, grid, tableau roundings (-ffp-contract=off) and activations;
//   * a workgroup of 4 waves owns 128 row slots and takes floor(128 / N) WHOLE sets per pass: sets never straddle workgroups, they
//     may straddle waves.  Slots past the last set are padding: they compute on zeros, attend to themselves and are never stored;
//   * the exchange: per evaluation every lane writes its row's k and v (E floats each, row stride 36) to one of TWO exchange areas in
//     LDS (they alternate, so one workgroup barrier per evaluation is enough: nobody writes area b again before everybody has passed
//     the barrier that follows the reads of area b).  Every wave reaches that barrier (padding waves included): the pass loop, the
//     stage loop and `want` are uniform over the workgroup.  N = 1 needs no exchange: o = v_i, or 0 under mask_diagonal;
//   * scores: the keys of a 32-slot tile are the A operand (from the exchange area), the wave's 32 queries the B operand -- a lane then
//     holds the scores of its query against the 16 keys kmap(r, h) of the tile, and the softmax reductions are in-register plus one
//     exchange between the two lane halves.  A wave visits the key tiles that can hold rows of its own sets; keys of other sets,
//     padding slots and (mask_diagonal) the row itself are masked before the maximum.  A head contracts its own features only: the
//     query operand is zero outside the head (0 * k adds an exact 0), and 8-feature groups no feature of which is the head's are
//     skipped.  Max-subtracted softmax (expf), the maximum and the sum taken in one sweep over the tiles, p in a second one;
//   * P.V: the values of a tile transposed are the A operand (zero outside the head's features), the scores' own fragment is the B
//     operand; the heads accumulate into one tile;
//   * under want_ldj the same again per coordinate d (one at a time) with the tangent query and the two diagonal terms; with
//     want_ldj == 0 none of the tangent work runs;
//   * non-finite values: a k / v value that is not finite is written to the exchange area as 0 and raises its set's flag in LDS (so does
//     a NaN hidden unit of the k / v embeddings under ReLU, which fmaxf would turn into 0 where torch keeps the NaN); a
//     flagged set is stored as NaN in every element (as the reference's 0 * NaN inside p @ v makes it) and no other set of the
//     workgroup sees it (a zero weight times a NaN inside a shared MFMA would otherwise poison its neighbours);
//   * time: per stage the first layers' bias is b1 + t W1[:, 0].  The latent columns ride in the state tile behind x (dim + latent_dim
//     <= 32: the first layers' GEMM contracts one 32-feature tile either way, so this costs no MFMA and no register, where a separate
//     latent GEMM per pass would keep 3 x HT more tiles -- 96 registers at HT = 2, against the 10 the <2, 2> build has left -- alive for
//     the whole grid); their derivative is an exact 0.
//
// Coverage: 1 <= N <= 128, dim <= 8, 1 + dim + latent_dim <= 33, embeddings [E] or [H1, E] with H1 <= 64 and E <= 32, 1, 2 or 4 heads
// (dividing E), the seven activations of sx_cnf_common.h, biases present, no mask.
#include "sx_cnf_attn_common.h"

namespace {

struct ca_args {
    sx_cnf_attn_net net;
    int base_a1[3], base_b1[3], base_w0[3], base_wx[3];     // LDS float offsets: first layers, their biases, time and x columns
    int base_a2[3], base_b2[3];                             // ... second layers (one hidden layer)
    int base_p, base_pb, base_pr;                           // ... the projection's image, bias and rows
    int base_x, base_flag;                                  // ... the two exchange areas [2][k, v][SX_CNF_ROWS][CA_LD], the set flags
    float scale;
    const float *x;
    const float *latent;
    float *y;
    float *ldj;
    int64_t n_rows;
    int solver, n_steps, want_ldj;
    float t0, t1, step_size;
};

// element hd (uniform, 0..3) of four per-head scalars kept in registers
__device__ __forceinline__ float ca_get(const float (&v)[4], int hd) { return hd == 0 ? v[0] : hd == 1 ? v[1] : hd == 2 ? v[2] : v[3]; }
__device__ __forceinline__ void ca_put(float (&v)[4], int hd, float x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = hd == i ? x : v[i];
}

// f(t, x) and -- when `want` -- tr = the row's share of the set's divergence, for the wave's 32 rows.  `area`: which exchange area
template <int HT, int NH>
__device__ __forceinline__ void ca_eval(const ca_args &a, const ca_pos &p, const f32x16 &xin, float t, int area,
                                        f32x16 &kout, bool want, float &tr, int lane) {
    const int h = lane >> 5, act = a.net.act, D = a.net.dim, H = a.net.n_heads, dh = a.net.embed / H, N = a.net.set_size;
    const bool md = a.net.mask_diagonal != 0;
    const float scale = a.scale;
    // (keeps the loop-invariant LDS weight loads inside the step loop: without it the compiler holds whole matrices in registers)
    asm volatile("" ::: "memory");
    cnf_tile<1> xi;
    xi.v[0] = xin;
    f32x16 z[3];                           // q, k, v
    cnf_tile<HT> d1[3];                    // one hidden layer: act'(hidden) of the three embeddings (when `want`)
    bool bad = false;                      // the row's k or v is not finite (or would not be in torch): its set is flagged
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const float *b1 = cnf_smem + a.base_b1[e] + 4 * h, *w0 = cnf_smem + a.base_w0[e] + 4 * h;
        cnf_tile<HT> h1;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            f32x16 acc = {};
            cnf_mma<1>(acc, xi, cnf_smem + a.base_a1[e] + m * 1024 + lane * 4);
#pragma unroll
            for (int r = 0; r < 16; ++r) h1.v[m][r] = acc[r] + (cnf_vec(b1, m, r) + t * cnf_vec(w0, m, r));
        }
        if (NH == 1) {
            z[e] = h1.v[0];
        } else {
            // cnf_act's ReLU is fmaxf(v, 0), which turns a NaN into 0 where torch keeps it: a NaN hidden unit of k or v counts as a NaN k or v
            if (e > 0 && act == SX_ACT_RELU) {
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) bad = bad || h1.v[m][r] != h1.v[m][r];
            }
            cnf_act_all<HT>(h1, act);
            f32x16 acc = {};
            cnf_mma<HT>(acc, h1, cnf_smem + a.base_a2[e] + lane * 4);
            const float *b2 = cnf_smem + a.base_b2[e] + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[e][r] = acc[r] + cnf_vec(b2, 0, r);
            if (want) {
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) d1[e].v[m][r] = cnf_dact(h1.v[m][r], act);
            }
        }
    }
    const float *xk = cnf_smem + a.base_x + area * (2 * CA_AREA), *xv = xk + CA_AREA;
    f32x16 o = {};
    float mh[4] = {0.f, 0.f, 0.f, 0.f}, il[4] = {0.f, 0.f, 0.f, 0.f}, pii[4] = {0.f, 0.f, 0.f, 0.f};
    if (N == 1) {
        if (!md) o = z[2];
    } else {
        {
            float *mk = cnf_smem + a.base_x + area * (2 * CA_AREA) + p.rho * CA_LD + 4 * h, *mv = mk + CA_AREA;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<f32x4 *>(mk + 8 * g) = f32x4{ca_finite(z[1][4 * g], bad), ca_finite(z[1][4 * g + 1], bad),
                                                               ca_finite(z[1][4 * g + 2], bad), ca_finite(z[1][4 * g + 3], bad)};
                *reinterpret_cast<f32x4 *>(mv + 8 * g) = f32x4{ca_finite(z[2][4 * g], bad), ca_finite(z[2][4 * g + 1], bad),
                                                               ca_finite(z[2][4 * g + 2], bad), ca_finite(z[2][4 * g + 3], bad)};
            }
            if (bad) reinterpret_cast<int *>(cnf_smem + a.base_flag)[p.first] = 1;
        }
        __syncthreads();
#pragma nounroll
        for (int hd = 0; hd < H; ++hd) {
            {
                asm volatile("" ::: "memory");
                const int lo = hd * dh, hi = lo + dh;
                const bool e_in = (lane & 31) >= lo && (lane & 31) < hi;
                f32x16 qm;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = sx_kmap(r, h);
                    qm[r] = (f >= lo && f < hi) ? z[0][r] : 0.f;
                }
                float m = -INFINITY, l = 0.f;
#pragma nounroll
                for (int kt = p.kt_lo; kt <= p.kt_hi; ++kt) {
                    f32x16 s = ca_scores(qm, xk + (32 * kt + (lane & 31)) * CA_LD + 4 * h, lo, hi);
                    float tmax = -INFINITY;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        s[r] = ca_valid(p, 32 * kt + sx_kmap(r, h), md) ? s[r] * scale : -INFINITY;
                        tmax = fmaxf(tmax, s[r]);
                    }
                    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
                    const float m_new = fmaxf(m, tmax), m_use = m_new == -INFINITY ? 0.f : m_new;
                    float ts = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) ts += s[r] == -INFINITY ? 0.f : expf(s[r] - m_use);
                    ts = ts + __shfl_xor(ts, 32, 64);
                    l = l * expf(m - m_use) + ts;
                    m = m_new;
                }
                const float mu = m == -INFINITY ? 0.f : m;
                const float inv = l > 0.f ? 1.f / l : l != l ? l : 0.f;          // (a fully masked row: zeros; a NaN sum stays NaN)
                ca_put(mh, hd, mu);
                ca_put(il, hd, inv);
                float own = 0.f;
#pragma nounroll
                for (int kt = p.kt_lo; kt <= p.kt_hi; ++kt) {
                    f32x16 s = ca_scores(qm, xk + (32 * kt + (lane & 31)) * CA_LD + 4 * h, lo, hi);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int js = 32 * kt + sx_kmap(r, h);
                        s[r] = ca_valid(p, js, md) ? expf(s[r] * scale - mu) * inv : 0.f;
                        own += js == p.rho ? s[r] : 0.f;
                    }
                    ca_pv(o, s, xv + (32 * kt + 4 * h) * CA_LD + (lane & 31), e_in);
                }
                ca_put(pii, hd, own + __shfl_xor(own, 32, 64));
            }
        }
    }
    {
        cnf_tile<1> ot;
        ot.v[0] = o;
        f32x16 acc = {};
        cnf_mma<1>(acc, ot, cnf_smem + a.base_p + lane * 4);
        const float *pb = cnf_smem + a.base_pb + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) kout[r] = acc[r] + cnf_vec(pb, 0, r);
    }
    if (!want) return;
    float trs = 0.f;
#pragma nounroll
    for (int d = 0; d < D; ++d) {
        asm volatile("" ::: "memory");
        f32x16 zd[3];                      // the tangents of q, k, v along x_i[d]
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float *wx = cnf_smem + a.base_wx[e] + d * (32 * HT) + 4 * h;
            if (NH == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) zd[e][r] = cnf_vec(wx, 0, r);
            } else {
                cnf_tile<HT> tt;
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tt.v[m][r] = d1[e].v[m][r] * cnf_vec(wx, m, r);
                f32x16 acc = {};
                cnf_mma<HT>(acc, tt, cnf_smem + a.base_a2[e] + lane * 4);
                zd[e] = acc;
            }
        }
        // tr_d = P[d, :] . od with od = u - c o + p_ii vd per head: only the dot products are kept (pr: the projection's row d)
        const float *pr = cnf_smem + a.base_pr + 32 * d + 4 * h;
        float s = 0.f;
        if (N == 1) {
            if (!md) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s += cnf_vec(pr, 0, r) * zd[2][r];
            }
        } else {
            // the two diagonal terms need kd and vd of the row itself only: own[hd] = scale q_i . kd_i, and p_ii P[d, :] . vd_i
            float own[4] = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
            for (int hd = 0; hd < H; ++hd) {
                const int lo = hd * dh, hi = lo + dh;
                const float self = ca_get(pii, hd);
                float dot = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = sx_kmap(r, h);
                    const bool in = f >= lo && f < hi;
                    dot += in ? z[0][r] * zd[1][r] : 0.f;
                    s += in ? cnf_vec(pr, 0, r) * (self * zd[2][r]) : 0.f;
                }
                ca_put(own, hd, md ? 0.f : (dot + __shfl_xor(dot, 32, 64)) * scale);
            }
            f32x16 u = {};
#pragma nounroll
            for (int hd = 0; hd < H; ++hd) {
                asm volatile("" ::: "memory");
                const int lo = hd * dh, hi = lo + dh;
                const bool e_in = (lane & 31) >= lo && (lane & 31) < hi;
                const float mu = ca_get(mh, hd), inv = ca_get(il, hd), own_h = ca_get(own, hd);
                f32x16 qm, qdm;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = sx_kmap(r, h);
                    const bool in = f >= lo && f < hi;
                    qm[r] = in ? z[0][r] : 0.f;
                    qdm[r] = in ? zd[0][r] : 0.f;
                }
                float c = 0.f;
#pragma nounroll
                for (int kt = p.kt_lo; kt <= p.kt_hi; ++kt) {
                    const float *kb = xk + (32 * kt + (lane & 31)) * CA_LD + 4 * h;
                    const f32x16 sc = ca_scores(qm, kb, lo, hi);
                    f32x16 w = ca_scores(qdm, kb, lo, hi);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int js = 32 * kt + sx_kmap(r, h);
                        const float pj = expf(sc[r] * scale - mu) * inv;
                        const float sd = w[r] * scale + (js == p.rho ? own_h : 0.f);
                        w[r] = ca_valid(p, js, md) ? pj * sd : 0.f;
                        c += w[r];
                    }
                    ca_pv(u, w, xv + (32 * kt + 4 * h) * CA_LD + (lane & 31), e_in);
                }
                c = c + __shfl_xor(c, 32, 64);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = sx_kmap(r, h);
                    s += (f >= lo && f < hi) ? cnf_vec(pr, 0, r) * (u[r] - c * o[r]) : 0.f;
                }
            }
        }
        trs += s;
    }
    tr = trs + __shfl_xor(trs, 32, 64);
}

template <int HT, int NH>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_attn_flow_kernel(const ca_args a) {
    const sx_cnf_attn_net &net = a.net;
    const int D = net.dim, L = net.latent_dim, in_dim = 1 + D + L, E = net.embed, N = net.set_size;
    const int n1 = NH == 1 ? E : net.hidden[0];               // rows of the first layers
    for (int e = 0; e < 3; ++e) {
        cnf_stage(net.W1[e], n1, D + L, in_dim, 1, HT, 1, a.base_a1[e]);
        cnf_stage_vec(net.b1[e], n1, 1, HT * 32, a.base_b1[e]);
        cnf_stage_vec(net.W1[e], n1, in_dim, HT * 32, a.base_w0[e]);
        if (a.want_ldj)
            for (int d = 0; d < D; ++d) cnf_stage_vec(net.W1[e] + 1 + d, n1, in_dim, HT * 32, a.base_wx[e] + d * (HT * 32));
        if (NH == 2) {
            cnf_stage(net.W2[e], E, n1, n1, 0, 1, HT, a.base_a2[e]);
            cnf_stage_vec(net.b2[e], E, 1, 32, a.base_b2[e]);
        }
    }
    cnf_stage(net.P, D, E, E, 0, 1, 1, a.base_p);
    cnf_stage_vec(net.pb, D, 1, 32, a.base_pb);
    if (a.want_ldj)
        for (int d = 0; d < D; ++d) cnf_stage_vec(net.P + (int64_t)d * E, E, 1, 32, a.base_pr + 32 * d);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_passes = cnf_set_passes(N, a.n_rows);
    int *flags = reinterpret_cast<int *>(cnf_smem + a.base_flag);
    cnf_set_pos sp;
    ca_pos p;
    p.rho = sp.rho = wave * 32 + (lane & 31);          // (cnf_set_slot, spelt with this kernel's `wave`: the call compiles to other code)
    int area = 0;
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        cnf_set_pass(sp, pass, N, a.n_rows);
        const int n_here = sp.n_here;
        const bool live = sp.live;
        const int64_t row = sp.row;
        p.first = sp.first;
        p.n = live ? N : 1;
        if (32 * wave < n_here) {
            const int last = 32 * wave + 31 < n_here - 1 ? 32 * wave + 31 : n_here - 1;
            const int hi_end = (last / N) * N + N - 1;
            p.kt_lo = ((32 * wave / N) * N) >> 5;
            p.kt_hi = (hi_end >> 5) > wave ? (hi_end >> 5) : wave;
        } else {
            p.kt_lo = p.kt_hi = wave;
        }
        if (N > 1) {
            if (threadIdx.x < SX_CNF_ROWS) flags[threadIdx.x] = 0;
            __syncthreads();
        }
        // the state tile: x at features 0 .. D - 1, the row's latent behind it (its derivative is an exact 0: the projection's image and
        // bias are zero there, so every stage leaves it as it is)
        cnf_tile<1> y;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = sx_kmap(r, h);
            y.v[0][r] = !live ? 0.f : f < D ? a.x[row * D + f] : f < D + L ? a.latent[row * L + (f - D)] : 0.f;
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
                ca_eval<HT, NH>(a, p, xs.v[0], ts, area, k.v[0], want, q, lane);
                area ^= 1;
                cnf_tableau<1>(a.solver, st, ta, tb, dt, half, third, two_thirds, k, q, k1, k2, q1, q2, xs, ts, y, l);
            }
        }
        bool poison = false;
        if (N > 1) {
            poison = flags[p.first] != 0;
            __syncthreads();                // the flags are read: the next pass may clear them
        }
        if (live) {
            const float nan = __builtin_nanf("");
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = sx_kmap(r, h);
                if (f < D) a.y[row * D + f] = poison ? nan : y.v[0][r];
            }
            if (want && h == 0) a.ldj[row] = poison ? nan : l;
        }
    }
}

// the LDS plan: float offsets into `a` (may be null), -> floats used
size_t ca_plan(const sx_cnf_attn_net &net, ca_args *a) {
    const int NH = net.n_hidden + 1, HT = NH == 1 ? 1 : cnf_tiles(net.hidden[0]);
    size_t off = 0;
    ca_args unused{};
    ca_args &t = a ? *a : unused;
    const auto take = [&off](size_t floats) { const int at = (int)off; off += floats; return at; };
    for (int e = 0; e < 3; ++e) {
        t.base_a1[e] = take((size_t)HT * 1024);
        t.base_b1[e] = take((size_t)HT * 32);
        t.base_w0[e] = take((size_t)HT * 32);
        t.base_wx[e] = take((size_t)net.dim * HT * 32);
        if (NH == 2) {
            t.base_a2[e] = take((size_t)HT * 1024);
            t.base_b2[e] = take(32);
        }
    }
    t.base_p = take(1024);
    t.base_pb = take(32);
    t.base_pr = take((size_t)net.dim * 32);
    t.base_x = take((size_t)4 * CA_AREA);
    t.base_flag = take(SX_CNF_ROWS);
    return off;
}

// the shape of the network alone (no pointer is read)
int ca_check_shape(const sx_cnf_attn_net *net_host) {
    SX_REQUIRE(net_host != nullptr, "sx_cnf_attn_flow: null network");
    const sx_cnf_attn_net &net = *net_host;
    SX_REQUIRE(net.n_hidden == 0 || net.n_hidden == 1, "sx_cnf_attn_flow: embeddings of one or two Linear layers (got %d hidden layers)", net.n_hidden);
    SX_REQUIRE(net.dim >= 1 && net.dim <= SX_CNF_ATTN_MAX_DIM, "sx_cnf_attn_flow: dim must be in 1..%d (got %d)", SX_CNF_ATTN_MAX_DIM, net.dim);
    SX_REQUIRE(net.latent_dim >= 0 && 1 + net.dim + net.latent_dim <= SX_CNF_ATTN_MAX_IN,
               "sx_cnf_attn_flow: 1 + dim + latent_dim must be <= %d (x and latent share one tile)", SX_CNF_ATTN_MAX_IN);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "sx_cnf_attn_flow: activation %d has no in-kernel derivative", net.act);
    SX_REQUIRE(net.set_size >= 1 && net.set_size <= SX_CNF_ATTN_MAX_SIZE, "sx_cnf_attn_flow: set_size must be in 1..%d (got %d)",
               SX_CNF_ATTN_MAX_SIZE, net.set_size);
    SX_REQUIRE(net.n_hidden == 0 || (net.hidden[0] >= 1 && net.hidden[0] <= SX_CNF_ATTN_MAX_HIDDEN),
               "sx_cnf_attn_flow: the hidden layer must have 1..%d units (got %d)", SX_CNF_ATTN_MAX_HIDDEN, net.hidden[0]);
    SX_REQUIRE(net.embed >= 1 && net.embed <= SX_CNF_ATTN_MAX_EMBED, "sx_cnf_attn_flow: the embedding must have 1..%d features (got %d)",
               SX_CNF_ATTN_MAX_EMBED, net.embed);
    SX_REQUIRE((net.n_heads == 1 || net.n_heads == 2 || net.n_heads == 4) && net.embed % net.n_heads == 0,
               "sx_cnf_attn_flow: 1, 2 or 4 heads that divide the embedding (got %d heads, %d features)", net.n_heads, net.embed);
    return SX_OK;
}

}  // namespace

extern "C" size_t sx_cnf_attn_lds_bytes(const sx_cnf_attn_net *net_host) {
    if (ca_check_shape(net_host) != SX_OK) return 0;
    const size_t bytes = ca_plan(*net_host, nullptr) * 4;
    return bytes <= SX_CNF_LDS_BYTES ? bytes : 0;
}

extern "C" int sx_cnf_attn_flow(const sx_cnf_attn_net *net_host, const float *x, const float *latent, float *y, float *ldj, int64_t n_rows,
                                int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj, void *stream) {
    const int rc = ca_check_shape(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_attn_net &net = *net_host;
    for (int e = 0; e < 3; ++e) {
        SX_REQUIRE(net.W1[e] != nullptr && net.b1[e] != nullptr, "sx_cnf_attn_flow: embedding %d lacks its first weight or bias", e);
        SX_REQUIRE(net.n_hidden == 0 || (net.W2[e] != nullptr && net.b2[e] != nullptr), "sx_cnf_attn_flow: embedding %d lacks its second weight or bias", e);
    }
    SX_REQUIRE(net.P != nullptr && net.pb != nullptr, "sx_cnf_attn_flow: the projection's weight or bias is missing");
    const int rc_call = cnf_check_call("sx_cnf_attn_flow", solver, n_rows, net.set_size, n_steps, step_size, x, y);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "sx_cnf_attn_flow: latent rows missing");
    SX_REQUIRE(!want_ldj || ldj != nullptr, "sx_cnf_attn_flow: want_ldj needs ldj");
    ca_args a{};
    a.net = net;
    const size_t lds = ca_plan(net, &a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_attn_flow: the padded weights need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    a.scale = (float)sqrt(1.0 / (double)(net.embed / net.n_heads));
    a.x = x; a.latent = latent; a.y = y; a.ldj = ldj; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.want_ldj = want_ldj ? 1 : 0;
    a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    const int64_t want = cnf_set_blocks(n_rows, net.set_size);
    const char *fn = "sx_cnf_attn_flow";
    if (net.n_hidden == 0) return cnf_launch<cnf_attn_flow_kernel<1, 1>>(fn, a, lds, want, stream);
    return cnf_tiles(net.hidden[0]) == 1 ? cnf_launch<cnf_attn_flow_kernel<1, 2>>(fn, a, lds, want, stream)
                                         : cnf_launch<cnf_attn_flow_kernel<2, 2>>(fn, a, lds, want, stream);
}
