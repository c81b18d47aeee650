// Exact-trace continuous normalizing flow over SETS with attention (ContinuousTransform with divergence='exact' over
// net.DiffeqExactTraceAttention; reference: stribor/net/diffeq_exact_trace.py:104-130, diffeq_zero_trace.py:179-227, made.py, diagjac.py)
// on a fixed grid, in one launch.
//
// sx_cnf_exact_attn_flow -- rows are set elements, the N = set_size elements of a set contiguous.  With hidden_dims = [E] or [H1, E], H
// heads of width dh = E / H and scale = dh^-1/2, for element i and dimension d
//     q_i[d, :] = MADE_q(x_i)[d, :]                   E values (MADE column e D + d); does not depend on x_i[d]
//     k_j = K(x_j),  v_j = V(x_j)                     E values each (one Linear, or Linear - act - Linear); no time, no latent
//     per head:  s_ij = scale q_i[d] . k_j for j != i,  s_ii = -inf,   p_i = safe_softmax_j(s_ij),   o_i[d] = sum_j p_ij v_j
//     h_i[d, :] = P o_i[d] + b                        d_h values per dimension; no term depends on x_i[d]
//     f_i[d]    = g(t, x_i[d], h_i[d, :], latent_i)   the dimwise net g: one MLP shared by every dimension
//     jac_i[d]  = dg/dx at fixed h                    = df_i[d]/dx_i[d] exactly
// One half is sx_cnf_exact.hip's, and is the same code: the dimwise loop with its forward-mode tangent, the solve of a row group, the
// dimwise block of the image and the host checks come from sx_cnf_exact_common.h.  The other half is sx_cnf_attn.hip's (the set layout,
// the k / v exchange, the scores and P.V on the matrix pipe, the key mask, the flagged-set rule: sx_cnf_attn_common.h).  This file joins
// them: dim attentions per evaluation, each with its own masked query, against ONE set of keys and values.  There is no tangent
// attention: the trace is the dimwise net's tangent, and want_ldj == 0 drops only that.  The conventions hold: one wave = 32 rows on
// the MFMA column, exact fp32 (v_mfma_f32_32x32x2_f32), -ffp-contract=off, the same solvers, grid and tableau, state / stage vectors /
// h / log-det in registers for the whole grid.
//   * a workgroup of 4 waves owns 128 row slots and takes WHOLE sets per pass: sets never straddle workgroups, they may straddle
//     waves.  A set sits in a block of S slots, S the power of two that holds N, aligned to S -- 128 / S sets a pass, where
//     sx_cnf_attn.hip packs floor(128 / N): element j of a set then has one place relative to the MFMA's key pairs, the 8-key groups
//     and the tiles in EVERY block, the masked keys between add exact zeros, and so the sums over keys (softmax, P.V) run in one order:
//     a set's rows are bit-identical wherever the set stands in the batch.  The slots behind a set's N and past the last set are
//     padding: they compute on zeros, attend to themselves (every key masked: o = 0) and are never stored.  The pass loop, the stage
//     loop and N are uniform over the workgroup, so every wave reaches every barrier;
//   * per evaluation k and v are computed once and written (E floats each, row stride 36) to ONE exchange area in LDS, between two
//     workgroup barriers: the first closes the previous evaluation's reads, the second publishes the rows.  (Two alternating areas
//     would save the first barrier and cost 36 KiB more than the largest image leaves.)  N = 1 needs no exchange: o = 0, h = b;
//   * the query operand: the MADE's last layer puts dimension d's E values at positions (d % per) * slot .. + E - 1 of output tile
//     d / per, with slot = 8, 16 or 32 (the smallest that holds E) and per = 32 / slot dimensions a tile.  A tile is computed when its
//     first dimension comes up and serves its `per` dimensions; for a dimension at offset o the key rows are read o floats early, so
//     that the k-groups of the query tile meet the key features they belong to (o is a multiple of 8: every read stays inside the
//     row's 32 written floats).  A head contracts its own features only, as in sx_cnf_attn.hip;
//   * scores, softmax (max-subtracted, expf, one sweep for maximum and sum, a second for p) and P.V as in sx_cnf_attn.hip;
//   * the projection's rows sit at the slot positions kmap(kk >> 1, kk & 1): register c of lane half hh of its result is slot 2c + hh
//     -- the slot pair the dimwise loop reads from tile c --, and is copied to register d of that tile;
//   * non-finite values follow sx_cnf_attn.hip: a k / v value that is not finite is written as 0 and raises its set's flag (so does a
//     NaN hidden unit of K or V under ReLU); a flagged set is stored as NaN in every element, no other set of the workgroup sees it;
//   * the latent columns' share of the dimwise first layer: one GEMM per pass before the grid loop, A fragments from global memory.
//
// Coverage: 1 <= N <= 128, dim <= 8, hidden_dims [E] or [H1, E] with H1 <= 64 and E <= 32, slot(E) * dim <= 128 (at most four query
// tiles: E <= 8 and E <= 16 at any dim, wider at dim <= 4), 1, 2 or 4 heads dividing E, d_h <= 8, latent_dim <= 64, activations
// Identity .. LeakyReLU.  The largest image ([64, E], four query tiles, d_h any) is 26368 floats = 103 KiB; the exchange (two areas of
// 128 x 36 floats and 128 flags) 36.5 KiB: 139.5 KiB of the 160.  ([64, 32], dim 2: 86.75 KiB; [32, 16], dim 8: 50 KiB.)
#include "sx_cnf_exact_common.h"
#include "sx_cnf_attn_common.h"

#define SX_XA_EXCHANGE (2 * CA_AREA + SX_CNF_ROWS)      /* floats behind the image: the k area, the v area, the set flags */

namespace {

// the LDS image: float offsets (sx_cnf_exact_attn_net.image is laid out in this order; net/diffeq_exact_trace.py builds it); the
// exchange follows it.  QT, the query tiles, is a property of (E, dim), not of the instantiation: the plan is made at run time
struct xa_plan {
    int qw1, qb1;                 // the q MADE's hidden layer (two hidden layers in the dimwise net: NH == 2)
    int qwl, qbl;                 // its last layer [QT x KT tiles] and bias [32 QT]
    int ew1[2], eb1[2];           // K and V: the hidden layer (NH == 2)
    int ewl[2], ebl[2];           // ... the last layer [1 x KT tiles] and bias [32]
    int pw, pb;                   // the projection [1 x 1 tile] and bias [32]
    cnf_exact_dimwise dw;
    int total;                    // floats of the image = the offset of the exchange
};

// slots of a set's block: the power of two that holds N.  Blocks are aligned to their size, so element j of a set has ONE place relative
// to the 8-key groups, the lane halves and the tiles whatever the set's block: the sums over keys run in one order
__host__ __device__ inline int xa_stride(int N) { int s = 1; while (s < N) s *= 2; return s; }
__host__ __device__ inline int xa_slot(int E) { return E <= 8 ? 8 : E <= 16 ? 16 : 32; }
__host__ __device__ inline int xa_query_tiles(int E, int D) { const int per = 32 / xa_slot(E); return (D + per - 1) / per; }

__host__ __device__ inline xa_plan xa_make_plan(int HT, int NH, int QT) {
    xa_plan p{};
    int off = 0;
    const int KT = NH == 2 ? HT : 1;
    if (NH == 2) {
        p.qw1 = off; off += HT * 1024;
        p.qb1 = off; off += HT * 32;
    }
    p.qwl = off; off += QT * KT * 1024;
    p.qbl = off; off += QT * 32;
    for (int e = 0; e < 2; ++e) {
        if (NH == 2) {
            p.ew1[e] = off; off += HT * 1024;
            p.eb1[e] = off; off += HT * 32;
        }
        p.ewl[e] = off; off += KT * 1024;
        p.ebl[e] = off; off += 32;
    }
    p.pw = off; off += 1024;
    p.pb = off; off += 32;
    p.dw = cnf_exact_plan_dimwise(off, HT, NH);
    p.total = off;
    return p;
}

struct xa_args : cnf_exact_args<sx_cnf_exact_attn_net> {
    float scale;
};

// the input of a last layer: the state itself, or act(W1 x + b1); `nan_is_bad`: a NaN before a ReLU (fmaxf would turn it into 0
// where torch keeps it) counts as a NaN result
template <int HT, int NH>
__device__ __forceinline__ void xa_hidden(cnf_tile<(NH == 2 ? HT : 1)> &hid, const cnf_tile<1> &xi, int w1, int b1, int act, bool nan_is_bad,
                                          bool &bad, int lane) {
    if constexpr (NH == 2) {
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            hid.v[m] = f32x16{};
            cnf_mma<1>(hid.v[m], xi, cnf_smem + w1 + m * 1024 + lane * 4);
        }
        cnf_add_vec<HT>(hid, cnf_smem + b1 + 4 * (lane >> 5));
        if (nan_is_bad && act == SX_ACT_RELU) {
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) bad = bad || hid.v[m][r] != hid.v[m][r];
        }
        cnf_act_all<HT>(hid, act);
    } else {
        hid.v[0] = xi.v[0];
    }
}

// f(t, x) -> k (dimension i at register i of the lower lane half) and -- when `want` -- tr = sum_i jac_i, for the wave's 32 rows
template <int HT, int NH, int OT>
__device__ __forceinline__ void xa_eval(const xa_args &a, const xa_plan &p, const ca_pos &pos, const f32x16 &xin, float t, const cnf_tile<HT> &lat,
                                        f32x16 &kout, bool want, float &tr, int lane) {
    constexpr int KT = NH == 2 ? HT : 1;
    const int h = lane >> 5, act = a.net.act, D = a.net.dim, H = a.net.n_heads, E = a.net.hidden[NH - 1], dh = E / H, N = a.net.set_size;
    const int slot = xa_slot(E), per = 32 / slot;
    const float scale = a.scale;
    // the image never changes: without this the compiler hoists its loads out of the step loop and holds matrices in registers
    asm volatile("" ::: "memory");
    cnf_tile<1> xi;
    xi.v[0] = xin;
    const float *xk = cnf_smem + p.total, *xv = xk + CA_AREA;
    // ---- keys and values, once per evaluation ----
    if (N > 1) {
        f32x16 z[2];
        bool bad = false;                  // the row's k or v is not finite (or would not be in torch): its set is flagged
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            cnf_tile<KT> hid;
            xa_hidden<HT, NH>(hid, xi, p.ew1[e], p.eb1[e], act, true, bad, lane);
            f32x16 acc = {};
            cnf_mma<KT>(acc, hid, cnf_smem + p.ewl[e] + lane * 4);
            const float *bl = cnf_smem + p.ebl[e] + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[e][r] = acc[r] + cnf_vec(bl, 0, r);
        }
        __syncthreads();                   // the reads of the previous evaluation are over
        float *mk = cnf_smem + p.total + pos.rho * CA_LD + 4 * h, *mv = mk + CA_AREA;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            *reinterpret_cast<f32x4 *>(mk + 8 * g) = f32x4{ca_finite(z[0][4 * g], bad), ca_finite(z[0][4 * g + 1], bad),
                                                           ca_finite(z[0][4 * g + 2], bad), ca_finite(z[0][4 * g + 3], bad)};
            *reinterpret_cast<f32x4 *>(mv + 8 * g) = f32x4{ca_finite(z[1][4 * g], bad), ca_finite(z[1][4 * g + 1], bad),
                                                           ca_finite(z[1][4 * g + 2], bad), ca_finite(z[1][4 * g + 3], bad)};
        }
        if (bad) reinterpret_cast<int *>(cnf_smem + p.total + 2 * CA_AREA)[pos.first] = 1;
        __syncthreads();
    }
    // ---- the exclusive net: per dimension an attention of the MADE's query against those keys and values, projected to d_h slots ----
    cnf_tile<OT> raw;
#pragma unroll
    for (int m = 0; m < OT; ++m) raw.v[m] = f32x16{};
    cnf_tile<KT> qh;
    {
        bool unused = false;
        xa_hidden<HT, NH>(qh, xi, p.qw1, p.qb1, act, false, unused, lane);
    }
    const float *pbv = cnf_smem + p.pb + 4 * h;
#pragma nounroll
    for (int qt = 0; qt * per < D; ++qt) {
        asm volatile("" ::: "memory");
        f32x16 qv = {};
        cnf_mma<KT>(qv, qh, cnf_smem + p.qwl + qt * (KT * 1024) + lane * 4);
        {
            const float *qb = cnf_smem + p.qbl + 32 * qt + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) qv[r] = qv[r] + cnf_vec(qb, 0, r);
        }
#pragma nounroll
        for (int dd = 0; dd < per; ++dd) {
            const int d = qt * per + dd, o0 = dd * slot;
            if (d >= D) break;
            f32x16 o = {};
            if (N > 1) {
#pragma nounroll
                for (int hd = 0; hd < H; ++hd) {
                    asm volatile("" ::: "memory");
                    const int lo = o0 + hd * dh, hi = lo + dh;
                    const bool e_in = (lane & 31) >= hd * dh && (lane & 31) < hd * dh + dh;
                    f32x16 qm;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int f = sx_kmap(r, h);
                        qm[r] = (f >= lo && f < hi) ? qv[r] : 0.f;
                    }
                    float m = -INFINITY, l = 0.f;
#pragma nounroll
                    for (int kt = pos.kt_lo; kt <= pos.kt_hi; ++kt) {
                        f32x16 s = ca_scores(qm, xk + (32 * kt + (lane & 31)) * CA_LD + 4 * h - o0, lo, hi);
                        float tmax = -INFINITY;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            s[r] = ca_valid(pos, 32 * kt + sx_kmap(r, h), true) ? s[r] * scale : -INFINITY;
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
#pragma nounroll
                    for (int kt = pos.kt_lo; kt <= pos.kt_hi; ++kt) {
                        f32x16 s = ca_scores(qm, xk + (32 * kt + (lane & 31)) * CA_LD + 4 * h - o0, lo, hi);
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            s[r] = ca_valid(pos, 32 * kt + sx_kmap(r, h), true) ? expf(s[r] * scale - mu) * inv : 0.f;
                        ca_pv(o, s, xv + (32 * kt + 4 * h) * CA_LD + (lane & 31), e_in);
                    }
                }
            }
            cnf_tile<1> ot;
            ot.v[0] = o;
            f32x16 acc = {};
            cnf_mma<1>(acc, ot, cnf_smem + p.pw + lane * 4);
#pragma unroll
            for (int c = 0; c < OT; ++c) {
                const float hv = acc[c] + cnf_vec(pbv, 0, c);
#pragma unroll
                for (int r = 0; r < 16; ++r) raw.v[c][r] = (d == r) ? hv : raw.v[c][r];
            }
        }
    }
    // ---- the dimwise net, one dimension at a time ----
    cnf_exact_dimwise_eval<HT, NH, OT>(p.dw, act, D, xin, raw, t, lat, kout, want, tr, lane);
}

template <int HT, int NH, int OT>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_exact_attn_kernel(const xa_args a) {
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6, D = a.net.dim, L = a.net.latent_dim, N = a.net.set_size;
    const xa_plan pl = xa_make_plan(HT, NH, xa_query_tiles(a.net.hidden[NH - 1], D));
    cnf_stage_image(a.net.image, pl.total);
    __syncthreads();
    const bool want = a.want_ldj != 0;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int S = xa_stride(N), sets_per_pass = SX_CNF_ROWS / S;
    const int64_t n_sets = a.n_rows / N, n_passes = (n_sets + sets_per_pass - 1) / sets_per_pass;
    int *flags = reinterpret_cast<int *>(cnf_smem + pl.total + 2 * CA_AREA);
    ca_pos p;
    p.rho = wave * 32 + (lane & 31);
    const int set_in_pass = p.rho / S, j = p.rho - set_in_pass * S;          // the slot's block and its place in it
    // the key tiles of the wave's queries: its own (blocks of <= 32 slots never leave a tile), or the tiles of its block that hold rows
    p.kt_lo = S <= 32 ? wave : (32 * wave / S) * (S / 32);
    p.kt_hi = S <= 32 ? wave : p.kt_lo + ((N - 1) >> 5);
    // (every bound of this loop is uniform over the workgroup: all four waves make every pass and meet at every barrier)
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        const int64_t set0 = pass * sets_per_pass, left = n_sets - set0;
        const int sets_here = left < sets_per_pass ? (int)left : sets_per_pass;
        const bool live = j < N && set_in_pass < sets_here;
        const int64_t row = (set0 + set_in_pass) * N + j;
        p.first = live ? p.rho - j : p.rho;
        p.n = live ? N : 1;
        if (N > 1) {
            if (threadIdx.x < SX_CNF_ROWS) flags[threadIdx.x] = 0;
            __syncthreads();
        }
        CNF_EXACT_SOLVE_ROWS(HT, a, row, live, h, D, L, want, sgn, lane, xa_eval<HT, NH, OT>(a, pl, p, xs.v[0], ts, lat, k.v[0], want, q, lane))
        if (N > 1) {
            const bool poison = flags[p.first] != 0;
            __syncthreads();                // the flags are read: the next pass may clear them
            // a flagged set: NaN over what the solve stored (the same thread stored it)
            if (poison && live && h == 0) {
                const float nan = __builtin_nanf("");
                for (int r = 0; r < D; ++r) a.y[row * D + r] = nan;
                if (want) a.ldj[row] = nan;
            }
        }
    }
}

int xa_check_net(const sx_cnf_exact_attn_net *net_host) {
    const char *fn = "sx_cnf_exact_attn_flow";
    const int rc = cnf_exact_check_net(fn, net_host, SX_CNF_EXACT_ATTN_MAX_DIM, SX_CNF_EXACT_ATTN_MAX_DH, SX_CNF_EXACT_ATTN_MAX_LATENT,
                                       SX_CNF_EXACT_ATTN_MAX_HIDDEN);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_attn_net &net = *net_host;
    const int E = net.hidden[net.n_hidden - 1];
    SX_REQUIRE(E <= SX_CNF_EXACT_ATTN_MAX_EMBED, "%s: the last hidden width (the embedding) must be in 1..%d (got %d)", fn,
               SX_CNF_EXACT_ATTN_MAX_EMBED, E);
    SX_REQUIRE(xa_query_tiles(E, net.dim) <= 4, "%s: %d dimensions of %d-feature queries need more than four 32-feature tiles", fn, net.dim, E);
    SX_REQUIRE((net.n_heads == 1 || net.n_heads == 2 || net.n_heads == 4) && E % net.n_heads == 0,
               "%s: 1, 2 or 4 heads that divide the embedding (got %d heads, %d features)", fn, net.n_heads, E);
    SX_REQUIRE(net.set_size >= 1 && net.set_size <= SX_CNF_EXACT_ATTN_MAX_SIZE, "%s: set_size must be in 1..%d (got %d)", fn,
               SX_CNF_EXACT_ATTN_MAX_SIZE, net.set_size);
    return SX_OK;
}

// floats of the image, by the kernel's plan; the exchange follows them
inline size_t xa_image_floats(const sx_cnf_exact_attn_net &net) {
    int HT, OT;
    cnf_exact_shape(net, &HT, &OT);
    return (size_t)xa_make_plan(HT, net.n_hidden, xa_query_tiles(net.hidden[net.n_hidden - 1], net.dim)).total;
}

}  // namespace

extern "C" size_t sx_cnf_exact_attn_lds_bytes(const sx_cnf_exact_attn_net *net_host) {
    if (xa_check_net(net_host) != SX_OK) return 0;
    const size_t lds = (xa_image_floats(*net_host) + SX_XA_EXCHANGE) * 4;
    return lds <= SX_CNF_LDS_BYTES ? lds : 0;
}

#define XA_CASE(H_, N_, O_)                                                                                                        \
    if (HT == H_ && NH == N_ && OT == O_) return cnf_launch<cnf_exact_attn_kernel<H_, N_, O_>>(fn, a, lds, blocks, stream);

extern "C" int sx_cnf_exact_attn_flow(const sx_cnf_exact_attn_net *net_host, const float *x, const float *latent, float *y, float *ldj,
                                      int64_t n_rows, int32_t solver, int32_t n_steps, float t0, float t1, float step_size, int32_t want_ldj,
                                      void *stream) {
    const char *fn = "sx_cnf_exact_attn_flow";
    int rc = xa_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_exact_attn_net &net = *net_host;
    rc = cnf_check_call(fn, solver, n_rows, net.set_size, n_steps, step_size, x, y);
    if (rc != SX_OK) return rc;
    int HT, OT;
    cnf_exact_shape(net, &HT, &OT);
    const int NH = net.n_hidden;
    const size_t image = xa_image_floats(net), lds = (image + SX_XA_EXCHANGE) * 4;
    rc = cnf_exact_check_flow(fn, net, latent, ldj, want_ldj, image, lds, "the image and the exchange need");
    if (rc != SX_OK || n_rows == 0) return rc;
    xa_args a = cnf_exact_fill<xa_args>(net, x, latent, y, ldj, n_rows, solver, n_steps, t0, t1, step_size, want_ldj);
    a.scale = (float)sqrt(1.0 / (double)(net.hidden[NH - 1] / net.n_heads));
    const int64_t sets_per_pass = SX_CNF_ROWS / xa_stride(net.set_size), blocks = (n_rows / net.set_size + sets_per_pass - 1) / sets_per_pass;
    // (one hidden layer: the only hidden width is the embedding, <= 32 -- one tile)
    XA_CASE(1, 1, 1) XA_CASE(1, 1, 2) XA_CASE(1, 1, 4)
    XA_CASE(1, 2, 1) XA_CASE(1, 2, 2) XA_CASE(1, 2, 4)
    XA_CASE(2, 2, 1) XA_CASE(2, 2, 2) XA_CASE(2, 2, 4)
    sx_set_error("%s: no kernel for %d hidden x %d output tiles, %d hidden layers", fn, HT, OT, NH);
    return SX_E_BADARG;
}
