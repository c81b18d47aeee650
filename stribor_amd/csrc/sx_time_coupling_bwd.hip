// Backward of the time-conditioned affine coupling (ContinuousAffineCoupling, stribor/flows/coupling.py:98-213, with the time nets
// of stribor/net/time_net.py:6-47): sx_time_coupling_bwd.  DESIGN.md section 4.20.
//
// The layer, for one row (m: the 0/1 mask, live = 1 - m, sigma = ldj_scale):
//     z = [x (.) m (zeros when dim == 1), latent, t (concat_time)],   h = act(W1 z + b1),   (ls | sh) = W2 h + b2,
//     (ts | th) = time_net(t),   a = ls (.) ts,   c = sh (.) th,   ldj = sigma sum live (.) a
//     forward  y = live (.) (x e^a + c) + m (.) x          reverse  y = live (.) (x - c) e^-a + m (.) x
// Given gy = dloss/dy and gl = dloss/dldj (either may be absent: zeros):
//     forward  g_a = live (.) (gy x e^a + sigma gl),  g_c = live (.) gy,                 gx_dir = live (.) gy e^a + m (.) gy
//     reverse  g_a = live (.) (-gy (x - c) e^-a + sigma gl),  g_c = -live (.) gy e^-a,   gx_dir = live (.) gy e^-a + m (.) gy
//     e2 = (g_a ts | g_c th),   dW2 = sum_rows e2 h^T,   db2 = sum_rows e2,   e1 = act'(h) (.) (W2^T e2),
//     dW1 = sum_rows e1 z^T,   db1 = sum_rows e1,   g_z = W1^T e1,   gx = gx_dir + m (.) g_z[:dim],   glatent = g_z[dim : dim + L],
//     gt = g_z[dim + L] + sum_live (g_a ls dts/dt + g_c sh dth/dt),   dtime = sum_rows (g_a ls dts/ds | g_c sh dth/ds)
//   * the conventions of sx_cnf_common.h: a workgroup of 4 waves = 128 row slots, one wave = 32 rows on the MFMA column, features on
//     the C rows, exact fp32 (v_mfma_f32_32x32x2_f32), weights in LDS in A-fragment order, cnf_launch;
//   * PRUNED images, as the forward's planner prunes: only the columns of x with m = 1 (and the latent) reach the conditioner, so
//     W1's image holds those columns, packed (kin: packed input -> column of W1); only the live rows of W2 matter, so its image holds
//     the live log-scale rows, then the live shift rows, each padded to whole tiles (orow: packed output -> row of W2).  Register r
//     of log-scale tile j and of shift tile j then belong to the same column of x.  The transposed images are pruned the same way;
//   * the time column of W1 is a rank-1 per-row term (a vector in LDS), as sx_cnf.hip handles its time column: its gradient is the
//     row sum of e1 t, its share of gt a sum of e1 w over the features;
//   * a wave takes 32-row groups grid-stride (the pass loop); nothing is exchanged between waves, so there is no barrier in it.
//     h, ls, sh and a are recomputed from x, latent and t: the forward saves nothing;
//   * dW1, db1, dW2, db2 and dtime are contracted over the wave's 32 rows by sx_train_contract.h (both operands turn through two
//     per-wave LDS slots) into the wave's own partial -- the first group writes it, later groups add -- and tc_reduce_kernel sums
//     the partials in slot order, scattering the pruned rows and columns back to the parameter's own layout (zeros elsewhere).
//     No atomics, no zero-fill: the same inputs give the same bits.
// Launches: ONE, plus the ordered sum when a parameter gradient is wanted.
//
// Coverage (sx_time_coupling_bwd_lds_bytes): one hidden layer, dim <= 64, dim + latent_dim <= 64, hidden <= 64, the seven
// activations of sx_cnf_common.h, time kinds 0..3 of half-width dim or 1, any mask with a live column (dim == 1: the column is
// live), fp32 rows.  The largest plan (dim 64 under mask 'none': 20 tiles) takes 115.1 KiB of SX_CNF_LDS_BYTES.
#include "sx_cnf_common.h"
#include "sx_train_contract.h"

#define SX_TK_BWD_MAX_BLOCKS 512         /* partial slots = 4 waves x min(row blocks, this) */

namespace {

struct tk_args {
    sx_time_coupling_net net;
    uint64_t keep_in, live;              // columns of W1 (without the time column) that are staged; live columns of x
    int n_in, n_live;                    // their counts
    int base_w1, base_w2, base_w1t, base_w2t;      // LDS float offsets of the images
    int base_b1, base_wt, base_b2, base_ts, base_th, base_kin, base_orow, base_scr;
    int off_w1, off_w2, off_b1, off_wt, off_b2, off_dt, part_floats;       // float offsets inside a wave's partial
    int want_w1, want_b1, want_w2, want_b2, want_dt, any_param;
    const float *x, *latent, *t, *gy, *gl;
    float *gx, *glatent, *gt, *partial;
    int64_t n_rows;
    int reverse;
    float sigma;
};

// the i-th set bit of `bits` is bit ...: each thread finds the rank of its own bit
__device__ __forceinline__ int tk_rank(uint64_t bits, int i) { return __popcll(bits & ((1ull << i) - 1)); }

// an image through index maps: tile (m, c), float g*256 + lane*4 + j holds W[rmap[i]][cmap[k]] with (i, k) =
// (32m + (lane & 31), 32c + kmap(4g + j, lane >> 5)), or -- TR, the transposed image, tc_stage_t's order -- W[rmap[k']][cmap[i']] with
// (k', i') = (32c + kmap(4g + j, lane >> 5), 32m + (lane & 31)).  A NULL map is the identity below its bound; -1: a zero.
template <bool TR>
__device__ __forceinline__ void tk_stage(int base, const float *__restrict__ W, int ld, int MT, int KT, const int *rmap, int n_r,
                                         const int *cmap, int n_c) {
    const int n_w = MT * KT * 1024;
    for (int e = threadIdx.x; e < n_w; e += SX_CNF_THREADS) {
        const int tile = e >> 10, rem = e & 1023;
        const int g = rem >> 8, lane = (rem >> 2) & 63, j = rem & 3;
        const int m = tile / KT, c = tile - m * KT;
        const int on_lane = 32 * m + (lane & 31), on_k = 32 * c + sx_kmap(4 * g + j, lane >> 5);
        const int ri = TR ? on_k : on_lane, ci = TR ? on_lane : on_k;
        const int row = rmap != nullptr ? rmap[ri] : (ri < n_r ? ri : -1);
        const int col = cmap != nullptr ? cmap[ci] : (ci < n_c ? ci : -1);
        cnf_smem[base + e] = (row >= 0 && col >= 0) ? W[(int64_t)row * ld + col] : 0.f;
    }
}

// out[m] = (image . in)[m], m < MT, an output tile at a time (the reads of a tile stay beside its MFMAs)
template <int KT, int MT>
__device__ __forceinline__ void tk_gemm(const cnf_tile<KT> &in, cnf_tile<MT> &out, int base, int lane) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        SX_NO_HOIST();
        f32x16 acc = {};
        cnf_mma<KT>(acc, in, cnf_smem + base + m * KT * 1024 + lane * 4);
        out.v[m] = acc;
    }
}

// W += X Y^T and v += sum X over the wave's 32 rows, into the wave's partial (pw: MT x KT tiles, pv: MT x 64 floats)
template <int MT, int KT>
__device__ __forceinline__ void tk_contract(const cnf_tile<MT> &X, const cnf_tile<KT> &Y, float *pw, float *pv, bool want_w, bool want_v,
                                            bool first, float *sA, float *sB, int lane) {
    if (want_w) {
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            SX_NO_HOIST();
            tc_put(sB, Y.v[c], lane);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                SX_NO_HOIST();
                tc_put(sA, X.v[m], lane);
                tc_add_tile(pw + (m * KT + c) * 1024 + lane, sA, sB, first, lane);
            }
        }
    }
    if (want_v) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            SX_NO_HOIST();
            tc_put(sA, X.v[m], lane);
            tc_add_rowsum(pv + m * 64 + lane, sA, first, lane);
        }
    }
}

// the time net at (s, t): tau, dtau/ds, dtau/dt (stribor/net/time_net.py:6-47)
__device__ __forceinline__ void tk_time(int kind, float s, float t, float &tau, float &d_s, float &d_t) {
    if (kind == SX_TIME_LINEAR) {
        tau = s * t; d_s = t; d_t = s;
    } else if (kind == SX_TIME_TANH) {
        tau = tanhf(s * t);
        const float q = 1.f - tau * tau;
        d_s = q * t; d_t = s * q;
    } else if (kind == SX_TIME_LOG) {
        const float es = expf(s), den = es * t + 1.f;
        tau = logf(den); d_s = es * t / den; d_t = es / den;
    } else {
        tau = t; d_s = 0.f; d_t = 1.f;
    }
}

template <int KT, int HT, int LT>
__global__ __launch_bounds__(SX_CNF_THREADS) void time_coupling_bwd_kernel(const tk_args a) {
    const sx_time_coupling_net &net = a.net;
    const int D = net.dim, L = net.latent_dim, H = net.hidden, in1 = D + L + (net.concat_time ? 1 : 0);
    int *kin = reinterpret_cast<int *>(cnf_smem + a.base_kin), *orow = reinterpret_cast<int *>(cnf_smem + a.base_orow);
    // ---- the maps: packed conditioner input -> column of W1; packed output -> row of W2 (log-scale rows, then shift rows)
    for (int i = threadIdx.x; i < KT * 32; i += SX_CNF_THREADS) kin[i] = -1;
    for (int i = threadIdx.x; i < 2 * LT * 32; i += SX_CNF_THREADS) orow[i] = -1;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int i = threadIdx.x;
        if ((a.keep_in >> i) & 1) kin[tk_rank(a.keep_in, i)] = i;
        if ((a.live >> i) & 1) {
            const int j = tk_rank(a.live, i);
            orow[j] = i;
            orow[LT * 32 + j] = D + i;
        }
    }
    __syncthreads();
    tk_stage<false>(a.base_w1, net.W1, in1, HT, KT, nullptr, H, kin, 0);
    tk_stage<true>(a.base_w1t, net.W1, in1, KT, HT, nullptr, H, kin, 0);
    tk_stage<false>(a.base_w2, net.W2, H, 2 * LT, HT, orow, 0, nullptr, H);
    tk_stage<true>(a.base_w2t, net.W2, H, HT, 2 * LT, orow, 0, nullptr, H);
    cnf_stage_vec(net.b1, H, 1, HT * 32, a.base_b1);
    cnf_stage_vec(net.concat_time ? net.W1 + (D + L) : nullptr, H, in1, HT * 32, a.base_wt);
    for (int i = threadIdx.x; i < 2 * LT * 32; i += SX_CNF_THREADS) cnf_smem[a.base_b2 + i] = orow[i] >= 0 ? net.b2[orow[i]] : 0.f;
    for (int i = threadIdx.x; i < LT * 32; i += SX_CNF_THREADS) {
        const int col = orow[i], half = net.time_half;
        const bool has = col >= 0 && net.time_kind != SX_TIME_IDENTITY;
        cnf_smem[a.base_ts + i] = has ? net.time_scale[half == 1 ? 0 : col] : 0.f;
        cnf_smem[a.base_th + i] = has ? net.time_scale[half + (half == 1 ? 0 : col)] : 0.f;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, act = net.act, kind = net.time_kind;
    float *sA = cnf_smem + a.base_scr + wave * 2 * SX_TC_SLOT, *sB = sA + SX_TC_SLOT;
    const int64_t slot = (int64_t)blockIdx.x * SX_CNF_WAVES + wave;
    float *part = a.partial + slot * a.part_floats;            // only dereferenced when a parameter gradient is wanted
    const int *kin_h = kin + 4 * h, *lcol_h = orow + 4 * h;
    const bool params = a.any_param != 0;
    bool first = true;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = slot; grp < n_groups; grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        const float t = live ? a.t[row] : 0.f;
        const float sgl = (live && a.gl != nullptr) ? a.sigma * a.gl[row] : 0.f;
        const float *xr = tc_here(a.x + row * D), *gyr = tc_here(a.gy + row * D), *lr = tc_here(a.latent + row * L);
        // ---- the conditioner's packed input: the columns of x with m = 1, then the latent
        cnf_tile<KT> z;
#pragma unroll
        for (int c = 0; c < KT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = kin_h[32 * c + 8 * (r >> 2) + (r & 3)];
                z.v[c][r] = (!live || col < 0) ? 0.f : col < D ? xr[col] : lr[col - D];
            }
        // ---- the forward again: h, (ls | sh)
        cnf_tile<HT> hid;
        tk_gemm<KT, HT>(z, hid, a.base_w1, lane);
        {
            const float *vb = cnf_smem + a.base_b1 + 4 * h, *vt = cnf_smem + a.base_wt + 4 * h;
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) hid.v[m][r] = cnf_act((hid.v[m][r] + cnf_vec(vb, m, r)) + cnf_vec(vt, m, r) * t, act);
        }
        cnf_tile<2 * LT> e2;                                     // (ls | sh), then in place (g_ls | g_sh)
        tk_gemm<HT, 2 * LT>(hid, e2, a.base_w2, lane);
        cnf_add_vec<2 * LT>(e2, cnf_smem + a.base_b2 + 4 * h);
        // ---- the affine map's backward on the live columns; the time net's parameter gradient is summed tile by tile
        float gt = 0.f;
#pragma unroll
        for (int j = 0; j < LT; ++j) {
            SX_NO_HOIST();
            f32x16 dts, dth;
            const float *vs = cnf_smem + a.base_ts + 4 * h, *vh = cnf_smem + a.base_th + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = lcol_h[32 * j + 8 * (r >> 2) + (r & 3)];
                const bool ok = live && col >= 0;
                const float xv = ok ? xr[col] : 0.f, gv = (ok && a.gy != nullptr) ? gyr[col] : 0.f;
                float ts, ts_s, ts_t, th, th_s, th_t;
                tk_time(kind, cnf_vec(vs, j, r), t, ts, ts_s, ts_t);
                tk_time(kind, cnf_vec(vh, j, r), t, th, th_s, th_t);
                const float ls = e2.v[j][r], sh = e2.v[LT + j][r], av = ls * ts;
                float g_a, g_c, gxv;
                if (a.reverse) {
                    const float E = expf(-av);
                    gxv = gv * E;
                    g_a = -(gxv * (xv - sh * th)) + sgl;
                    g_c = -gxv;
                } else {
                    const float E = expf(av);
                    gxv = gv * E;
                    g_a = gxv * xv + sgl;
                    g_c = gv;
                }
                if (!ok) { g_a = 0.f; g_c = 0.f; }
                const float g_ts = g_a * ls, g_th = g_c * sh;
                e2.v[j][r] = g_a * ts;
                e2.v[LT + j][r] = g_c * th;
                gt += g_ts * ts_t + g_th * th_t;
                dts[r] = g_ts * ts_s;
                dth[r] = g_th * th_s;
                if (ok && a.gx != nullptr) a.gx[row * D + col] = gxv;
            }
            if (a.want_dt) {
                tc_put(sA, dts, lane);
                tc_add_rowsum(part + a.off_dt + j * 64 + lane, sA, first, lane);
                tc_put(sA, dth, lane);
                tc_add_rowsum(part + a.off_dt + (LT + j) * 64 + lane, sA, first, lane);
            }
        }
        // ---- dW2, db2; e1 = act'(h) (.) (W2^T e2)
        if (a.want_w2 || a.want_b2)
            tk_contract<2 * LT, HT>(e2, hid, part + a.off_w2, part + a.off_b2, a.want_w2 != 0, a.want_b2 != 0, first, sA, sB, lane);
        cnf_tile<HT> e1;
        tk_gemm<2 * LT, HT>(e2, e1, a.base_w2t, lane);
#pragma unroll
        for (int m = 0; m < HT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) e1.v[m][r] = cnf_dact(hid.v[m][r], act) * e1.v[m][r];
        // ---- the time column of W1: its share of gt, and its gradient (the row sum of e1 t)
        if (net.concat_time) {
            const float *vt = cnf_smem + a.base_wt + 4 * h;
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) gt += e1.v[m][r] * cnf_vec(vt, m, r);
            if (a.want_w1) {
#pragma unroll
                for (int m = 0; m < HT; ++m) {
                    SX_NO_HOIST();
                    f32x16 et;
#pragma unroll
                    for (int r = 0; r < 16; ++r) et[r] = e1.v[m][r] * t;
                    tc_put(sA, et, lane);
                    tc_add_rowsum(part + a.off_wt + m * 64 + lane, sA, first, lane);
                }
            }
        }
        if (a.gt != nullptr) {
            const float other = __shfl_xor(gt, 32, 64);          // the two lane halves hold the two halves of every tile's features
            if (live && h == 0) a.gt[row] = gt + other;
        }
        // ---- dW1, db1; g_z = W1^T e1
        if (a.want_w1 || a.want_b1)
            tk_contract<HT, KT>(e1, z, part + a.off_w1, part + a.off_b1, a.want_w1 != 0, a.want_b1 != 0, first, sA, sB, lane);
        if (a.gx != nullptr || a.glatent != nullptr) {
            cnf_tile<KT> gz;
            tk_gemm<HT, KT>(e1, gz, a.base_w1t, lane);
            if (live) {
#pragma unroll
                for (int c = 0; c < KT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int col = kin_h[32 * c + 8 * (r >> 2) + (r & 3)];
                        if (col < 0) continue;
                        if (col < D) {
                            if (a.gx != nullptr) a.gx[row * D + col] = (a.gy != nullptr ? gyr[col] : 0.f) + gz.v[c][r];
                        } else if (a.glatent != nullptr) {
                            a.glatent[row * L + (col - D)] = gz.v[c][r];
                        }
                    }
            }
        }
        if (params) first = false;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline int tk_popc(uint64_t v) { return __builtin_popcountll(v); }
inline uint64_t tk_low(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// is this layer inside the coverage?  (the integer fields only: no pointer is looked at)
bool tk_covered(const sx_time_coupling_net *net) {
    if (!net) return false;
    if (net->dim < 1 || net->dim > SX_TIME_COUPLING_BWD_MAX_DIM || net->latent_dim < 0) return false;
    if (net->dim + net->latent_dim > SX_TIME_COUPLING_BWD_MAX_IN) return false;
    if (net->hidden < 1 || net->hidden > SX_TIME_COUPLING_BWD_MAX_HIDDEN) return false;
    if (net->act < SX_ACT_IDENTITY || net->act > SX_ACT_LEAKYRELU) return false;
    if (net->time_kind < SX_TIME_IDENTITY || net->time_kind > SX_TIME_LOG) return false;
    if (net->time_half != 1 && net->time_half != net->dim) return false;
    if (net->concat_time != 0 && net->concat_time != 1) return false;
    const uint64_t m = ((uint64_t)net->mask[1] << 32 | net->mask[0]);
    if (m & ~tk_low(net->dim)) return false;                  // a mask bit beyond dim
    return (m & tk_low(net->dim)) != tk_low(net->dim);        // a live column (dim == 1: the one column)
}

// the pruning, the LDS plan (floats) and the layout of a wave's partial
size_t tk_plan(const sx_time_coupling_net &net, tk_args &a, int &KT, int &HT, int &LT) {
    const int D = net.dim, L = net.latent_dim;
    const uint64_t m = ((uint64_t)net.mask[1] << 32 | net.mask[0]) & tk_low(D);
    a.live = ~m & tk_low(D);
    a.keep_in = (D == 1 ? 0 : m) | (L > 0 ? tk_low(L) << D : 0);           // coupling.py:148-149: dim 1 conditions on zeros
    a.n_in = tk_popc(a.keep_in);
    a.n_live = tk_popc(a.live);
    KT = cnf_tiles(a.n_in);
    HT = cnf_tiles(net.hidden);
    LT = cnf_tiles(a.n_live);
    size_t off = 0;
    a.base_w1 = (int)off; off += (size_t)HT * KT * 1024;
    a.base_w1t = (int)off; off += (size_t)HT * KT * 1024;
    a.base_w2 = (int)off; off += (size_t)2 * LT * HT * 1024;
    a.base_w2t = (int)off; off += (size_t)2 * LT * HT * 1024;
    a.base_b1 = (int)off; off += (size_t)HT * 32;
    a.base_wt = (int)off; off += (size_t)HT * 32;
    a.base_b2 = (int)off; off += (size_t)2 * LT * 32;
    a.base_ts = (int)off; off += (size_t)LT * 32;
    a.base_th = (int)off; off += (size_t)LT * 32;
    a.base_kin = (int)off; off += (size_t)KT * 32;
    a.base_orow = (int)off; off += (size_t)2 * LT * 32;
    a.base_scr = (int)off; off += (size_t)SX_CNF_WAVES * 2 * SX_TC_SLOT;
    int poff = 0;
    a.off_w1 = poff; poff += HT * KT * 1024;
    a.off_w2 = poff; poff += 2 * LT * HT * 1024;
    a.off_b1 = poff; poff += HT * 64;
    a.off_wt = poff; poff += HT * 64;
    a.off_b2 = poff; poff += 2 * LT * 64;
    a.off_dt = poff; poff += 2 * LT * 64;
    a.part_floats = poff;
    return off;
}

int64_t tk_blocks(int64_t n_rows) {
    const int64_t want = cnf_row_blocks(n_rows);
    return want < SX_TK_BWD_MAX_BLOCKS ? want : SX_TK_BWD_MAX_BLOCKS;
}

}  // namespace

extern "C" size_t sx_time_coupling_bwd_lds_bytes(const sx_time_coupling_net *net_host) {
    if (!tk_covered(net_host)) return 0;
    tk_args a{};
    int KT, HT, LT;
    const size_t bytes = tk_plan(*net_host, a, KT, HT, LT) * 4;
    return bytes <= SX_CNF_LDS_BYTES ? bytes : 0;
}

extern "C" size_t sx_time_coupling_bwd_partial_floats(const sx_time_coupling_net *net_host, int64_t n_rows) {
    if (!tk_covered(net_host) || n_rows <= 0) return 0;
    tk_args a{};
    int KT, HT, LT;
    tk_plan(*net_host, a, KT, HT, LT);
    return (size_t)tk_blocks(n_rows) * SX_CNF_WAVES * (size_t)a.part_floats;
}

extern "C" int sx_time_coupling_bwd(const sx_time_coupling_net *net_host, const float *x, const float *latent, const float *t,
                                    const float *gy, const float *gl, float *gx, float *glatent, float *gt, float *partial,
                                    const sx_time_coupling_grads *grads, int64_t n_rows, int32_t reverse, float ldj_scale, void *stream) {
    const char *fn = "sx_time_coupling_bwd";
    SX_REQUIRE(net_host != nullptr, "%s: null layer", fn);
    const sx_time_coupling_net &net = *net_host;
    SX_REQUIRE(net.dim >= 1 && net.dim <= SX_TIME_COUPLING_BWD_MAX_DIM && net.latent_dim >= 0 &&
               net.dim + net.latent_dim <= SX_TIME_COUPLING_BWD_MAX_IN,
               "%s: dim must be in 1..%d and dim + latent_dim at most %d (got %d, %d)", fn, SX_TIME_COUPLING_BWD_MAX_DIM,
               SX_TIME_COUPLING_BWD_MAX_IN, net.dim, net.latent_dim);
    SX_REQUIRE(net.hidden >= 1 && net.hidden <= SX_TIME_COUPLING_BWD_MAX_HIDDEN, "%s: hidden must be in 1..%d (got %d)", fn,
               SX_TIME_COUPLING_BWD_MAX_HIDDEN, net.hidden);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "%s: the activation code must be in 0..%d (got %d)", fn,
               SX_ACT_LEAKYRELU, net.act);
    SX_REQUIRE(net.time_kind >= SX_TIME_IDENTITY && net.time_kind <= SX_TIME_LOG, "%s: the time kind must be in 0..%d (got %d)", fn,
               SX_TIME_LOG, net.time_kind);
    SX_REQUIRE(net.time_half == 1 || net.time_half == net.dim, "%s: the time net's half-width must be 1 or dim (got %d)", fn, net.time_half);
    SX_REQUIRE(tk_covered(net_host), "%s: concat_time must be 0 or 1, and the mask must lie within dim and leave a live column", fn);
    SX_REQUIRE(n_rows >= 0, "%s: negative n_rows", fn);
    SX_REQUIRE(reverse == 0 || reverse == 1, "%s: reverse must be 0 or 1 (got %d)", fn, reverse);
    SX_REQUIRE(net.W1 != nullptr && net.b1 != nullptr && net.W2 != nullptr && net.b2 != nullptr, "%s: the conditioner lacks a weight or a bias", fn);
    SX_REQUIRE(net.time_kind == SX_TIME_IDENTITY || net.time_scale != nullptr, "%s: time kind %d needs its scale", fn, net.time_kind);
    SX_REQUIRE(sx_aligned4(net.W1) && sx_aligned4(net.b1) && sx_aligned4(net.W2) && sx_aligned4(net.b2) && sx_aligned4(net.time_scale),
               "%s: a parameter is not 4-byte aligned", fn);
    SX_REQUIRE(x != nullptr && t != nullptr, "%s: null x / t", fn);
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "%s: latent_dim is %d and latent is null", fn, net.latent_dim);
    SX_REQUIRE(gy != nullptr || gl != nullptr, "%s: neither gy nor gl is given", fn);
    SX_REQUIRE(sx_aligned4(x) && sx_aligned4(latent) && sx_aligned4(t) && sx_aligned4(gy) && sx_aligned4(gl) && sx_aligned4(gx) &&
               sx_aligned4(glatent) && sx_aligned4(gt) && sx_aligned4(partial), "%s: every pointer must be 4-byte aligned", fn);
    SX_REQUIRE(glatent == nullptr || net.latent_dim > 0, "%s: glatent is given and latent_dim is 0", fn);
    float *g[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (grads != nullptr) { g[0] = grads->dW1; g[1] = grads->db1; g[2] = grads->dW2; g[3] = grads->db2; g[4] = grads->dtime; }
    bool any = false;
    for (int k = 0; k < 5; ++k) {
        SX_REQUIRE(sx_aligned4(g[k]), "%s: gradient %d is not 4-byte aligned", fn, k);
        any = any || g[k] != nullptr;
    }
    SX_REQUIRE(g[4] == nullptr || net.time_kind != SX_TIME_IDENTITY, "%s: dtime is given and the time net has no parameter", fn);
    SX_REQUIRE(any || gx != nullptr || glatent != nullptr || gt != nullptr, "%s: nothing to compute (no output and no parameter gradient)", fn);
    SX_REQUIRE(!any || n_rows == 0 || partial != nullptr, "%s: the partial buffer is missing (sx_time_coupling_bwd_partial_floats)", fn);
    tk_args a{};
    a.net = net;
    int KT, HT, LT;
    const size_t lds = tk_plan(net, a, KT, HT, LT) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "%s: the images and the slots need %zu bytes of LDS (budget %d)", fn, lds, SX_CNF_LDS_BYTES);
    a.want_w1 = g[0] != nullptr; a.want_b1 = g[1] != nullptr; a.want_w2 = g[2] != nullptr; a.want_b2 = g[3] != nullptr;
    a.want_dt = g[4] != nullptr; a.any_param = any ? 1 : 0;
    int grid = 0;
    if (n_rows > 0) {
        a.x = x; a.latent = latent; a.t = t; a.gy = gy; a.gl = gl; a.gx = gx; a.glatent = glatent; a.gt = gt; a.partial = partial;
        a.n_rows = n_rows; a.reverse = reverse; a.sigma = ldj_scale;
        const int64_t blocks = tk_blocks(n_rows);
        int rc = SX_E_UNSUPPORTED;
#define TK_CASE(K_, H_, L_) if (KT == K_ && HT == H_ && LT == L_) rc = cnf_launch<time_coupling_bwd_kernel<K_, H_, L_>>(fn, a, lds, blocks, stream, &grid);
        // (packed inputs + live columns = dim + latent_dim <= 64: never two tiles of both)
        TK_CASE(1, 1, 1) TK_CASE(1, 1, 2) TK_CASE(1, 2, 1) TK_CASE(1, 2, 2) TK_CASE(2, 1, 1) TK_CASE(2, 2, 1)
#undef TK_CASE
        if (rc == SX_E_UNSUPPORTED) sx_set_error("%s: no kernel for %d / %d / %d tiles", fn, KT, HT, LT);
        if (rc != SX_OK) return rc;
    }
    if (!any) return SX_OK;
    // dW1 [hidden, in1]: the staged columns, and the time column from its own vector; dW2 [2 dim, hidden]: the live log-scale rows,
    // then the live shift rows; db2 and dtime [2 dim] likewise.  Rows and columns that pruning skipped are written as zeros.
    const int D = net.dim, L = net.latent_dim, H = net.hidden, in1 = D + L + (net.concat_time ? 1 : 0);
    tc_reduce_args<9> r{};
    const int PR = SX_TC_PRUNE_ROWS, PC = SX_TC_PRUNE_COLS;
    r.e[0] = {g[0], H, D + L, KT, a.off_w1, in1, PC, 0, a.keep_in};
    r.e[1] = {(net.concat_time && g[0]) ? g[0] + D + L : nullptr, net.concat_time ? H : 0, 0, 0, a.off_wt, in1, 0, 0, 0};
    r.e[2] = {g[1], H, 0, 0, a.off_b1, 0, 0, 0, 0};
    r.e[3] = {g[2], D, H, HT, a.off_w2, 0, PR, a.live, 0};
    r.e[4] = {g[2] ? g[2] + (size_t)D * H : nullptr, D, H, HT, a.off_w2 + LT * HT * 1024, 0, PR, a.live, 0};
    r.e[5] = {g[3], D, 0, 0, a.off_b2, 0, PR, a.live, 0};
    r.e[6] = {g[3] ? g[3] + D : nullptr, D, 0, 0, a.off_b2 + LT * 64, 0, PR, a.live, 0};
    r.e[7] = {g[4], D, 0, 0, a.off_dt, 0, PR, a.live, 0};
    r.e[8] = {g[4] ? g[4] + D : nullptr, D, 0, 0, a.off_dt + LT * 64, 0, PR, a.live, 0};
    int total = 0;
    for (int k = 0; k < 9; ++k) total += r.e[k].cols ? r.e[k].rows * r.e[k].cols : r.e[k].rows;
    // every wave with a row group wrote its slot: slots 0 .. min(groups, 4 * grid) - 1 (no rows: no slots, the gradients are zero)
    const int64_t n_groups = (n_rows + 31) / 32, n_waves = (int64_t)grid * SX_CNF_WAVES;
    r.partial = partial; r.part_floats = a.part_floats; r.n_slots = (int)(n_groups < n_waves ? n_groups : n_waves);
    return tc_reduce(fn, r, total, stream);
}
