// Training of the dense DiffeqMLP CNF (ContinuousTransform with divergence='approximate' in training mode) on the fixed grid.
//
// sx_cnf_train_fwd -- the solve of sx_cnf_flow (same layout, images, grid, tableau and x arithmetic: y is bit-identical) with the
// Hutchinson estimate q = e^T (df/dx) e in place of the exact trace, e a fixed noise row; on request the state at the start of every
// step goes to a checkpoint buffer [n_steps, n, dim].
// sx_cnf_train_bwd -- the discrete adjoint of that solve: the grid walked backwards, per step the stage inputs z_i recomputed from
// the checkpoint (kept in per-wave LDS, one state tile each), the stages swept in reverse order, the hidden layers re-evaluated at
// z_i.  One evaluation at (t, z), given kb (the adjoint of k) and qb (of q), with d = act', s = act'' from the activation's output,
// u1 = W1x e, v = W_last^T e (both constant along a row's solve):
//   one hidden layer   q = sum d1 u1 v;   a1b = (W2^T kb) d1 + qb s1 u1 v;   zb = W1x^T a1b
//                      dW2 += kb h1^T + e (qb d1 u1)^T;   dW1x += a1b z^T + (qb d1 v) e^T
//   two hidden layers  w = d1 u1, r = W2 w, q = sum v d2 r;   rb = qb v d2;   a2b = (W3^T kb) d2 + qb s2 v r;   wb = W2^T rb
//                      a1b = (W2^T a2b) d1 + wb s1 u1;   zb = W1x^T a1b
//                      dW3 += kb h2^T + e (qb d2 r)^T;   dW2 += a2b h1^T + rb w^T;   dW1x += a1b z^T + (wb d1) e^T
// (the e terms are the u1 / v adjoints contracted with e at once: no per-row accumulator is kept for them).  Products with W^T use
// transposed A-fragment images staged beside the forward ones.  Weight gradients contract over the 32 rows of a wave with the same
// MFMA: both operands need the rows on the K index, so the two tiles turn through per-wave LDS scratch (feature-major, stride 33),
// where a bias gradient is a row sum of the same scratch.  The accumulators stay in registers across a wave's whole pass loop and
// are written once, as one partial per wave; the latent columns of dW1 (contracted once per row group from sum a1b) are added into
// the wave's own partial in global memory.  cnf_train_reduce_kernel sums the partials in slot order: no atomics anywhere, so two
// calls on the same inputs give the same bits.
//
// Everything the solve has in common with sx_cnf_flow -- the staging of the forward images, the row load / store, the latent GEMM,
// the hidden layers, the output layer, the network validator and the plan of the forward images -- is sx_cnf_dense.h's, used here
// with one state tile and one hidden tile.  The contraction slots (tc_put / tc_outer / tc_rowsum), the transposed stager and the
// layout of an accumulator tile (tc_tile_off) are sx_train_contract.h's, shared with sx_resnet_bwd.hip and sx_equivariant.hip.  Every
// row sum here is followed by a tc_put to the OTHER slot and then tc_outer's opening fence, so tc_rowsum's missing closing fence is
// not needed (the header's fence rule).  This file's own are the estimate, the adjoint sweep and the fp32 sum of the partials, whose
// dW_1 is assembled from three places and does not fit the shared table.
//
// Coverage: dim <= 32, 1 + dim + latent_dim <= 64, one or two hidden layers of <= 32 units (one tile: the adjoint sweep of a
// two-tile hidden layer does not build without scratch, so every hidden quantity below is ONE tile), the seven activations of
// sx_cnf_flow.
#include "sx_cnf_dense.h"
#include "sx_train_contract.h"

#define SX_CNF_TRAIN_MAX_BLOCKS 512      /* partial slots = 4 waves x min(row blocks, this) */
#if SX_CNF_TRAIN_MAX_HIDDEN != 32 || SX_CNF_TRAIN_MAX_DIM != 32 || SX_CNF_TRAIN_MAX_IN != 64
#error "the kernels below are built for one hidden tile, one state tile and two latent tiles"
#endif

namespace {

typedef cnf_tile<1> ct_tile;             /* a state or a hidden layer: one tile either way */

struct ct_args : cnf_dense_args {
    int base_t[3];                           // LDS float offsets of the transposed images W1x^T, W2^T (two hidden layers), W_last^T
    int base_scr, scr_stride;                // ... of wave 0's scratch, floats per wave
    int off_w2, off_wl, off_lat, off_vec;    // float offsets inside a wave's partial (dW1x at 0)
    int part_floats, n_virtual;
    const float *x, *latent, *e, *ckpt_in, *gy, *gldj;
    float *y, *ldj, *ckpt, *gx, *glat, *partial;
    int64_t n_rows;
    int solver, n_steps;
    float t0, t1, step_size;
};

// d = act'(v) of a whole tile from a = act(v): one wave-uniform switch around the sweep, not one per element (sx_cnf_common.h's
// cnf_dact_tile switches per element: other code here, see cnf_dense_act for the same choice)
__device__ __forceinline__ void ct_dact_tile(const f32x16 &a, f32x16 &d, int act) {
    switch (act) {
        case SX_ACT_TANH:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 1.f - a[r] * a[r];
            break;
        case SX_ACT_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = a[r] > 0.f ? 1.f : 0.f;
            break;
        case SX_ACT_SIGMOID:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = a[r] * (1.f - a[r]);
            break;
        case SX_ACT_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = a[r] > 0.f ? 1.f : a[r] + 1.f;
            break;
        case SX_ACT_SOFTPLUS:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 1.f - expf(-a[r]);          // sigmoid(v) = 1 - exp(-softplus(v))
            break;
        case SX_ACT_LEAKYRELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = a[r] > 0.f ? 1.f : 0.01f;
            break;
        default:
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 1.f;
    }
}

// s = act''(v) of a whole tile from a = act(v) and d = act'(v)
__device__ __forceinline__ void ct_d2act_tile(const f32x16 &a, const f32x16 &d, f32x16 &s, int act) {
    switch (act) {
        case SX_ACT_TANH:
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = -2.f * a[r] * d[r];
            break;
        case SX_ACT_SIGMOID:
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = d[r] * (1.f - 2.f * a[r]);
            break;
        case SX_ACT_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = a[r] > 0.f ? 0.f : a[r] + 1.f;
            break;
        case SX_ACT_SOFTPLUS:
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = d[r] * (1.f - d[r]);
            break;
        default:
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
    }
}

template <int NH>
__device__ __forceinline__ void ct_stage_all(const ct_args &a, bool backward) {
    const sx_cnf_net &net = a.net;
    const int D = net.dim, in_dim = 1 + D + net.latent_dim, H1 = net.layer[0].out_dim, Hl = net.layer[NH - 1].out_dim;
    cnf_dense_stage<1, 1, NH>(a);
    tc_stage_t(cnf_smem + a.base_t[NH], net.layer[NH].W, D, Hl, Hl, 0, 1, 1, SX_CNF_THREADS);
    if (backward) {
        tc_stage_t(cnf_smem + a.base_t[0], net.layer[0].W, H1, D, in_dim, 1, 1, 1, SX_CNF_THREADS);
        if (NH == 2) tc_stage_t(cnf_smem + a.base_t[1], net.layer[1].W, Hl, H1, H1, 0, 1, 1, SX_CNF_THREADS);
    }
}

// the Hutchinson estimate e^T J e of a row from the hidden activations
template <int NH>
__device__ __forceinline__ float ct_estimate(const ct_args &a, const ct_tile &h1, const ct_tile &h2, const ct_tile &u1, const ct_tile &v, int lane) {
    const int act = a.net.act;
    float s = 0.f;
    if (NH == 1) {
        f32x16 d1;
        ct_dact_tile(h1.v[0], d1, act);
#pragma unroll
        for (int r = 0; r < 16; ++r) s += (d1[r] * u1.v[0][r]) * v.v[0][r];
    } else {
        ct_tile w, rr;
        ct_dact_tile(h1.v[0], w.v[0], act);
#pragma unroll
        for (int r = 0; r < 16; ++r) w.v[0][r] = w.v[0][r] * u1.v[0][r];
        SX_NO_HOIST();
        cnf_gemm<1, 1>(w, rr, cnf_smem + a.base_w[1] + lane * 4);
        f32x16 d2;
        ct_dact_tile(h2.v[0], d2, act);
#pragma unroll
        for (int r = 0; r < 16; ++r) s += (v.v[0][r] * d2[r]) * rr.v[0][r];
    }
    return s + __shfl_xor(s, 32, 64);          // the two lane halves hold the two feature halves of a row
}

// the per-row constants of a solve: u1 = W1x e, v = W_last^T e
template <int NH>
__device__ __forceinline__ void ct_row_constants(const ct_args &a, const ct_tile &e, ct_tile &u1, ct_tile &v, int lane) {
    SX_NO_HOIST();
    cnf_gemm<1, 1>(e, u1, cnf_smem + a.base_w[0] + lane * 4);
    cnf_gemm<1, 1>(e, v, cnf_smem + a.base_t[NH] + lane * 4);
}

template <int NH>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_train_fwd_kernel(const ct_args a) {
    ct_stage_all<NH>(a, false);
    __syncthreads();
    const int D = a.net.dim;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_CNF_WAVES + (threadIdx.x >> 6); grp < n_groups;
         grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        ct_tile y, e, lat, u1, v;
        cnf_load_row<1>(y, a.x, row, D, live, h);
        cnf_load_row<1>(e, a.e, row, D, live, h);
        cnf_dense_latent<1>(a, lat, a.latent, row, live, lane);
        ct_row_constants<NH>(a, e, u1, v, lane);
        float l = 0.f;
        const int n_stages = cnf_stages(a.solver);
        const float third = 1.f / 3.f, two_thirds = 2.f / 3.f;
        for (int i = 0; i < a.n_steps; ++i) {
            float ta, tb;
            cnf_grid(a, sgn, i, ta, tb);
            const float dt = tb - ta, half = 0.5f * dt;
            if (a.ckpt != nullptr) cnf_store_row<1>(a.ckpt + (int64_t)i * a.n_rows * D, y, row, D, live, h);
            ct_tile k1, k2, xs = y;
            float q1 = 0.f, q2 = 0.f, ts = ta;
            for (int st = 0; st < n_stages; ++st) {
                ct_tile k, h1, h2;
                cnf_dense_hidden<1, 1, NH, true>(a, xs, ts, lat, h1, h2, lane);
                const float q = ct_estimate<NH>(a, h1, h2, u1, v, lane);
                cnf_dense_out<1, 1, NH>(a, NH == 1 ? h1 : h2, k, lane);
                cnf_tableau<1>(a.solver, st, ta, tb, dt, half, third, two_thirds, k, q, k1, k2, q1, q2, xs, ts, y, l);
            }
        }
        cnf_store_row<1>(a.y, y, row, D, live, h);
        if (live && h == 0) a.ldj[row] = l;
    }
}

// ---- the backward ---------------------------------------------------------------------------------------------------------------
// The backward moves rows between global memory and its tiles through the wave's LDS: a coalesced copy of the group's contiguous
// block (rows row0 .. row0 + n_live - 1 of a row-major [n, ld] array, ld <= 62: at most 2 slots), then one LDS address per lane --
// no per-element 64-bit addresses and no lane-dependent branches, which this kernel has no registers for.
__device__ __forceinline__ void ct_fetch(float *slot, const float *p, int64_t row0, int n_live, int ld, int lane) {
    const float *src = p + row0 * ld;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll 1
    for (int i = lane; i < n_live * ld; i += 64) slot[i] = src[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

__device__ __forceinline__ void ct_flush(float *p, const float *slot, int64_t row0, int n_live, int ld, int lane) {
    float *dst = p + row0 * ld;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll 1
    for (int i = lane; i < n_live * ld; i += 64) dst[i] = slot[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// columns c0 + kmap(r, h) of the lane's row of a fetched block (0 beyond the live rows and beyond column ld)
__device__ __forceinline__ void ct_take(f32x16 &v, const float *slot, int ld, int c0, bool live, int lane) {
    const float *pr = slot + (lane & 31) * ld + c0 + 4 * (lane >> 5);
    const int room = ld - c0 - 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = sx_kmap(r, 0);
        const float t = pr[f];                       // (inside the wave's scratch whatever f is)
        v[r] = (live && f < room) ? t : 0.f;
    }
}

// the reverse: columns c0 + kmap(r, h) of the lane's row (columns beyond ld go to the spare words at `spare`)
__device__ __forceinline__ void ct_give(float *slot, const f32x16 &v, int ld, int c0, int spare, int lane) {
    const int h = lane >> 5, n = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = c0 + sx_kmap(r, h);
        slot[f < ld ? n * ld + f : spare + n] = v[r];
    }
}

__device__ __forceinline__ float ct_stage_time(int solver, int st, float ta, float tb, float dt, float half, float third, float two_thirds) {
    if (st == 0) return ta;
    if (solver == SX_CNF_MIDPOINT) return ta + half;
    return st == 1 ? ta + dt * third : st == 2 ? ta + dt * two_thirds : tb;
}

template <int NH, int SOLVER>
__global__ __launch_bounds__(SX_CNF_THREADS) void cnf_train_bwd_kernel(const ct_args a) {
    ct_stage_all<NH>(a, true);
    __syncthreads();
    const sx_cnf_net &net = a.net;
    const int D = net.dim, L = net.latent_dim, in_dim = 1 + D + L, H1 = net.layer[0].out_dim, act = net.act;
    const int LT = (L + 31) >> 5;
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;
    // the wave's scratch: two transposition slots, the stage inputs z_1 .. z_3 (also the staging area of the latent rows), e, gx
    float *sA = cnf_smem + a.base_scr + wave * a.scr_stride, *sB = sA + SX_TC_SLOT, *zb = sB + SX_TC_SLOT, *sE = zb + 3 * 1024, *sY = sE + 1024;
    float *sL = sY + SX_TC_SLOT + lane;          // sum a1b of the group's rows (read by the latent columns only), [register][lane]
    float *sP = zb + 2 * 1024 + lane, *sQ = zb + 1024 + lane;          // the tableau's two carried tiles, in the z slots their stages have left
    float *part = a.partial + ((int64_t)blockIdx.x * SX_CNF_WAVES + wave) * a.part_floats;
    const float sgn = a.t1 < a.t0 ? -1.f : 1.f;
    const int n_stages = cnf_stages(SOLVER);
    const float third = 1.f / 3.f, two_thirds = 2.f / 3.f;
    // the accumulators of the whole pass loop
    f32x16 gW1 = {}, gWl = {}, gW2 = {};
    float gb1 = 0.f, gtc = 0.f, gb2 = 0.f, gbl = 0.f;
    for (int i = lane; i < LT * 1024; i += 64) part[a.off_lat + i] = 0.f;

    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_CNF_WAVES + wave; grp < n_groups; grp += (int64_t)gridDim.x * SX_CNF_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        // the running adjoint of the state lives in gx between the stages, and e is re-read and u1, v are recomputed where an
        // evaluation needs them: registers are what limits this kernel, and these are a tile load or a tile product each
        const int64_t row0 = grp * 32;
        const int n_live = a.n_rows - row0 < 32 ? (int)(a.n_rows - row0) : 32;
        ct_fetch(sY, a.gy, row0, n_live, D, lane);
        ct_fetch(sE, a.e, row0, n_live, D, lane);
        const float lb = a.gldj[live ? row : 0] * (live ? 1.f : 0.f);
        ct_tile lat;
        if (L > 0) ct_fetch(zb, a.latent, row0, n_live, L, lane);
        cnf_dense_latent<1>(a, lat, a.latent, row, live, lane, zb);
#pragma unroll
        for (int r = 0; r < 16; ++r) sL[r * 64] = 0.f;

#pragma unroll 1
        for (int i = a.n_steps - 1; i >= 0; --i) {
            float ta, tb;
            cnf_grid(a, sgn, i, ta, tb);
            const float dt = tb - ta, half = 0.5f * dt;
            if (n_stages > 1) {   // the stage inputs z_1 .. z_{S-1} (z_0 is the checkpoint): the forward's own tableau
                ct_tile k1, k2, xs, yy;
                ct_fetch(sA, a.ckpt_in + (int64_t)i * a.n_rows * D, row0, n_live, D, lane);
                ct_take(yy.v[0], sA, D, 0, live, lane);
                xs = yy;
                float q1 = 0.f, q2 = 0.f, ts = ta, l = 0.f;
#pragma unroll 1
                for (int st = 0; st + 1 < n_stages; ++st) {
                    ct_tile k, h1, h2;
                    cnf_dense_hidden<1, 1, NH, true>(a, xs, ts, lat, h1, h2, lane);
                    cnf_dense_out<1, 1, NH>(a, NH == 1 ? h1 : h2, k, lane);
                    cnf_tableau<1>(SOLVER, st, ta, tb, dt, half, third, two_thirds, k, 0.f, k1, k2, q1, q2, xs, ts, yy, l);
#pragma unroll
                    for (int r = 0; r < 16; ++r) zb[st * 1024 + r * 64 + lane] = xs.v[0][r];
                }
            }
            // the stages in reverse order: kb_i = dt (b_i yb + sum_{j > i} a_ji zb_j), qb_i = dt b_i lb.  Two tiles carry the zb_j
            // between the stages: rk4 -- after stage 3: P = zb_4; after 2: Q = zb_3; after 1: P = zb_4 - zb_3 / 3 + zb_2 / 3 (what
            // stage 0 needs) and Q = zb_4 + zb_3 + zb_2; midpoint -- P = zb_2
#pragma unroll 1
            for (int st = n_stages - 1; st >= 0; --st) {
                ct_tile z, kb, zbar, yb, e;
                ct_take(yb.v[0], sY, D, 0, live, lane);
                if (st == 0) {
                    ct_fetch(sA, a.ckpt_in + (int64_t)i * a.n_rows * D, row0, n_live, D, lane);
                    ct_take(z.v[0], sA, D, 0, live, lane);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) z.v[0][r] = zb[(st - 1) * 1024 + r * 64 + lane];
                }
                const float t = ct_stage_time(SOLVER, st, ta, tb, dt, half, third, two_thirds);
                float qb;
                if (SOLVER == SX_CNF_EULER || (SOLVER == SX_CNF_MIDPOINT && st == 1)) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) kb.v[0][r] = dt * yb.v[0][r];
                    qb = dt * lb;
                } else if (SOLVER == SX_CNF_MIDPOINT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) kb.v[0][r] = half * sP[r * 64];
                    qb = 0.f;
                } else {
                    const float by = (st == 3 || st == 0) ? 0.125f : 0.375f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float zsum = st == 3 ? 0.f : st == 1 ? sQ[r * 64] - sP[r * 64] : sP[r * 64];
                        kb.v[0][r] = dt * (by * yb.v[0][r] + zsum);
                    }
                    qb = (dt * by) * lb;
                }

                // ---- one evaluation's adjoint at (t, z) -------------------------------------------------------------------------
                ct_tile h1, h2, a1;
                cnf_dense_hidden<1, 1, NH, true>(a, z, t, lat, h1, h2, lane);
                SX_NO_HOIST();
                if constexpr (NH == 1) {
                    ct_tile hb1, u1, v;
                    cnf_gemm<1, 1>(kb, hb1, cnf_smem + a.base_t[1] + lane * 4);
                    // dW2 += kb h1^T + e (qb d1 u1)^T, db2 += kb
                    tc_put(sA, kb.v[0], lane);
                    gbl += tc_rowsum(sA, lane);
                    tc_put(sB, h1.v[0], lane);
                    tc_outer(gWl, sA, sB, lane);
                    ct_take(e.v[0], sE, D, 0, live, lane);
                    ct_row_constants<NH>(a, e, u1, v, lane);
                    tc_put(sA, e.v[0], lane);
                    f32x16 pv, d1, s1;
                    ct_dact_tile(h1.v[0], d1, act);
                    ct_d2act_tile(h1.v[0], d1, s1, act);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        pv[r] = (qb * d1[r]) * u1.v[0][r];
                        a1.v[0][r] = hb1.v[0][r] * d1[r] + ((qb * s1[r]) * u1.v[0][r]) * v.v[0][r];
                        u1.v[0][r] = (qb * d1[r]) * v.v[0][r];          // (the adjoint of u1)
                    }
                    tc_put(sB, pv, lane);
                    tc_outer(gWl, sA, sB, lane);
                    // the u1 adjoint's share of dW1x: (qb d1 v) e^T
                    tc_put(sB, e.v[0], lane);
                    tc_put(sA, u1.v[0], lane);
                    tc_outer(gW1, sA, sB, lane);
                } else {
                    ct_tile w, rr, hb2, a2, rb, wb, hb1, u1, v;
                    ct_take(e.v[0], sE, D, 0, live, lane);
                    ct_row_constants<NH>(a, e, u1, v, lane);
                    ct_dact_tile(h1.v[0], w.v[0], act);
#pragma unroll
                    for (int r = 0; r < 16; ++r) w.v[0][r] = w.v[0][r] * u1.v[0][r];
                    cnf_gemm<1, 1>(w, rr, cnf_smem + a.base_w[1] + lane * 4);
                    cnf_gemm<1, 1>(kb, hb2, cnf_smem + a.base_t[2] + lane * 4);
                    // dW3 += kb h2^T + e (qb d2 r)^T, db3 += kb
                    tc_put(sA, kb.v[0], lane);
                    gbl += tc_rowsum(sA, lane);
                    tc_put(sB, h2.v[0], lane);
                    tc_outer(gWl, sA, sB, lane);
                    tc_put(sA, e.v[0], lane);
                    f32x16 pv, d2, s2;
                    ct_dact_tile(h2.v[0], d2, act);
                    ct_d2act_tile(h2.v[0], d2, s2, act);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        pv[r] = (qb * d2[r]) * rr.v[0][r];
                        rb.v[0][r] = (qb * v.v[0][r]) * d2[r];
                        a2.v[0][r] = hb2.v[0][r] * d2[r] + ((qb * s2[r]) * v.v[0][r]) * rr.v[0][r];
                    }
                    tc_put(sB, pv, lane);
                    tc_outer(gWl, sA, sB, lane);
                    SX_NO_HOIST();
                    // dW2 += a2b h1^T + rb w^T, db2 += a2b
                    tc_put(sA, a2.v[0], lane);
                    gb2 += tc_rowsum(sA, lane);
                    tc_put(sB, h1.v[0], lane);
                    tc_outer(gW2, sA, sB, lane);
                    tc_put(sA, rb.v[0], lane);
                    tc_put(sB, w.v[0], lane);
                    tc_outer(gW2, sA, sB, lane);
                    SX_NO_HOIST();
                    cnf_gemm<1, 1>(rb, wb, cnf_smem + a.base_t[1] + lane * 4);
                    cnf_gemm<1, 1>(a2, hb1, cnf_smem + a.base_t[1] + lane * 4);
                    f32x16 d1, s1;
                    ct_dact_tile(h1.v[0], d1, act);
                    ct_d2act_tile(h1.v[0], d1, s1, act);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        a1.v[0][r] = hb1.v[0][r] * d1[r] + (wb.v[0][r] * s1[r]) * u1.v[0][r];
                        wb.v[0][r] = wb.v[0][r] * d1[r];          // (the adjoint of u1)
                    }
                    // the u1 adjoint's share of dW1x: (wb d1) e^T
                    ct_take(e.v[0], sE, D, 0, live, lane);
                    tc_put(sB, e.v[0], lane);
                    tc_put(sA, wb.v[0], lane);
                    tc_outer(gW1, sA, sB, lane);
                }
                // dW1x += a1b z^T, db1 += a1b, the time column += t a1b, and sum a1b for the latent columns
                tc_put(sB, z.v[0], lane);
                tc_put(sA, a1.v[0], lane);
                const float s = tc_rowsum(sA, lane);
                gb1 += s;
                gtc += t * s;
                tc_outer(gW1, sA, sB, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) sL[r * 64] += a1.v[0][r];
                SX_NO_HOIST();
                cnf_gemm<1, 1>(a1, zbar, cnf_smem + a.base_t[0] + lane * 4);

                if (SOLVER == SX_CNF_EULER || st == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) yb.v[0][r] += (SOLVER == SX_CNF_EULER ? 0.f : SOLVER == SX_CNF_MIDPOINT ? sP[r * 64] : sQ[r * 64]) + zbar.v[0][r];
                    ct_give(sY, yb.v[0], D, 0, 1024, lane);
                } else if (SOLVER == SX_CNF_MIDPOINT || st == 3) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) sP[r * 64] = zbar.v[0][r];
                } else if (st == 2) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) sQ[r * 64] = zbar.v[0][r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = sP[r * 64], q = sQ[r * 64];
                        sP[r * 64] = (p - q * third) + zbar.v[0][r] * third;
                        sQ[r * 64] = (p + q) + zbar.v[0][r];
                    }
                }
            }
        }

        ct_flush(a.gx, sY, row0, n_live, D, lane);

        if (L > 0) {
            const float *W1 = net.layer[0].W;
            f32x16 A1;
#pragma unroll
            for (int r = 0; r < 16; ++r) A1[r] = sL[r * 64];
            // g_latent = W1[:, latent]^T A1 (A fragments straight from global memory: once per group), gathered in LDS as rows
            if (a.glat != nullptr) {
                for (int c = 0; c < LT; ++c) {
                    f32x16 g = {};
                    const int lc = 32 * c + (lane & 31);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int j = sx_kmap(q, h);
                        const float t = W1[(int64_t)(j < H1 ? j : 0) * in_dim + 1 + D + (lc < L ? lc : 0)];
                        const float av = (lc < L && j < H1) ? t : 0.f;
                        g = __builtin_amdgcn_mfma_f32_32x32x2f32(av, A1[q], g, 0, 0, 0);
                    }
                    ct_give(zb, g, L, 32 * c, 2048, lane);
                }
                ct_flush(a.glat, zb, row0, n_live, L, lane);
            }
            // the latent columns of dW1 += A1 latent^T, into the wave's own partial
            ct_fetch(zb, a.latent, row0, n_live, L, lane);
            for (int c = 0; c < LT; ++c) {
                f32x16 lt, acc;
                ct_take(lt, zb, L, 32 * c, live, lane);
                tc_put(sB, lt, lane);
                float *p = part + a.off_lat + c * 1024 + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = p[r * 64];
                tc_put(sA, A1, lane);
                tc_outer(acc, sA, sB, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r * 64] = acc[r];
            }
        }
    }

    // one partial per wave: dW1x, dW_last (and dW2), then db1, the time column, db2 and db_last, 64 floats each
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        part[r * 64 + lane] = gW1[r];
        part[a.off_wl + r * 64 + lane] = gWl[r];
        if constexpr (NH == 2) part[a.off_w2 + r * 64 + lane] = gW2[r];
    }
    part[a.off_vec + lane] = gb1;
    part[a.off_vec + 64 + lane] = gtc;
    part[a.off_vec + 128 + lane] = gb2;
    part[a.off_vec + 192 + lane] = gbl;
    // the slots of the workgroups the launcher did not start hold zeros
    for (int64_t vb = (int64_t)blockIdx.x + gridDim.x; vb < a.n_virtual; vb += gridDim.x) {
        float *p = a.partial + (vb * SX_CNF_WAVES + wave) * a.part_floats;
        for (int i = lane; i < a.part_floats; i += 64) p[i] = 0.f;
    }
}

// ---- the partial sum: one thread per gradient element, the slots in order -------------------------------------------------------
struct ct_reduce_args {
    const float *partial;
    float *dW[3], *db[3];
    int n_slots, part_floats, NH, D, L, H1, H2;
    int off_w2, off_wl, off_lat, off_vec;
};

__global__ void cnf_train_reduce_kernel(const ct_reduce_args a) {
    const int in_dim = 1 + a.D + a.L, Hl = a.NH == 1 ? a.H1 : a.H2;
    const int n0 = a.H1 * in_dim, n1 = a.H1, n2 = a.NH == 2 ? a.H2 * a.H1 : 0, n3 = a.NH == 2 ? a.H2 : 0, n4 = a.D * Hl, n5 = a.D;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    float *dst = nullptr;
    int off = 0, pair = 0;          // pair: a bias-like entry, whose two row halves sit 32 floats apart
    if (i < n0) {
        const int j = i / in_dim, c = i - j * in_dim;
        dst = a.dW[0];
        if (c == 0) { off = a.off_vec + 64 + j; pair = 1; }
        else if (c <= a.D) off = tc_tile_off(j, c - 1);
        else off = a.off_lat + ((c - 1 - a.D) >> 5) * 1024 + tc_tile_off(j, (c - 1 - a.D) & 31);
    } else if ((i -= n0) < n1) {
        dst = a.db[0]; off = a.off_vec + i; pair = 1;
    } else if ((i -= n1) < n2) {
        const int k = i / a.H1, j = i - k * a.H1;
        dst = a.dW[1]; off = a.off_w2 + tc_tile_off(k, j);
    } else if ((i -= n2) < n3) {
        dst = a.db[1]; off = a.off_vec + 128 + i; pair = 1;
    } else if ((i -= n3) < n4) {
        const int d = i / Hl, j = i - d * Hl;
        dst = a.dW[a.NH]; off = a.off_wl + tc_tile_off(d, j);
    } else if ((i -= n4) < n5) {
        dst = a.db[a.NH]; off = a.off_vec + 192 + i; pair = 1;
    } else return;
    if (dst == nullptr) return;
    float s = 0.f;
    const float *p = a.partial + off;
    for (int k = 0; k < a.n_slots; ++k, p += a.part_floats) s += pair ? p[0] + p[32] : p[0];
    dst[i] = s;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int ct_check_net(const sx_cnf_net *net_host) {
    return cnf_dense_check_net("sx_cnf_train", net_host, SX_CNF_TRAIN_MAX_DIM, SX_CNF_TRAIN_MAX_IN, SX_CNF_TRAIN_MAX_HIDDEN);
}

// the LDS plan (floats): the forward images, the transposed ones, the waves' scratch; and the layout of a wave's partial
size_t ct_plan(const sx_cnf_net &net, bool backward, ct_args &a) {
    const int NH = net.n_layers - 1, LT = (net.latent_dim + 31) >> 5;
    size_t off = cnf_dense_plan(net, a);
    a.base_t[NH] = (int)off; off += 1024;
    if (backward) {
        a.base_t[0] = (int)off; off += 1024;
        if (NH == 2) { a.base_t[1] = (int)off; off += 1024; }
        a.base_scr = (int)off; a.scr_stride = 3 * SX_TC_SLOT + 5 * 1024;
        off += (size_t)SX_CNF_WAVES * a.scr_stride;
    }
    a.off_w2 = 1024;
    a.off_wl = a.off_w2 + (NH == 2 ? 1024 : 0);
    a.off_lat = a.off_wl + 1024;
    a.off_vec = a.off_lat + LT * 1024;
    a.part_floats = a.off_vec + 4 * 64;
    return off;
}

int64_t ct_virtual_blocks(int64_t n_rows) {
    const int64_t want = cnf_row_blocks(n_rows);
    return want < SX_CNF_TRAIN_MAX_BLOCKS ? want : SX_CNF_TRAIN_MAX_BLOCKS;
}

}  // namespace

extern "C" size_t sx_cnf_train_lds_bytes(const sx_cnf_net *net_host, int32_t backward) {
    if (ct_check_net(net_host) != SX_OK) return 0;
    ct_args a{};
    const size_t bytes = ct_plan(*net_host, backward != 0, a) * 4;
    return bytes <= SX_CNF_LDS_BYTES ? bytes : 0;
}

extern "C" int64_t sx_cnf_train_partial_floats(const sx_cnf_net *net_host, int64_t n_rows) {
    if (ct_check_net(net_host) != SX_OK || n_rows < 0) return 0;
    ct_args a{};
    ct_plan(*net_host, true, a);
    const int64_t blocks = ct_virtual_blocks(n_rows);
    return (blocks < 1 ? 1 : blocks) * SX_CNF_WAVES * a.part_floats;
}

extern "C" int sx_cnf_train_fwd(const sx_cnf_net *net_host, const float *x, const float *latent, const float *e, float *y, float *ldj,
                                float *checkpoints, int64_t n_rows, int32_t solver, int32_t n_steps, float t0, float t1, float step_size,
                                void *stream) {
    const int rc = ct_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_net &net = *net_host;
    const int rc_call = cnf_check_call("sx_cnf_train_fwd", solver, n_rows, 1, n_steps, step_size, x, y);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "sx_cnf_train_fwd: latent rows missing");
    SX_REQUIRE(e != nullptr && ldj != nullptr, "sx_cnf_train_fwd: null noise / ldj");
    ct_args a{};
    a.net = net;
    const size_t lds = ct_plan(net, false, a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_train_fwd: the padded weights need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    a.x = x; a.latent = latent; a.e = e; a.y = y; a.ldj = ldj; a.ckpt = checkpoints; a.n_rows = n_rows;
    a.solver = solver; a.n_steps = n_steps; a.t0 = t0; a.t1 = t1; a.step_size = step_size;
    const int64_t want = cnf_row_blocks(n_rows);
    if (net.n_layers == 2) return cnf_launch<cnf_train_fwd_kernel<1>>("sx_cnf_train_fwd", a, lds, want, stream);
    return cnf_launch<cnf_train_fwd_kernel<2>>("sx_cnf_train_fwd", a, lds, want, stream);
}

extern "C" int sx_cnf_train_bwd(const sx_cnf_net *net_host, const float *checkpoints, const float *latent, const float *e, const float *gy,
                                const float *gldj, float *gx, float *g_latent, float *partial, const sx_cnf_train_grads *grads,
                                int64_t n_rows, int32_t solver, int32_t n_steps, float t0, float t1, float step_size, void *stream) {
    const int rc = ct_check_net(net_host);
    if (rc != SX_OK) return rc;
    const sx_cnf_net &net = *net_host;
    const int rc_call = cnf_check_call("sx_cnf_train_bwd", solver, n_rows, 1, n_steps, step_size, gy, gx);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(net.latent_dim == 0 || latent != nullptr, "sx_cnf_train_bwd: latent rows missing");
    SX_REQUIRE(e != nullptr && gldj != nullptr && grads != nullptr, "sx_cnf_train_bwd: null noise / gldj / grads");
    SX_REQUIRE(n_steps == 0 || n_rows == 0 || checkpoints != nullptr, "sx_cnf_train_bwd: checkpoints missing");
    SX_REQUIRE(n_rows == 0 || partial != nullptr, "sx_cnf_train_bwd: the partial buffer is missing (sx_cnf_train_partial_floats)");
    ct_args a{};
    a.net = net;
    const size_t lds = ct_plan(net, true, a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "sx_cnf_train_bwd: the images and scratch need %zu bytes of LDS (budget %d)", lds, SX_CNF_LDS_BYTES);
    const int NH = net.n_layers - 1;
    const int64_t blocks = ct_virtual_blocks(n_rows);
    ct_reduce_args r{};
    r.partial = partial; r.n_slots = (int)(blocks * SX_CNF_WAVES); r.part_floats = a.part_floats;
    for (int l = 0; l < 3; ++l) { r.dW[l] = grads->dW[l]; r.db[l] = grads->db[l]; }
    r.NH = NH; r.D = net.dim; r.L = net.latent_dim;
    r.H1 = net.layer[0].out_dim; r.H2 = net.layer[1].out_dim;
    r.off_w2 = a.off_w2; r.off_wl = a.off_wl; r.off_lat = a.off_lat; r.off_vec = a.off_vec;
    if (n_rows > 0) {
        a.ckpt_in = checkpoints; a.latent = latent; a.e = e; a.gy = gy; a.gldj = gldj; a.gx = gx; a.glat = g_latent; a.partial = partial;
        a.n_rows = n_rows; a.n_virtual = (int)blocks;
        a.solver = solver; a.n_steps = n_steps; a.t0 = t0; a.t1 = t1; a.step_size = step_size;
        int rcl = SX_E_BADARG;
        // The solver is a template argument: with a run-time tableau the adjoint sweep does not fit the register file.  Hidden layers
        // of two tiles (33..64 units) are not built: their sweep needs 216 .. 1308 bytes of scratch per lane and more LDS than a
        // workgroup has, so those networks train on the composition path (SX_CNF_TRAIN_MAX_HIDDEN).
#define CT_CASE(N_)                                                                                                                 \
    if (NH == N_)                                                                                                                   \
        rcl = solver == SX_CNF_EULER      ? cnf_launch<cnf_train_bwd_kernel<N_, SX_CNF_EULER>>("sx_cnf_train_bwd", a, lds, blocks, stream)    \
              : solver == SX_CNF_MIDPOINT ? cnf_launch<cnf_train_bwd_kernel<N_, SX_CNF_MIDPOINT>>("sx_cnf_train_bwd", a, lds, blocks, stream) \
                                          : cnf_launch<cnf_train_bwd_kernel<N_, SX_CNF_RK4>>("sx_cnf_train_bwd", a, lds, blocks, stream);
        CT_CASE(1) CT_CASE(2)
#undef CT_CASE
        if (rcl != SX_OK) return rcl;
    }
    // (no rows: no slots, every wanted gradient is written as zero)
    const int in_dim = 1 + r.D + r.L, Hl = NH == 1 ? r.H1 : r.H2;
    const int total = r.H1 * in_dim + r.H1 + (NH == 2 ? r.H2 * r.H1 + r.H2 : 0) + r.D * Hl + r.D;
    hipLaunchKernelGGL(cnf_train_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, sx_stream(stream), r);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { sx_set_error("sx_cnf_train_bwd: reduce launch failed: %s", hipGetErrorString(err)); return (int)err; }
    return SX_OK;
}
