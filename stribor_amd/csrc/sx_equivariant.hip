// Deep Sets conditioner (net.EquivariantNet / net.EquivariantLayer, stribor/net/equivariant.py:6-93): the whole net in one launch
// (sx_equivariant_fwd) and its backward in one launch plus an ordered sum (sx_equivariant_bwd).  DESIGN.md section 4.16.
//
// Rows are set elements, the N = set_size elements of a set contiguous.  With h_0 = x, S = sum_j h_{l-1,j} over EVERY element of the
// set (masked ones included), layer l (A = l1.weight, a = l1.bias, B = l2.weight, b = l2.bias) is
//     no mask   z_i = (A h_{l-1,i} + a) + (B S + b) / N
//     mask      z_i = (A h_{l-1,i} + a) m_i + ((B S + b) m_i) / c,      m_i = mask[i], c = sum_j m_j     (a true division)
// h_l = act(z_l) for l < L, y = final_act(z_L).  A masked element has z = 0, hence h = act(0), which enters the next S; a set with
// c = 0 is NaN in every element, and no other set sees it.
//   * the conventions of sx_cnf_common.h: a workgroup of 4 waves = 128 row slots, one wave = 32 rows on the MFMA column, features on
//     the C rows, exact fp32 (v_mfma_f32_32x32x2_f32), weights in LDS in A-fragment order, cnf_launch and its pass loop;
//   * a workgroup takes floor(128 / N) WHOLE sets per pass: sets never straddle workgroups, they may straddle waves.  Slots past
//     the last set are padding: they compute on zeros (m = 1, c = 1) and are never stored;
//   * a set sum is sx_cnf_common.h's cnf_setsum through an LDS scratch [128][LD], its additions in row order; the scalar it carries
//     along is the mask on the first exchange, so c costs nothing;
//   * the descriptor holds the module's parameters themselves.  The A and B images of the layers go into LDS in layer order while
//     they fit SX_CNF_LDS_BYTES beside the vectors and the scratch; an image that does not fit is not staged, and its A fragments are
//     read from the parameter in global memory (bounds-checked scalar loads: the parameters are not padded, so cnf_mma_global's
//     16-byte reads do not apply).
//
// Backward (the mask gets no gradient).  e_l = dloss/dz_l, w_i = 1 / N or m_i / c, m_i = 1 without a mask:
//     dA_l = sum_i (m_i e_l,i) h_{l-1,i}^T,  da_l = sum_i m_i e_l,i,   r_l = sum_{i in set} w_i e_l,i  (per set),
//     dB_l = sum_sets r_l S_{l-1}^T,  db_l = sum_sets r_l,   dh_{l-1,i} = A_l^T (m_i e_l,i) + B_l^T r_l,   e_{l-1} = act'(h_{l-1}) dh_{l-1}
// One launch recomputes h_l from x (the forward saves nothing), walks the layers down with transpose products from transposed
// images staged once per workgroup, exchanges r_l through the same scratch, and contracts dA, da, dB, db over its rows with the
// same MFMA (sx_train_contract.h, shared with sx_cnf_train.hip and sx_resnet_bwd.hip: both operands turn through two per-wave LDS
// slots, feature-major; dB's row operand is r on the FIRST row of each set and zero elsewhere).  A wave owns one partial and
// accumulates into it in place: the first pass writes, later passes add, so nothing needs a zero-fill and no two waves touch the
// same word.  tc_reduce_kernel then sums the partials in slot order: no atomics, and two calls on the same inputs give the same bits.
// From sx_train_contract.h: the slots, tc_put / tc_add_tile / tc_add_rowsum, the transposed stager and the ordered sum; this file's
// own: eq_contract's loop nest over operands held in registers.  Both launches are cnf_launch.
#include "sx_cnf_common.h"
#include "sx_train_contract.h"

#define SX_EQ_BWD_MAX_BLOCKS 512         /* partial slots = 4 waves x min(passes, this) */
// the backward's instantiations (input tiles, hidden tiles, output tiles, layers): every shape within SX_EQUIVARIANT_BWD_MAX_* whose
// forward and transposed images all fit SX_CNF_LDS_BYTES beside the scratch and the slots (eq_bwd_resident)
#define EQ_BWD_CASES EQ_CASE(1, 1, 1, 2) EQ_CASE(1, 1, 2, 2) EQ_CASE(1, 2, 1, 2) EQ_CASE(1, 1, 1, 3) EQ_CASE(1, 1, 2, 3)

namespace {

struct eq_args {
    sx_equivariant_net net;
    int base_a[3], base_b[3];            // LDS float offsets of the A / B images; -1: read from the parameter
    int base_at[3], base_bt[3];          // ... of the transposed images (backward)
    int base_va[3], base_vb[3];          // ... of the biases
    int base_x;                          // ... of the exchange scratch [SX_CNF_ROWS][LD]
    int base_scr;                        // ... of the contraction slots (backward)
    int off_a[3], off_b[3], off_va[3], off_vb[3];      // float offsets inside a wave's partial
    int want_a[3], want_va[3], want_b[3], want_vb[3];
    int part_floats;
    const float *x, *mask, *gy;
    float *y, *dx, *partial;
    int64_t x_rs, mask_rs, n_rows;
};

// where a lane stands in its workgroup's pass
struct eq_row : cnf_set_pos {
    float mi, c;        // the row's mask value (1 without a mask) and its set's divisor: sum of the mask, or N
};

__device__ __forceinline__ int eq_in_dim(const sx_equivariant_net &net, int l) { return l == 0 ? net.in_dim : net.out_dim[l - 1]; }

// acc += (rows 32m .. 32m + 31 of W) . in -- from the LDS image at `base`, or (base < 0) from the parameter W [out_dim, in_dim] itself
template <int KT, bool G>
__device__ __forceinline__ void eq_mma(f32x16 &acc, const cnf_tile<KT> &in, int base, int m, const float *__restrict__ W, int out_dim, int in_dim,
                                       int lane) {
    if (!G || base >= 0) {
        cnf_mma<KT>(acc, in, cnf_smem + base + m * KT * 1024 + lane * 4);
        return;
    }
    const int row = 32 * m + (lane & 31), h = lane >> 5;
    const float *wr = W + (int64_t)row * in_dim;
#pragma unroll
    for (int c = 0; c < KT; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = 32 * c + 8 * g + 4 * h + j;
                const float w = (row < out_dim && col < in_dim) ? wr[col] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w, in.v[c][4 * g + j], acc, 0, 0, 0);
            }
}

// acc += (rows 32m .. 32m + 31 of W^T) . e -- from the transposed image at `base` (KT = W's output tiles)
template <int KT>
__device__ __forceinline__ void eq_mma_t(f32x16 &acc, const cnf_tile<KT> &e, int base, int m, int lane) {
    cnf_mma<KT>(acc, e, cnf_smem + base + m * KT * 1024 + lane * 4);
}

// tiles of layer l: KT inputs, MT outputs (NL layers; KT0 / HT / OT: input, hidden and output tiles of the net)
__host__ __device__ inline int eq_kt(int l, int KT0, int HT) { return l == 0 ? KT0 : HT; }
__host__ __device__ inline int eq_mt(int l, int NL, int HT, int OT) { return l == NL - 1 ? OT : HT; }

__device__ __forceinline__ void eq_stage(const eq_args &a, int KT0, int HT, int OT, bool backward) {
    const sx_equivariant_net &net = a.net;
    for (int l = 0; l < net.n_layers; ++l) {
        const int KT = eq_kt(l, KT0, HT), MT = eq_mt(l, net.n_layers, HT, OT), in = eq_in_dim(net, l), out = net.out_dim[l];
        if (a.base_a[l] >= 0) cnf_stage(net.A[l], out, in, in, 0, MT, KT, a.base_a[l]);
        if (a.base_b[l] >= 0) cnf_stage(net.B[l], out, in, in, 0, MT, KT, a.base_b[l]);
        cnf_stage_vec(net.a[l], out, 1, MT * 32, a.base_va[l]);
        cnf_stage_vec(net.b[l], out, 1, MT * 32, a.base_vb[l]);
        if (backward) {
            if (a.base_at[l] >= 0) tc_stage_t(cnf_smem + a.base_at[l], net.A[l], out, in, in, 0, KT, MT, SX_CNF_THREADS);
            if (a.base_bt[l] >= 0) tc_stage_t(cnf_smem + a.base_bt[l], net.B[l], out, in, in, 0, KT, MT, SX_CNF_THREADS);
        }
    }
}

// output tile m of z_l at the rows' inputs `hin` and their set sums `S`
template <int KT, bool G>
__device__ __forceinline__ void eq_z(const eq_args &a, int l, int m, const cnf_tile<KT> &hin, const cnf_tile<KT> &S, const eq_row &p, f32x16 &z,
                                     int lane) {
    SX_NO_HOIST();
    const int h = lane >> 5, in = eq_in_dim(a.net, l), out = a.net.out_dim[l];
    f32x16 u = {}, v = {};
    eq_mma<KT, G>(u, hin, a.base_a[l], m, a.net.A[l], out, in, lane);
    eq_mma<KT, G>(v, S, a.base_b[l], m, a.net.B[l], out, in, lane);
    const float *va = cnf_smem + a.base_va[l] + 4 * h, *vb = cnf_smem + a.base_vb[l] + 4 * h;
    const bool masked = a.mask != nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float y1 = u[r] + cnf_vec(va, m, r), y2 = v[r] + cnf_vec(vb, m, r);
        z[r] = masked ? y1 * p.mi + (y2 * p.mi) / p.c : y1 + y2 / p.c;
    }
}

template <int KT, int MT, bool G>
__device__ __forceinline__ void eq_hidden(const eq_args &a, int l, const cnf_tile<KT> &hin, const cnf_tile<KT> &S, const eq_row &p, cnf_tile<MT> &hout,
                                          int lane) {
#pragma unroll
    for (int m = 0; m < MT; ++m) eq_z<KT, G>(a, l, m, hin, S, p, hout.v[m], lane);
    cnf_act_all<MT>(hout, a.net.act);
}

// the lane's place in pass `pass`, its x row (zeros on padding) and its mask value
template <int KT0>
__device__ __forceinline__ void eq_begin(const eq_args &a, int64_t pass, eq_row &p, cnf_tile<KT0> &x, int lane) {
    const int N = a.net.set_size, h = lane >> 5, D = a.net.in_dim;
    p.rho = cnf_set_slot(lane);
    cnf_set_pass(p, pass, N, a.n_rows);
    const float *xr = a.x + p.row * a.x_rs;          // (cnf_load_row reads rows of stride D)
#pragma unroll
    for (int c = 0; c < KT0; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * c + sx_kmap(r, h);
            x.v[c][r] = (p.live && f < D) ? xr[f] : 0.f;
        }
    p.mi = (a.mask != nullptr && p.live) ? a.mask[p.row * a.mask_rs] : 1.f;
    p.c = (float)N;
}

template <int KT0, int HT, int NL>
__global__ __launch_bounds__(SX_CNF_THREADS) void equivariant_fwd_kernel(const eq_args a) {
    constexpr int LD = 32 * (KT0 > HT ? KT0 : HT) + 4;
    const int OT = cnf_tiles(a.net.out_dim[NL - 1]), out_dim = a.net.out_dim[NL - 1], fact = a.net.final_act;
    eq_stage(a, KT0, HT, OT, false);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int64_t n_passes = cnf_set_passes(a.net.set_size, a.n_rows);
    // (every bound of this loop is uniform over the workgroup: all four waves make every pass and meet at every barrier)
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        eq_row p;
        cnf_tile<KT0> x, S0;
        eq_begin<KT0>(a, pass, p, x, lane);
        float c;
        cnf_setsum<KT0, LD>(a.base_x, a.net.set_size, p, x, S0, p.mi, c, lane);
        if (a.mask != nullptr) p.c = c;
        cnf_tile<HT> hl, Sl;
        eq_hidden<KT0, HT, true>(a, 0, x, S0, p, hl, lane);
        float unused;
        if (NL == 3) {
            cnf_tile<HT> h1 = hl;
            cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h1, Sl, 0.f, unused, lane);
            eq_hidden<HT, HT, true>(a, 1, h1, Sl, p, hl, lane);
        }
        cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, hl, Sl, 0.f, unused, lane);
        float *yr = a.y + p.row * out_dim;
#pragma nounroll
        for (int m = 0; m < OT; ++m) {
            f32x16 z;
            eq_z<HT, true>(a, NL - 1, m, hl, Sl, p, z, lane);
            if (p.live) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * m + sx_kmap(r, h);
                    if (f < out_dim) yr[f] = cnf_act(z[r], fact);
                }
            }
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// W += X Y^T and v += sum X over the wave's 32 rows, into the wave's partial (pw: MT x KT tiles, pv: MT x 64 floats)
template <int MT, int KT>
__device__ __forceinline__ void eq_contract(const cnf_tile<MT> &X, const cnf_tile<KT> &Y, float *pw, float *pv, bool want_w, bool want_v, bool first,
                                            float *sA, float *sB, int lane) {
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

// one layer down: from e = e_l (in place: becomes m_i e_l), the layer's inputs hin and (when dB is wanted) their set sums Sin, the
// wave's share of dA, da, dB, db and -- want_dh -- dh_{l-1}
template <int KT, int MT, int LD>
__device__ __forceinline__ void eq_bwd_layer(const eq_args &a, int l, const eq_row &p, cnf_tile<MT> &e, const cnf_tile<KT> &hin, const cnf_tile<KT> &Sin,
                                             cnf_tile<KT> &dh, bool want_dh, float *part, bool first, float *sA, float *sB, int lane) {
    const bool masked = a.mask != nullptr;
    cnf_tile<MT> r;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) r.v[m][q] = masked ? (e.v[m][q] / p.c) * p.mi : e.v[m][q] / p.c;
    float unused;
    cnf_setsum<MT, LD>(a.base_x, a.net.set_size, p, r, r, 0.f, unused, lane);
    if (masked) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) e.v[m][q] = e.v[m][q] * p.mi;
    }
    if (a.want_a[l] || a.want_va[l])
        eq_contract<MT, KT>(e, hin, part + a.off_a[l], part + a.off_va[l], a.want_a[l] != 0, a.want_va[l] != 0, first, sA, sB, lane);
    if (a.want_b[l] || a.want_vb[l]) {
        const bool head = p.live && p.rho == p.first;         // r counts once per set: on its first row
        cnf_tile<MT> rh;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) rh.v[m][q] = head ? r.v[m][q] : 0.f;
        eq_contract<MT, KT>(rh, Sin, part + a.off_b[l], part + a.off_vb[l], a.want_b[l] != 0, a.want_vb[l] != 0, first, sA, sB, lane);
    }
    if (want_dh) {
#pragma unroll
        for (int m = 0; m < KT; ++m) {
            SX_NO_HOIST();
            f32x16 acc = {};
            eq_mma_t<MT>(acc, e, a.base_at[l], m, lane);
            eq_mma_t<MT>(acc, r, a.base_bt[l], m, lane);
            dh.v[m] = acc;
        }
    }
}

// dh <- act'(h) dh from hout = act(h) (a product, not cnf_dact_all's sweep in place)
template <int T>
__device__ __forceinline__ void eq_times_dact(cnf_tile<T> &dh, const cnf_tile<T> &hout, int act) {
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) dh.v[m][r] = cnf_dact(hout.v[m][r], act) * dh.v[m][r];
}

template <int KT0, int HT, int OT, int NL>
__global__ __launch_bounds__(SX_CNF_THREADS) void equivariant_bwd_kernel(const eq_args a) {
    constexpr int XT = KT0 > HT ? KT0 : HT, LD = 32 * (XT > OT ? XT : OT) + 4;
    const int out_dim = a.net.out_dim[NL - 1], fact = a.net.final_act, act = a.net.act, D = a.net.in_dim;
    eq_stage(a, KT0, HT, OT, true);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    float *sA = cnf_smem + a.base_scr + wave * 2 * SX_TC_SLOT, *sB = sA + SX_TC_SLOT;
    float *part = a.partial + ((int64_t)blockIdx.x * SX_CNF_WAVES + wave) * a.part_floats;
    const int64_t n_passes = cnf_set_passes(a.net.set_size, a.n_rows);
    bool first = true;
    // (every bound of this loop, and every want flag, is uniform over the workgroup: all four waves meet at every barrier)
    for (int64_t pass = blockIdx.x; pass < n_passes; pass += gridDim.x) {
        eq_row p;
        cnf_tile<KT0> x, S0;
        eq_begin<KT0>(a, pass, p, x, lane);
        float c, unused;
        cnf_setsum<KT0, LD>(a.base_x, a.net.set_size, p, x, S0, p.mi, c, lane);
        if (a.mask != nullptr) p.c = c;
        // ---- the forward again: h_1 (, h_2), y
        cnf_tile<HT> h1, h2, Sl;
        eq_hidden<KT0, HT, false>(a, 0, x, S0, p, h1, lane);
        if (NL == 3) {
            cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h1, Sl, 0.f, unused, lane);
            eq_hidden<HT, HT, false>(a, 1, h1, Sl, p, h2, lane);
        }
        const cnf_tile<HT> &hl = NL == 3 ? h2 : h1;
        cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, hl, Sl, 0.f, unused, lane);
        // ---- e_L = final_act'(y) gy (zero on padding rows and padded features)
        cnf_tile<OT> e;
        const float *gr = tc_here(a.gy + p.row * out_dim);
#pragma unroll
        for (int m = 0; m < OT; ++m) {
            f32x16 z;
            eq_z<HT, false>(a, NL - 1, m, hl, Sl, p, z, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * m + sx_kmap(r, h);
                e.v[m][r] = (p.live && f < out_dim) ? cnf_dact(cnf_act(z[r], fact), fact) * gr[f] : 0.f;
            }
        }
        // ---- the layers, last to first
        cnf_tile<HT> dh;
        eq_bwd_layer<HT, OT, LD>(a, NL - 1, p, e, hl, Sl, dh, true, part, first, sA, sB, lane);
        if (NL == 3) {
            eq_times_dact<HT>(dh, h2, act);
            if (a.want_b[1]) cnf_setsum<HT, LD>(a.base_x, a.net.set_size, p, h1, Sl, 0.f, unused, lane);
            cnf_tile<HT> e2 = dh;
            eq_bwd_layer<HT, HT, LD>(a, 1, p, e2, h1, Sl, dh, true, part, first, sA, sB, lane);
        }
        eq_times_dact<HT>(dh, h1, act);
        cnf_tile<KT0> dx;
        if (a.want_b[0]) cnf_setsum<KT0, LD>(a.base_x, a.net.set_size, p, x, S0, 0.f, unused, lane);
        eq_bwd_layer<KT0, HT, LD>(a, 0, p, dh, x, S0, dx, a.dx != nullptr, part, first, sA, sB, lane);
        if (a.dx != nullptr && p.live) {
            float *dr = tc_here(a.dx + p.row * D);
#pragma unroll
            for (int m = 0; m < KT0; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * m + sx_kmap(r, h);
                    if (f < D) dr[f] = dx.v[m][r];
                }
        }
        first = false;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the shape of the network alone (no pointer is read)
int eq_check_shape(const char *fn, const sx_equivariant_net *net_host, bool backward) {
    SX_REQUIRE(net_host != nullptr, "%s: null network", fn);
    const sx_equivariant_net &net = *net_host;
    const int max_in = backward ? SX_EQUIVARIANT_BWD_MAX_IN : SX_EQUIVARIANT_MAX_IN;
    const int max_hidden = backward ? SX_EQUIVARIANT_BWD_MAX_HIDDEN : SX_EQUIVARIANT_MAX_HIDDEN;
    const int max_out = backward ? SX_EQUIVARIANT_BWD_MAX_OUT : SX_EQUIVARIANT_MAX_OUT;
    SX_REQUIRE(net.n_layers == 2 || net.n_layers == 3, "%s: one or two hidden layers (got %d equivariant layers)", fn, net.n_layers);
    SX_REQUIRE(net.in_dim >= 1 && net.in_dim <= max_in, "%s: in_dim must be in 1..%d (got %d)", fn, max_in, net.in_dim);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU && net.final_act >= SX_ACT_IDENTITY && net.final_act <= SX_ACT_LEAKYRELU,
               "%s: activation codes must be in 0..%d (got %d, %d)", fn, SX_ACT_LEAKYRELU, net.act, net.final_act);
    SX_REQUIRE(net.set_size >= 1 && net.set_size <= SX_EQUIVARIANT_MAX_SIZE, "%s: set_size must be in 1..%d (got %d)", fn,
               SX_EQUIVARIANT_MAX_SIZE, net.set_size);
    for (int l = 0; l + 1 < net.n_layers; ++l)
        SX_REQUIRE(net.out_dim[l] >= 1 && net.out_dim[l] <= max_hidden, "%s: hidden layer %d must have 1..%d units (got %d)", fn, l, max_hidden,
                   net.out_dim[l]);
    const int out = net.out_dim[net.n_layers - 1];
    SX_REQUIRE(out >= 1 && out <= max_out, "%s: out_dim must be in 1..%d (got %d)", fn, max_out, out);
    return SX_OK;
}

void eq_tiles(const sx_equivariant_net &net, int &KT0, int &HT, int &OT) {
    KT0 = cnf_tiles(net.in_dim);
    HT = 1;
    for (int l = 0; l + 1 < net.n_layers; ++l) HT = cnf_tiles(net.out_dim[l]) > HT ? cnf_tiles(net.out_dim[l]) : HT;
    OT = cnf_tiles(net.out_dim[net.n_layers - 1]);
}

// the LDS plan (floats) and -- backward -- the layout of a wave's partial.  Vectors, scratch and slots first; then the images in
// layer order (A, B, and for the backward A^T, B^T) while they fit: the others are read from the parameters.
size_t eq_plan(const sx_equivariant_net &net, bool backward, eq_args &a) {
    int KT0, HT, OT;
    eq_tiles(net, KT0, HT, OT);
    const int NL = net.n_layers;
    size_t off = 0;
    int poff = 0;
    for (int l = 0; l < NL; ++l) {
        const int MT = eq_mt(l, NL, HT, OT);
        a.base_va[l] = (int)off; off += (size_t)MT * 32;
        a.base_vb[l] = (int)off; off += (size_t)MT * 32;
    }
    int XT = KT0 > HT ? KT0 : HT;
    if (backward && OT > XT) XT = OT;
    a.base_x = (int)off; off += (size_t)SX_CNF_ROWS * (32 * XT + 4);
    a.base_scr = (int)off;
    if (backward) off += (size_t)SX_CNF_WAVES * 2 * SX_TC_SLOT;
    for (int l = 0; l < 3; ++l) a.base_a[l] = a.base_b[l] = a.base_at[l] = a.base_bt[l] = -1;
    for (int l = 0; l < NL; ++l) {
        const size_t img = (size_t)eq_mt(l, NL, HT, OT) * eq_kt(l, KT0, HT) * 1024;
        int *slots[4] = {&a.base_a[l], &a.base_b[l], &a.base_at[l], &a.base_bt[l]};
        for (int k = 0; k < (backward ? 4 : 2); ++k)
            if ((off + img) * 4 <= SX_CNF_LDS_BYTES) { *slots[k] = (int)off; off += img; }
        a.off_a[l] = poff; poff += (int)img;
        a.off_b[l] = poff; poff += (int)img;
        a.off_va[l] = poff; poff += eq_mt(l, NL, HT, OT) * 64;
        a.off_vb[l] = poff; poff += eq_mt(l, NL, HT, OT) * 64;
    }
    a.part_floats = poff;
    return off;
}

// the backward reads every image from LDS: inside its coverage they all fit
bool eq_bwd_resident(const sx_equivariant_net &net, const eq_args &a) {
    for (int l = 0; l < net.n_layers; ++l)
        if (a.base_a[l] < 0 || a.base_b[l] < 0 || a.base_at[l] < 0 || a.base_bt[l] < 0) return false;
    return true;
}

int64_t eq_bwd_blocks(int64_t n_rows, int set_size) {
    const int64_t want = cnf_set_blocks(n_rows, set_size);
    return want < SX_EQ_BWD_MAX_BLOCKS ? want : SX_EQ_BWD_MAX_BLOCKS;
}

// what both entry points ask of their common arguments
int eq_check_call(const char *fn, const sx_equivariant_net &net, const float *x, int64_t x_rs, const float *mask, int64_t mask_rs, int64_t n_rows) {
    for (int l = 0; l < net.n_layers; ++l) {
        SX_REQUIRE(net.A[l] != nullptr && net.a[l] != nullptr && net.B[l] != nullptr && net.b[l] != nullptr, "%s: layer %d lacks a weight or a bias", fn, l);
        SX_REQUIRE(sx_aligned4(net.A[l]) && sx_aligned4(net.a[l]) && sx_aligned4(net.B[l]) && sx_aligned4(net.b[l]),
                   "%s: layer %d has a pointer that is not 4-byte aligned", fn, l);
    }
    SX_REQUIRE(n_rows >= 0, "%s: negative n_rows", fn);
    SX_REQUIRE(n_rows % net.set_size == 0, "%s: n_rows (%lld) is not a multiple of set_size (%d)", fn, (long long)n_rows, net.set_size);
    SX_REQUIRE(x != nullptr && sx_aligned4(x), "%s: x is null or not 4-byte aligned", fn);
    SX_REQUIRE(x_rs >= net.in_dim, "%s: the row stride of x (%lld) is below in_dim (%d)", fn, (long long)x_rs, net.in_dim);
    SX_REQUIRE(mask == nullptr || (sx_aligned4(mask) && mask_rs >= 1), "%s: the mask is not 4-byte aligned, or its row stride (%lld) is below 1", fn,
               (long long)mask_rs);
    return SX_OK;
}

}  // namespace

extern "C" size_t sx_equivariant_lds_bytes(const sx_equivariant_net *net_host, int32_t backward) {
    if (eq_check_shape("sx_equivariant_lds_bytes", net_host, backward != 0) != SX_OK) return 0;
    eq_args a{};
    const size_t bytes = eq_plan(*net_host, backward != 0, a) * 4;
    if (backward && !eq_bwd_resident(*net_host, a)) return 0;
    return bytes <= SX_CNF_LDS_BYTES ? bytes : 0;
}

extern "C" size_t sx_equivariant_bwd_partial_floats(const sx_equivariant_net *net_host, int64_t n_rows) {
    if (eq_check_shape("sx_equivariant_bwd_partial_floats", net_host, true) != SX_OK || n_rows <= 0) return 0;
    eq_args a{};
    eq_plan(*net_host, true, a);
    return (size_t)eq_bwd_blocks(n_rows, net_host->set_size) * SX_CNF_WAVES * (size_t)a.part_floats;
}

extern "C" int sx_equivariant_fwd(const sx_equivariant_net *net_host, const float *x, int64_t x_rs, const float *mask, int64_t mask_rs, float *y,
                                  int64_t n_rows, void *stream) {
    const char *fn = "sx_equivariant_fwd";
    const int rc = eq_check_shape(fn, net_host, false);
    if (rc != SX_OK) return rc;
    const sx_equivariant_net &net = *net_host;
    const int rc_call = eq_check_call(fn, net, x, x_rs, mask, mask_rs, n_rows);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(y != nullptr && sx_aligned4(y), "%s: y is null or not 4-byte aligned", fn);
    eq_args a{};
    a.net = net;
    const size_t lds = eq_plan(net, false, a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES, "%s: the vectors and the scratch need %zu bytes of LDS (budget %d)", fn, lds, SX_CNF_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    a.x = x; a.x_rs = x_rs; a.mask = mask; a.mask_rs = mask_rs; a.y = y; a.n_rows = n_rows;
    int KT0, HT, OT;
    eq_tiles(net, KT0, HT, OT);
    const int NL = net.n_layers;
    const int64_t want = cnf_set_blocks(n_rows, net.set_size);
#define EQ_CASE(K_, H_, N_) if (KT0 == K_ && HT == H_ && NL == N_) return cnf_launch<equivariant_fwd_kernel<K_, H_, N_>>(fn, a, lds, want, stream);
    EQ_CASE(1, 1, 2) EQ_CASE(1, 2, 2) EQ_CASE(2, 1, 2) EQ_CASE(2, 2, 2)
    EQ_CASE(1, 1, 3) EQ_CASE(1, 2, 3) EQ_CASE(2, 1, 3) EQ_CASE(2, 2, 3)
#undef EQ_CASE
    sx_set_error("%s: no kernel for %d input tiles, %d hidden tiles, %d layers", fn, KT0, HT, NL);
    return SX_E_UNSUPPORTED;
}

extern "C" int sx_equivariant_bwd(const sx_equivariant_net *net_host, const float *x, int64_t x_rs, const float *mask, int64_t mask_rs,
                                  const float *gy, float *dx, float *partial, const sx_equivariant_grads *grads, int64_t n_rows, void *stream) {
    const char *fn = "sx_equivariant_bwd";
    const int rc = eq_check_shape(fn, net_host, true);
    if (rc != SX_OK) return rc;
    const sx_equivariant_net &net = *net_host;
    const int rc_call = eq_check_call(fn, net, x, x_rs, mask, mask_rs, n_rows);
    if (rc_call != SX_OK) return rc_call;
    SX_REQUIRE(gy != nullptr && sx_aligned4(gy), "%s: gy is null or not 4-byte aligned", fn);
    SX_REQUIRE(sx_aligned4(dx) && sx_aligned4(partial), "%s: dx or the partial buffer is not 4-byte aligned", fn);
    eq_args a{};
    a.net = net;
    const size_t lds = eq_plan(net, true, a) * 4;
    SX_REQUIRE(lds <= SX_CNF_LDS_BYTES && eq_bwd_resident(net, a), "%s: the images, the scratch and the slots do not fit %d bytes of LDS", fn,
               SX_CNF_LDS_BYTES);
    int KT0, HT, OT;
    eq_tiles(net, KT0, HT, OT);
    const int NL = net.n_layers;
    tc_reduce_args<12> r{};              // per layer: dA, da, dB, db
    bool any = false;
    int total = 0;
    for (int l = 0; l < NL; ++l) {
        float *g[4] = {nullptr, nullptr, nullptr, nullptr};
        if (grads != nullptr) { g[0] = grads->dA[l]; g[1] = grads->da[l]; g[2] = grads->dB[l]; g[3] = grads->db[l]; }
        const int off[4] = {a.off_a[l], a.off_va[l], a.off_b[l], a.off_vb[l]};
        for (int k = 0; k < 4; ++k) {
            SX_REQUIRE(sx_aligned4(g[k]), "%s: a gradient of layer %d is not 4-byte aligned", fn, l);
            any = any || g[k] != nullptr;
            const int cols = (k & 1) ? 0 : (l == 0 ? net.in_dim : net.out_dim[l - 1]);
            r.e[4 * l + k] = {g[k], net.out_dim[l], cols, eq_kt(l, KT0, HT), off[k]};
            total += net.out_dim[l] * ((k & 1) ? 1 : cols);
        }
        a.want_a[l] = g[0] != nullptr; a.want_va[l] = g[1] != nullptr; a.want_b[l] = g[2] != nullptr; a.want_vb[l] = g[3] != nullptr;
    }
    SX_REQUIRE(any || dx != nullptr, "%s: nothing to compute (no dx and no parameter gradient)", fn);
    SX_REQUIRE(!any || n_rows == 0 || partial != nullptr, "%s: the partial buffer is missing (sx_equivariant_bwd_partial_floats)", fn);
    int grid = 0;
    if (n_rows > 0) {
        a.x = x; a.x_rs = x_rs; a.mask = mask; a.mask_rs = mask_rs; a.gy = gy; a.dx = dx; a.partial = partial; a.n_rows = n_rows;
        const int64_t want = eq_bwd_blocks(n_rows, net.set_size);
        int rc_k = SX_E_UNSUPPORTED;
#define EQ_CASE(K_, H_, O_, N_) if (KT0 == K_ && HT == H_ && OT == O_ && NL == N_) rc_k = cnf_launch<equivariant_bwd_kernel<K_, H_, O_, N_>>(fn, a, lds, want, stream, &grid);
        EQ_BWD_CASES
#undef EQ_CASE
        if (rc_k == SX_E_UNSUPPORTED) sx_set_error("%s: no kernel for %d / %d / %d tiles, %d layers", fn, KT0, HT, OT, NL);
        if (rc_k != SX_OK) return rc_k;
    }
    if (!any) return SX_OK;
    // every wave of every workgroup launched wrote its slot on its first pass (no rows: no slots, the gradients are zero)
    r.partial = partial; r.part_floats = a.part_floats; r.n_slots = grid * SX_CNF_WAVES;
    return tc_reduce(fn, r, total, stream);
}
