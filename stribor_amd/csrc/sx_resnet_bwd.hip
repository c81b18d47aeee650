// Backward of the invertible ResNet flows (IResNet / ContinuousIResNet, stribor/flows/iresnet.py:9-99): sx_resnet_flow_bwd.
//
// The network, as sx_resnet.hip runs it: h_0 = x, a_l = (W_l h_{l-1}) / sigma_l + b_l, h_l = phi_l(a_l) (l = 1..L), g = h_L,
// r = s (.) g.  For a cotangent c on r, with d_l = phi_l'(a_l):
//     e_L = d_L (.) s (.) c,    p_l = W_l^T e_l / sigma_l,    e_{l-1} = d_{l-1} (.) p_l,    J_r^T c = p_1
//     G_l = sum_rows e_l h_{l-1}^T  (w.r.t. the EFFECTIVE weight W_l / sigma_l),   db_l = sum_rows e_l,   gs = c (.) g
//   inverse == 0 (the backward of y = x + r(x)):        gout = gin + J_r(x)^T gin;  G, db, gs at c = gin
//   inverse != 0 (the implicit backward at x = x*):     w_0 = gin, w_{k+1} = gin - J_r(x*)^T w_k, `iterations` times;
//                                                       gout = w_K;  G, db, gs at c = -w_K
// Layout and arithmetic are sx_resnet.hip's (sx_resnet_common.h): one wave = 32 rows on the MFMA column, features on the C rows
// in sx_kmap order, exact fp32 v_mfma_f32_32x32x2_f32, grid-stride over 32-row groups.  Per group a wave
//   * recomputes a_l, h_l at x once (nothing is saved by the forward) and forms d_l once -- from the output where the output
//     determines it, from the pre-activation for SiLU and GELU; s is folded into d_L;
//   * runs the `iterations` transpose products from registers: a C tile of e_l is the B operand of W_l^T, whose A fragments come
//     from TRANSPOSED images staged beside the forward ones, once per workgroup;
//   * makes one more sweep at c, contracting G_l and db_l over its 32 rows with the same MFMA: both operands need the rows on the
//     K index, so e_l and h_{l-1} turn through two per-wave LDS slots (feature-major, stride 33); db_l is a row sum of e_l's slot.
// Between the evaluation and the sweep the hidden outputs wait in the wave's own words of the partial buffer, x is read again and g
// waits in the gs rows: the iteration's registers hold only gin, w, d_L (.) s and the d_l.
// A wave owns one partial (slot = 4 * block + wave).  The partial is the accumulator: the wave's first group writes it, each later
// group adds to it in place (twelve accumulator tiles of a 64 / [64, 64] network do not fit the register file beside the sweep's
// state), so nothing needs a zero-fill and no two waves ever touch the same word.  tc_reduce_kernel then sums the partials in slot
// order: no atomics anywhere, and two calls on the same inputs give the same bits.
// The slots, the contraction, the in-place accumulation, the transposed stager and the ordered sum are sx_train_contract.h's
// (shared with sx_cnf_train.hip and sx_equivariant.hip); this file's own are the recompute, the w iteration, the stash and the loop
// nest of rb_contract.  The launcher is sx_common.h's.
// Launches: ONE for the recompute, the w iteration and the contraction, plus the reduce when any dW / db is wanted: two in all
// (one for a pure vector-Jacobian product).
//
// Coverage (sx_resnet_bwd_lds_bytes): dim <= 64, hidden_dims of length 0..3 with widths <= 64 (one or two tiles each way), the
// eight SX_ACT_* codes for both activations, and forward + transposed images + scratch within SX_RESNET_LDS_BYTES -- dim 64 with
// [64, 64] takes 129.75 KiB; dim 64 with [64, 64, 64] would take 162 KiB and is outside.
#include "sx_resnet_common.h"
#include "sx_train_contract.h"

#define SX_RESNET_BWD_MAX_BLOCKS 512     /* partial slots = 4 waves x min(row blocks, this) */
namespace {

struct rb_args {
    sx_resnet_net net;
    int base[SX_RESNET_MAX_LAYERS];      // LDS float offset of each layer's forward image
    int base_t[SX_RESNET_MAX_LAYERS];    // ... of its transposed image
    int off_w[SX_RESNET_MAX_LAYERS];     // float offset of G_l inside a wave's partial
    int off_b[SX_RESNET_MAX_LAYERS];     // ... of db_l (64 floats per output tile: the two row halves)
    int want_w[SX_RESNET_MAX_LAYERS], want_b[SX_RESNET_MAX_LAYERS];
    int off_h;                           // ... of the stash: x, h_1 .. h_{L-1}, e_1 .. e_L of the group at hand
    int base_scr, part_floats, any_param;
    const float *x, *s_rows, *sigma, *gin;
    float *gout, *gs, *partial;
    int64_t n_rows;
    int iterations, inverse;
};

// h = phi(a) and d = phi'(a) of one tile, in place (v: a in, h out).  Once per layer and row group, so ONE rolled copy of the
// activation code per layer: the tile goes through the wave's LDS slots (each lane reads back its own words: no barrier) and a
// 16-trip loop instead of sixteen inlined copies.  d comes from the output where the output determines it, from a for SiLU / GELU.
__device__ __forceinline__ void rb_act_dact(f32x16 &v, f32x16 &d, int act, float *sA, float *sB, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sA[r * 64 + lane] = v[r];
#pragma nounroll
    for (int r = 0; r < 16; ++r) {
        const float a = sA[r * 64 + lane], h = rn_act(a, act);
        float dv;
        switch (act) {
            case SX_ACT_TANH: dv = 1.f - h * h; break;
            case SX_ACT_RELU: dv = h > 0.f ? 1.f : 0.f; break;
            case SX_ACT_SIGMOID: dv = h * (1.f - h); break;
            case SX_ACT_ELU: dv = h > 0.f ? 1.f : h + 1.f; break;
            case SX_ACT_SOFTPLUS: dv = 1.f - expf(-h); break;                        // sigmoid(a) = 1 - exp(-softplus(a))
            case SX_ACT_LEAKYRELU: dv = h > 0.f ? 1.f : 0.01f; break;
            case SX_ACT_SILU: { const float sg = 1.f / (1.f + expf(-a)); dv = sg * (1.f + a * (1.f - sg)); break; }
            case SX_ACT_GELU: dv = 0.5f * (1.f + erff(a * 0.70710678118654752f)) + a * 0.3989422804014327f * expf(-0.5f * a * a); break;
            default: dv = 1.f;
        }
        sA[r * 64 + lane] = h;
        sB[r * 64 + lane] = dv;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { v[r] = sA[r * 64 + lane]; d[r] = sB[r * 64 + lane]; }
}

// h = phi(a), d = phi'(a) of one layer at `in`
template <int KT, int MT>
__device__ __forceinline__ void rb_forward(const rtile<KT> &in, rtile<MT> &h, rtile<MT> &d, int base, float scale, int act, float *sA,
                                           float *sB, int lane) {
    SX_NO_HOIST();
    rn_layer<KT, MT>(in, h, base, scale, SX_ACT_IDENTITY, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        SX_NO_HOIST();
        rb_act_dact(h.v[m], d.v[m], act, sA, sB, lane);
    }
    SX_NO_HOIST();
}

// p[m] = (W^T . e)[m] * scale (* d[m]), m < MT; W^T: the transposed image at float offset `base` (KT tiles of e)
template <int KT, int MT, bool HAS_D>
__device__ __forceinline__ void rb_layer_t(const rtile<KT> &e, rtile<MT> &p, const rtile<MT> &d, int base, float scale, int lane) {
    const float *wb = rn_smem + base + lane * 4;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        SX_NO_HOIST();
        f32x16 acc = {};
#pragma unroll
        for (int c = 0; c < KT; ++c) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(wb + (m * KT + c) * 1024 + g * 256);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, e.v[c][4 * g + 0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, e.v[c][4 * g + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, e.v[c][4 * g + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, e.v[c][4 * g + 3], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) p.v[m][r] = HAS_D ? acc[r] * scale * d.v[m][r] : acc[r] * scale;
    }
}

// G += e h^T and db += sum e of one layer into the wave's partial; e (its MT output tiles) and h (its KT input tiles) come from the
// wave's stash, one tile at a time: nothing else is live here
template <int MT, int KT>
__device__ __forceinline__ void rb_contract(const float *est, const float *hst, float *pw, float *pb, bool want_w, bool want_b,
                                            bool first, float *sA, float *sB, int lane) {
    if (want_w) {
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            SX_NO_HOIST();
            f32x16 t;
            const float *hp = tc_here(hst + c * 1024);
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = hp[r * 64];
            tc_put(sB, t, lane);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                SX_NO_HOIST();
                const float *ep = tc_here(est + m * 1024);
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = ep[r * 64];
                tc_put(sA, t, lane);
                tc_add_tile(pw + (m * KT + c) * 1024 + lane, sA, sB, first, lane);
            }
        }
    }
    if (want_b) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            SX_NO_HOIST();
            f32x16 t;
            const float *ep = tc_here(est + m * 1024);
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = ep[r * 64];
            tc_put(sA, t, lane);
            tc_add_rowsum(pb + m * 64 + lane, sA, first, lane);
        }
    }
}

// a tile to / from the wave's own words of global memory (lane-private: each lane reads back what it wrote)
template <int T>
__device__ __forceinline__ void rb_stash(float *dst, const rtile<T> &t) {
#pragma unroll
    for (int m = 0; m < T; ++m) {
        float *p = tc_here(dst + m * 1024);
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r * 64] = t.v[m][r];
    }
}
template <int T>
__device__ __forceinline__ void rb_unstash(rtile<T> &t, const float *src) {
#pragma unroll
    for (int m = 0; m < T; ++m) {
        const float *p = tc_here(src + m * 1024);
#pragma unroll
        for (int r = 0; r < 16; ++r) t.v[m][r] = p[r * 64];
    }
}

// Rows move between global memory and the tiles through ONE 64-bit address per lane and array (rb_row_off) plus compile-time
// element offsets: per-element addresses would cost two registers each, for every array, across the whole iteration.
// element (c, r) of a lane: feature fo + 4 h, fo = rb_feat(c, r), at p[rb_row_off + fo]
__device__ __forceinline__ constexpr int rb_feat(int c, int r) { return 32 * c + sx_kmap(r, 0); }

template <int DT>
__device__ __forceinline__ void rb_load_rows(rtile<DT> &t, const float *src, int64_t off, bool live, int D4) {
    const float *p = src + off;
#pragma unroll
    for (int c = 0; c < DT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) t.v[c][r] = (live && rb_feat(c, r) < D4) ? p[rb_feat(c, r)] : 0.f;
}

template <int DT, int HT, int NL>
__global__ __launch_bounds__(SX_RESNET_THREADS) void resnet_bwd_kernel(const rb_args a) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == NL - 1 ? DT : HT;
        rn_stage_layer(a.net.layer[l].W, a.net.layer[l].b, a.net.layer[l].out_dim, a.net.layer[l].in_dim, MT, KT, a.base[l]);
        tc_stage_t(rn_smem + a.base_t[l], a.net.layer[l].W, a.net.layer[l].out_dim, a.net.layer[l].in_dim, a.net.layer[l].in_dim, 0, KT, MT,
                   SX_RESNET_THREADS);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, D = a.net.dim;
    const int act = a.net.act, fact = a.net.final_act;
    float *sA = rn_smem + a.base_scr + wave * 2 * SX_TC_SLOT, *sB = sA + SX_TC_SLOT;
    float sc[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int col = a.net.layer[l].sigma_col;
        sc[l] = col < 0 ? 1.f : 1.f / a.sigma[col];
    }
    const int64_t slot = (int64_t)blockIdx.x * SX_RESNET_WAVES + wave;
    // the wave's partial: G_l, db_l, then room for the hidden outputs h_1 .. h_{L-1} of the group at hand (the contraction's
    // operands wait there while the iteration runs).  Only dereferenced when a dW / db is wanted.
    float *part = a.partial + slot * a.part_floats;
    float *hst = part + a.off_h + lane;                      // x, h_1 .. h_{L-1}: the layers' inputs
    float *est = hst + (DT + (NL - 1) * HT) * 1024;          // e_1 .. e_L
    const bool params = a.any_param != 0;
    bool first = true;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = slot; grp < n_groups; grp += (int64_t)gridDim.x * SX_RESNET_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        rtile<DT> gin, ds;
        rtile<HT> d1, d2, d3;
        const int64_t off = row * D + 4 * h;                  // a lane's feature fo + 4 h of its row, fo = rb_feat(c, r)
        const int D4 = D - 4 * h;                             // ... exists when fo < D4
        rb_load_rows<DT>(gin, a.gin, off, live, D4);
        // ---- one evaluation at x: h_l (stashed) and d_l ----------------------------------------------------------------------
        {
            rtile<DT> x, g;
            rb_load_rows<DT>(x, a.x, off, live, D4);
            if (params) rb_stash<DT>(hst, x);
            if constexpr (NL == 1) {
                rb_forward<DT, DT>(x, g, ds, a.base[0], sc[0], fact, sA, sB, lane);
            } else {
                rtile<HT> ha, hb;
                rb_forward<DT, HT>(x, ha, d1, a.base[0], sc[0], act, sA, sB, lane);
                if (params) rb_stash<HT>(hst + DT * 1024, ha);
                if constexpr (NL >= 3) {
                    rb_forward<HT, HT>(ha, hb, d2, a.base[1], sc[1], act, sA, sB, lane);
                    if (params) rb_stash<HT>(hst + (DT + HT) * 1024, hb);
                }
                if constexpr (NL >= 4) {
                    rb_forward<HT, HT>(hb, ha, d3, a.base[2], sc[2], act, sA, sB, lane);
                    if (params) rb_stash<HT>(hst + (DT + 2 * HT) * 1024, ha);
                }
                rb_forward<HT, DT>(NL == 3 ? hb : ha, g, ds, a.base[NL - 1], sc[NL - 1], fact, sA, sB, lane);
            }
            // d_L (.) s: 0 on dead rows and padded features.  g waits in the gs rows for its cotangent factor.
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = live && rb_feat(c, r) < D4;
                    ds.v[c][r] = !ok ? 0.f : a.s_rows == nullptr ? ds.v[c][r] : ds.v[c][r] * (a.s_rows + off)[rb_feat(c, r)];
                    if (a.gs != nullptr && ok) (a.gs + off)[rb_feat(c, r)] = g.v[c][r];
                }
        }
        // ---- w_{k+1} = gin - J_r^T w_k ---------------------------------------------------------------------------------------
        rtile<DT> w = gin;
        if (a.inverse) {
            for (int k = 0; k < a.iterations; ++k) {
                rtile<DT> e, p;
#pragma unroll
                for (int c = 0; c < DT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) e.v[c][r] = ds.v[c][r] * w.v[c][r];
                if constexpr (NL == 1) {
                    rb_layer_t<DT, DT, false>(e, p, p, a.base_t[0], sc[0], lane);
                } else {
                    rtile<HT> ea, eb;
                    rb_layer_t<DT, HT, true>(e, ea, NL == 2 ? d1 : NL == 3 ? d2 : d3, a.base_t[NL - 1], sc[NL - 1], lane);
                    if constexpr (NL >= 3) rb_layer_t<HT, HT, true>(ea, eb, NL == 3 ? d1 : d2, a.base_t[NL - 2], sc[NL - 2], lane);
                    if constexpr (NL >= 4) rb_layer_t<HT, HT, true>(eb, ea, d1, a.base_t[1], sc[1], lane);
                    rb_layer_t<HT, DT, false>(NL == 3 ? eb : ea, p, p, a.base_t[0], sc[0], lane);
                }
#pragma unroll
                for (int c = 0; c < DT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) w.v[c][r] = gin.v[c][r] - p.v[c][r];
            }
        }
        // ---- the sweep at c (gin, or -w_K): gs, G_l, db_l, and J_r^T gin of the forward's backward ----------------------------
        if (!a.inverse || params || a.gs != nullptr) {
            rtile<DT> e, p;
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float cv = a.inverse ? -w.v[c][r] : gin.v[c][r];
                    e.v[c][r] = ds.v[c][r] * cv;
                    if (a.gs != nullptr && live && rb_feat(c, r) < D4) (a.gs + off)[rb_feat(c, r)] *= cv;          // gs = c (.) g
                }
            if constexpr (NL == 1) {
                if (params) rb_stash<DT>(est, e);
                if (!a.inverse) rb_layer_t<DT, DT, false>(e, p, p, a.base_t[0], sc[0], lane);
            } else {
                rtile<HT> ea, eb;
                if (params) rb_stash<DT>(est + (NL - 1) * HT * 1024, e);
                rb_layer_t<DT, HT, true>(e, ea, NL == 2 ? d1 : NL == 3 ? d2 : d3, a.base_t[NL - 1], sc[NL - 1], lane);
                if (params) rb_stash<HT>(est + (NL - 2) * HT * 1024, ea);
                if constexpr (NL >= 3) {
                    rb_layer_t<HT, HT, true>(ea, eb, NL == 3 ? d1 : d2, a.base_t[NL - 2], sc[NL - 2], lane);
                    if (params) rb_stash<HT>(est + (NL - 3) * HT * 1024, eb);
                }
                if constexpr (NL >= 4) {
                    rb_layer_t<HT, HT, true>(eb, ea, d1, a.base_t[1], sc[1], lane);
                    if (params) rb_stash<HT>(est, ea);
                }
                if (!a.inverse) rb_layer_t<HT, DT, false>(NL == 3 ? eb : ea, p, p, a.base_t[0], sc[0], lane);
            }
            if (!a.inverse) {
#pragma unroll
                for (int c = 0; c < DT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) w.v[c][r] = gin.v[c][r] + p.v[c][r];
            }
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (rb_feat(c, r) < D4) (a.gout + off)[rb_feat(c, r)] = w.v[c][r];
        }
        // ---- G_l += e_l h_{l-1}^T, db_l += sum e_l: every operand from the stash, no other state left ----------------------------
        if (params) {
            SX_NO_HOIST();
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                constexpr int in0 = 0;
                const int in_tile = l == 0 ? in0 : DT + (l - 1) * HT, e_tile = l * HT;
                const float *hp = hst + in_tile * 1024, *ep = est + e_tile * 1024;
                float *pw = part + a.off_w[l], *pb = part + a.off_b[l];
                const bool ww = a.want_w[l] != 0, wb = a.want_b[l] != 0;
                if (l == 0 && NL == 1) rb_contract<DT, DT>(ep, hp, pw, pb, ww, wb, first, sA, sB, lane);
                else if (l == 0) rb_contract<HT, DT>(ep, hp, pw, pb, ww, wb, first, sA, sB, lane);
                else if (l == NL - 1) rb_contract<DT, HT>(ep, hp, pw, pb, ww, wb, first, sA, sB, lane);
                else rb_contract<HT, HT>(ep, hp, pw, pb, ww, wb, first, sA, sB, lane);
            }
            first = false;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline int rb_tiles(int n) { return n <= 32 ? 1 : 2; }

// is this network inside the coverage?  (shape only: no pointer is looked at)
bool rb_covered(const sx_resnet_net *net) {
    if (!net || net->n_layers < 1 || net->n_layers > SX_RESNET_MAX_LAYERS) return false;
    if (net->dim < 1 || net->dim > SX_RESNET_BWD_MAX_WIDTH) return false;
    if (net->act < 0 || net->act > SX_ACT_GELU || net->final_act < 0 || net->final_act > SX_ACT_GELU) return false;
    if (net->n_wrapped < 0 || net->n_wrapped > SX_RESNET_MAX_LAYERS) return false;
    for (int l = 0; l < net->n_layers; ++l) {
        const sx_resnet_layer &L = net->layer[l];
        if (L.out_dim < 1 || L.out_dim > SX_RESNET_BWD_MAX_WIDTH) return false;
        if (L.in_dim != (l == 0 ? net->dim : net->layer[l - 1].out_dim)) return false;
        if (L.sigma_col >= net->n_wrapped) return false;
    }
    return net->layer[net->n_layers - 1].out_dim == net->dim;
}

// the LDS plan (floats) and the layout of a wave's partial
size_t rb_plan(const sx_resnet_net &net, rb_args &a, int &DT, int &HT) {
    DT = rb_tiles(net.dim);
    HT = 1;
    for (int l = 0; l + 1 < net.n_layers; ++l) HT = rb_tiles(net.layer[l].out_dim) > HT ? rb_tiles(net.layer[l].out_dim) : HT;
    size_t off = 0;
    int poff = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == net.n_layers - 1 ? DT : HT;
        a.base[l] = (int)off;
        off += (size_t)MT * KT * 1024 + (size_t)MT * 32;
        a.off_w[l] = poff;
        poff += MT * KT * 1024;
    }
    for (int l = 0; l < net.n_layers; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == net.n_layers - 1 ? DT : HT;
        a.base_t[l] = (int)off;
        off += (size_t)MT * KT * 1024;
        a.off_b[l] = poff;
        poff += MT * 64;
    }
    a.base_scr = (int)off;
    off += (size_t)SX_RESNET_WAVES * 2 * SX_TC_SLOT;
    a.off_h = poff;
    poff += 2 * (DT + (net.n_layers - 1) * HT) * 1024;        // the layers' inputs x, h_1 .. h_{L-1}, then e_1 .. e_L
    a.part_floats = poff;
    return off;
}

int64_t rb_blocks(int64_t n_rows) {
    const int64_t want = ((n_rows + 31) / 32 + SX_RESNET_WAVES - 1) / SX_RESNET_WAVES;
    return want < SX_RESNET_BWD_MAX_BLOCKS ? want : SX_RESNET_BWD_MAX_BLOCKS;
}

}  // namespace

extern "C" size_t sx_resnet_bwd_lds_bytes(const sx_resnet_net *net_host) {
    if (!rb_covered(net_host)) return 0;
    rb_args a{};
    int DT, HT;
    const size_t bytes = rb_plan(*net_host, a, DT, HT) * 4;
    return bytes <= SX_RESNET_LDS_BYTES ? bytes : 0;
}

extern "C" size_t sx_resnet_bwd_partial_floats(const sx_resnet_net *net_host, int64_t n_rows) {
    if (!rb_covered(net_host) || n_rows <= 0) return 0;
    rb_args a{};
    int DT, HT;
    rb_plan(*net_host, a, DT, HT);
    return (size_t)rb_blocks(n_rows) * SX_RESNET_WAVES * (size_t)a.part_floats;
}

extern "C" int sx_resnet_flow_bwd(const sx_resnet_net *net_host, const float *x, const float *s_rows, const float *sigma,
                                  const float *gin, float *gout, float *gs, float *partial, const sx_resnet_grads *grads,
                                  int64_t n_rows, int32_t iterations, int32_t inverse, void *stream) {
    SX_REQUIRE(net_host != nullptr, "sx_resnet_flow_bwd: null network");
    const sx_resnet_net &net = *net_host;
    SX_REQUIRE(net.n_layers >= 1 && net.n_layers <= SX_RESNET_MAX_LAYERS, "sx_resnet_flow_bwd: 1..%d Linear layers (got %d)",
               SX_RESNET_MAX_LAYERS, net.n_layers);
    SX_REQUIRE(net.dim >= 1 && net.dim <= SX_RESNET_BWD_MAX_WIDTH, "sx_resnet_flow_bwd: dim must be in 1..%d (got %d)",
               SX_RESNET_BWD_MAX_WIDTH, net.dim);
    SX_REQUIRE(rb_covered(net_host), "sx_resnet_flow_bwd: layer widths must be in 1..%d and chain from dim back to dim, activation "
               "codes in 0..%d, sigma columns below n_wrapped", SX_RESNET_BWD_MAX_WIDTH, SX_ACT_GELU);
    SX_REQUIRE(n_rows >= 0 && iterations >= 0, "sx_resnet_flow_bwd: negative n_rows / iterations");
    bool wrapped = false;
    for (int l = 0; l < net.n_layers; ++l) {
        SX_REQUIRE(net.layer[l].W != nullptr && sx_aligned4(net.layer[l].W) && sx_aligned4(net.layer[l].b),
                   "sx_resnet_flow_bwd: layer %d has no weight, or a pointer that is not 4-byte aligned", l);
        wrapped = wrapped || net.layer[l].sigma_col >= 0;
    }
    SX_REQUIRE(!wrapped || sigma != nullptr, "sx_resnet_flow_bwd: a wrapped network needs its sigma row");
    SX_REQUIRE(x != nullptr && gin != nullptr && gout != nullptr, "sx_resnet_flow_bwd: null x / gin / gout");
    SX_REQUIRE(sx_aligned4(x) && sx_aligned4(s_rows) && sx_aligned4(sigma) && sx_aligned4(gin) && sx_aligned4(gout) && sx_aligned4(gs) &&
               sx_aligned4(partial), "sx_resnet_flow_bwd: every pointer must be 4-byte aligned");
    bool any = false;
    if (grads != nullptr)
        for (int l = 0; l < net.n_layers; ++l) {
            SX_REQUIRE(sx_aligned4(grads->dW[l]) && sx_aligned4(grads->db[l]), "sx_resnet_flow_bwd: gradient %d is not 4-byte aligned", l);
            any = any || grads->dW[l] != nullptr || grads->db[l] != nullptr;
        }
    SX_REQUIRE(!any || n_rows == 0 || partial != nullptr,
               "sx_resnet_flow_bwd: the partial buffer is missing (sx_resnet_bwd_partial_floats)");
    rb_args a{};
    a.net = net;
    int DT, HT;
    const size_t lds = rb_plan(net, a, DT, HT) * 4;
    SX_REQUIRE(lds <= SX_RESNET_LDS_BYTES, "sx_resnet_flow_bwd: the images and scratch need %zu bytes of LDS (budget %d)", lds,
               SX_RESNET_LDS_BYTES);
    tc_reduce_args<2 * SX_RESNET_MAX_LAYERS> r{};              // dW_0, db_0, dW_1, db_1, ...
    int total = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        a.want_w[l] = any && grads->dW[l] != nullptr;
        a.want_b[l] = any && grads->db[l] != nullptr;
        r.e[2 * l] = {any ? grads->dW[l] : nullptr, net.layer[l].out_dim, net.layer[l].in_dim, l == 0 ? DT : HT, a.off_w[l]};
        r.e[2 * l + 1] = {any ? grads->db[l] : nullptr, net.layer[l].out_dim, 0, 0, a.off_b[l]};
        total += net.layer[l].out_dim * (net.layer[l].in_dim + 1);
    }
    r.partial = partial; r.part_floats = a.part_floats;
    int grid = 0;
    if (n_rows > 0) {
        a.any_param = any ? 1 : 0;
        a.x = x; a.s_rows = s_rows; a.sigma = sigma; a.gin = gin; a.gout = gout; a.gs = gs; a.partial = partial;
        a.n_rows = n_rows; a.iterations = iterations; a.inverse = inverse ? 1 : 0;
        const int64_t blocks = rb_blocks(n_rows);
        const int NL = net.n_layers;
        int rc = SX_E_BADARG;
#define RB_CASE(D_, H_, N_) if (DT == D_ && HT == H_ && NL == N_) rc = sx_launch_capped<resnet_bwd_kernel<D_, H_, N_>>("sx_resnet_flow_bwd", a, SX_RESNET_THREADS, lds, SX_RESNET_LDS_BYTES, blocks, stream, &grid);
        RB_CASE(1, 1, 1) RB_CASE(2, 1, 1)
        RB_CASE(1, 1, 2) RB_CASE(1, 2, 2) RB_CASE(2, 1, 2) RB_CASE(2, 2, 2)
        RB_CASE(1, 1, 3) RB_CASE(1, 2, 3) RB_CASE(2, 1, 3) RB_CASE(2, 2, 3)
        RB_CASE(1, 1, 4) RB_CASE(1, 2, 4) RB_CASE(2, 1, 4) RB_CASE(2, 2, 4)
#undef RB_CASE
        if (rc != SX_OK) return rc;
    }
    if (!any) return SX_OK;
    // every wave with a row group wrote its slot: slots 0 .. min(groups, 4 * grid) - 1 (no rows: no slots, the gradients are zero)
    const int64_t n_groups = (n_rows + 31) / 32, n_waves = (int64_t)grid * SX_RESNET_WAVES;
    r.n_slots = (int)(n_groups < n_waves ? n_groups : n_waves);
    return tc_reduce("sx_resnet_flow_bwd", r, total, stream);
}
