// What the two kernel files of the dense DiffeqMLP CNF (sx_cnf.hip: the solve with the exact trace; sx_cnf_train.hip: the Hutchinson
// forward and its adjoint) have in common beyond sx_cnf_common.h -- everything that depends only on an sx_cnf_net and on the LDS
// layout of its forward images, written once, so that the x arithmetic of the two files is one piece of code and sx_cnf_train_fwd's
// y is sx_cnf_flow's by construction:
//   * device: the hidden-layer evaluation and the output layer (macros, which both files expand: see there), the activation sweep;
//     and, as functions that sx_cnf_train.hip alone calls (sx_cnf.hip keeps the same statements inline, see its header), the staging
//     of the forward images, biases and time column and the latent share of the first layer (a state's row load / store is
//     sx_cnf_common.h's cnf_load_row / cnf_store_row);
//   * host: the network validator (the entry point's name and its three limits are arguments), the hidden-tile count and the LDS plan
//     of the forward images, to which each file appends its own parts.
// The flavour of every device function is the one with which all instantiations of both files build without scratch (they sit at the
// edge of the register file): predicated global loads.  One piece comes in two flavours, the activation sweep (cnf_dense_act).
#pragma once
#include "sx_cnf_common.h"

namespace {

// the head of both files' kernel arguments: the network and the LDS float offsets of its forward images
struct cnf_dense_args {
    sx_cnf_net net;
    int base_w[3];          // W1x, W2(, W3)
    int base_b[3];          // the biases
    int base_w0;            // W1[:, 0] (the time column)
};

// (inlined on purpose: an out-of-line call would spill the live stage vectors around it)
template <int ACT>
__device__ __forceinline__ void cnf_dense_act_sweep(f32x16 &v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = cnf_act(v[r], ACT);
}

__device__ __forceinline__ void cnf_dense_act_tile(f32x16 *v, int act) {
#pragma unroll
    for (int r = 0; r < 16; ++r) (*v)[r] = cnf_act((*v)[r], act);
}

// act(v) of T tiles: cnf_act per element in either flavour, so the flavour moves registers and time, not bits.  Each file needs its own:
//   TILE_SWITCH = false (sx_cnf.hip): ReLU as a bare fmaxf loop, otherwise the switch per element.  With one switch per tile
//     cnf_flow_kernel<1, 4, 2> spills (20 bytes of scratch per lane), with cnf_act_all 30 VGPRs (124 bytes);
//   TILE_SWITCH = true (sx_cnf_train.hip): one wave-uniform switch around the unrolled sweeps.  Its one-tile kernels have the
//     registers for it, and with a branch chain per element a training step takes 10 % (dim 2 / [32]) to 18 % (dim 32 / [32, 32])
//     longer: there the activations, not the MFMAs, are most of an evaluation.
template <int T, bool TILE_SWITCH>
__device__ __forceinline__ void cnf_dense_act(cnf_tile<T> &v, int act) {
#pragma unroll
    for (int m = 0; m < T; ++m) {
        if (TILE_SWITCH) {
            switch (act) {
                case SX_ACT_TANH: cnf_dense_act_sweep<SX_ACT_TANH>(v.v[m]); break;
                case SX_ACT_RELU: cnf_dense_act_sweep<SX_ACT_RELU>(v.v[m]); break;
                case SX_ACT_SIGMOID: cnf_dense_act_sweep<SX_ACT_SIGMOID>(v.v[m]); break;
                case SX_ACT_ELU: cnf_dense_act_sweep<SX_ACT_ELU>(v.v[m]); break;
                case SX_ACT_SOFTPLUS: cnf_dense_act_sweep<SX_ACT_SOFTPLUS>(v.v[m]); break;
                case SX_ACT_LEAKYRELU: cnf_dense_act_sweep<SX_ACT_LEAKYRELU>(v.v[m]); break;
                default: break;
            }
        } else if (act == SX_ACT_RELU) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v.v[m][r] = fmaxf(v.v[m][r], 0.f);
        } else if (act != SX_ACT_IDENTITY) {
            cnf_dense_act_tile(&v.v[m], act);
        }
    }
}

// the forward images (layer image of cnf_stage, zero-padded to tiles of 32), the biases and the time column, once per workgroup
template <int DT, int HT, int NH>
__device__ __forceinline__ void cnf_dense_stage(const cnf_dense_args &a) {
    const sx_cnf_net &net = a.net;
    const int D = net.dim, in_dim = 1 + D + net.latent_dim, H1 = net.layer[0].out_dim, Hl = net.layer[NH - 1].out_dim;
    cnf_stage(net.layer[0].W, H1, D, in_dim, 1, HT, DT, a.base_w[0]);
    cnf_stage_vec(net.layer[0].b, H1, 1, HT * 32, a.base_b[0]);
    cnf_stage_vec(net.layer[0].W, H1, in_dim, HT * 32, a.base_w0);
    if (NH == 2) {
        cnf_stage(net.layer[1].W, Hl, H1, H1, 0, HT, HT, a.base_w[1]);
        cnf_stage_vec(net.layer[1].b, Hl, 1, HT * 32, a.base_b[1]);
    }
    cnf_stage(net.layer[NH].W, D, Hl, Hl, 0, DT, HT, a.base_w[NH]);
    cnf_stage_vec(net.layer[NH].b, D, 1, DT * 32, a.base_b[NH]);
}

// the latent share of the first layer: W1[:, 1 + D ..] . latent_row, once per row (its A fragments come straight from global memory:
// once per group, no LDS spent on it).  `staged`: the group's latent rows already in LDS, [32][L], read there instead (every lane
// reads, from an address inside the block)
template <int HT>
__device__ __forceinline__ void cnf_dense_latent(const cnf_dense_args &a, cnf_tile<HT> &lat, const float *latent, int64_t row, bool live, int lane,
                                                 const float *staged = nullptr) {
    const sx_cnf_net &net = a.net;
    const int D = net.dim, L = net.latent_dim, in_dim = 1 + D + L, H1 = net.layer[0].out_dim, h = lane >> 5;
#pragma unroll
    for (int m = 0; m < HT; ++m) lat.v[m] = f32x16{};
    if (L > 0) {
        const float *W1 = net.layer[0].W;
        for (int c = 0; c < (L + 31) >> 5; ++c) {
            f32x16 lb;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * c + sx_kmap(r, h);
                if (staged != nullptr) {
                    const float t = staged[(lane & 31) * L + (f < L ? f : 0)];
                    lb[r] = (live && f < L) ? t : 0.f;
                } else {
                    lb[r] = (live && f < L) ? latent[row * L + f] : 0.f;
                }
            }
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                const int wr = 32 * m + (lane & 31);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int f = 32 * c + sx_kmap(q, h);
                    const float av = (wr < H1 && f < L) ? W1[(int64_t)wr * in_dim + 1 + D + f] : 0.f;
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, lb[q], lat.v[m], 0, 0, 0);
                }
            }
        }
    }
}

// The hidden layers and the output layer are TEXT, not functions, for sx_cnf.hip's sake: cn_eval expands the three macros where it
// had these statements, and so compiles to the code it compiled to before the two files shared them.  Called as functions there
// (cnf_dense_hidden / cnf_dense_out below, with the same statements), cnf_flow_kernel<1, 4, 2> -- 256 + 256 registers -- is allocated
// differently and dim 32 / [128, 128] at 2^18 rows, rk4 x 16, takes 29.18 ms for 29.01 and 18.73 ms for 18.58 (+0.6 %, +0.8 %).
// h = lane >> 5, act = a.net.act; TILE_SWITCH: the caller's flavour of the activation sweep (cnf_dense_act).
// h1 = act(W1x xin + lat + (b1 + t W1[:, 0])).  The fence: the weights in LDS never change, so their loads are loop-invariant, and
// without it the compiler hoists them out of the step loop and holds whole matrices in registers
#define CNF_DENSE_H1(DT, HT, TILE_SWITCH, a, xin, t, lat, h1, lane, h, act)                                                       \
    asm volatile("" ::: "memory");                                                                                                \
    const float *b1 = cnf_smem + (a).base_b[0] + 4 * (h), *w0 = cnf_smem + (a).base_w0 + 4 * (h);                                 \
    cnf_gemm<DT, HT>(xin, h1, cnf_smem + (a).base_w[0] + (lane) * 4);                                                             \
    _Pragma("unroll") for (int m = 0; m < HT; ++m)                                                                                \
        _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                            \
            (h1).v[m][r] = ((h1).v[m][r] + (lat).v[m][r]) + (cnf_vec(b1, m, r) + (t) * cnf_vec(w0, m, r));                        \
    cnf_dense_act<HT, TILE_SWITCH>(h1, act)
// h2 = act(W2 h1 + b2)
#define CNF_DENSE_H2(HT, TILE_SWITCH, a, h1, h2, lane, h, act)                                                                    \
    cnf_gemm<HT, HT>(h1, h2, cnf_smem + (a).base_w[1] + (lane) * 4);                                                              \
    const float *b2 = cnf_smem + (a).base_b[1] + 4 * (h);                                                                         \
    _Pragma("unroll") for (int m = 0; m < HT; ++m)                                                                                \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) (h2).v[m][r] += cnf_vec(b2, m, r);                                         \
    cnf_dense_act<HT, TILE_SWITCH>(h2, act)
// k = W_last h_last + b_last (NH: hidden layers; the caller fences before it)
#define CNF_DENSE_OUT(DT, HT, NH, a, hl, k, lane, h)                                                                              \
    cnf_gemm<HT, DT>(hl, k, cnf_smem + (a).base_w[NH] + (lane) * 4);                                                              \
    const float *bl = cnf_smem + (a).base_b[NH] + 4 * (h);                                                                        \
    _Pragma("unroll") for (int m = 0; m < DT; ++m)                                                                                \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) (k).v[m][r] += cnf_vec(bl, m, r)

// the same as functions (sx_cnf_train.hip): the hidden activations at (t, xin), h2 with two hidden layers; k from the last of them
template <int DT, int HT, int NH, bool TILE_SWITCH>
__device__ __forceinline__ void cnf_dense_hidden(const cnf_dense_args &a, const cnf_tile<DT> &xin, float t, const cnf_tile<HT> &lat,
                                                 cnf_tile<HT> &h1, cnf_tile<HT> &h2, int lane) {
    const int h = lane >> 5, act = a.net.act;
    CNF_DENSE_H1(DT, HT, TILE_SWITCH, a, xin, t, lat, h1, lane, h, act);
    if (NH == 2) {
        CNF_DENSE_H2(HT, TILE_SWITCH, a, h1, h2, lane, h, act);
    }
}

template <int DT, int HT, int NH>
__device__ __forceinline__ void cnf_dense_out(const cnf_dense_args &a, const cnf_tile<HT> &hl, cnf_tile<DT> &k, int lane) {
    asm volatile("" ::: "memory");
    CNF_DENSE_OUT(DT, HT, NH, a, hl, k, lane, lane >> 5);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// `fn`: the prefix of the messages; the limits: dim, 1 + dim + latent_dim, the width of a hidden layer
inline int cnf_dense_check_net(const char *fn, const sx_cnf_net *net_host, int max_dim, int max_in, int max_hidden) {
    SX_REQUIRE(net_host != nullptr, "%s: null network", fn);
    const sx_cnf_net &net = *net_host;
    SX_REQUIRE(net.n_layers == 2 || net.n_layers == 3, "%s: one or two hidden layers (got %d Linear layers)", fn, net.n_layers);
    SX_REQUIRE(net.dim >= 1 && net.dim <= max_dim, "%s: dim must be in 1..%d (got %d)", fn, max_dim, net.dim);
    SX_REQUIRE(net.latent_dim >= 0 && 1 + net.dim + net.latent_dim <= max_in, "%s: 1 + dim + latent_dim must be <= %d", fn, max_in);
    SX_REQUIRE(net.act >= SX_ACT_IDENTITY && net.act <= SX_ACT_LEAKYRELU, "%s: activation %d has no in-kernel derivative", fn, net.act);
    for (int l = 0; l < net.n_layers; ++l) {
        const sx_cnf_layer &L = net.layer[l];
        SX_REQUIRE(L.W != nullptr, "%s: layer %d has no weight", fn, l);
        SX_REQUIRE(L.in_dim == (l == 0 ? 1 + net.dim + net.latent_dim : net.layer[l - 1].out_dim), "%s: layer %d input width", fn, l);
        SX_REQUIRE(L.out_dim >= 1 && L.out_dim <= max_hidden, "%s: layer %d width must be in 1..%d", fn, l, max_hidden);
    }
    SX_REQUIRE(net.layer[net.n_layers - 1].out_dim == net.dim, "%s: the last layer must map back to dim", fn);
    return SX_OK;
}

// tiles of the widest hidden layer
inline int cnf_dense_hidden_tiles(const sx_cnf_net &net) {
    int HT = 1;
    for (int l = 0; l + 1 < net.n_layers; ++l) HT = cnf_tiles(net.layer[l].out_dim) > HT ? cnf_tiles(net.layer[l].out_dim) : HT;
    return HT;
}

// the LDS plan of the forward images: float offsets into `a`, -> floats used (a file's own parts follow from there)
inline size_t cnf_dense_plan(const sx_cnf_net &net, cnf_dense_args &a) {
    const int DT = cnf_tiles(net.dim), NH = net.n_layers - 1, HT = cnf_dense_hidden_tiles(net);
    size_t off = 0;
    for (int l = 0; l <= NH; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == NH ? DT : HT;
        a.base_w[l] = (int)off; off += (size_t)MT * KT * 1024;
        a.base_b[l] = (int)off; off += (size_t)MT * 32;
    }
    a.base_w0 = (int)off; off += (size_t)HT * 32;
    return off;
}

}  // namespace
