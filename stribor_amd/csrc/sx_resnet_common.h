// What the ResNet-flow kernels share (sx_resnet.hip: the map and its fixed-point inverse; sx_resnet_bwd.hip: their backward):
// the wave layout -- 32 rows on the MFMA column, features on the C rows in sx_kmap order (sx_common.h) --, the activations, the LDS
// image of a layer in A-fragment order and the layer itself on exact fp32 v_mfma_f32_32x32x2_f32.  Both launch through sx_common.h's
// sx_launch_capped; the backward's weight-gradient contraction is sx_train_contract.h's.
#pragma once
#include "sx_common.h"

#define SX_RESNET_WAVES 4
#define SX_RESNET_THREADS (SX_RESNET_WAVES * 64)

namespace {

extern __shared__ __attribute__((aligned(16))) float rn_smem[];

__device__ __forceinline__ float rn_act(float v, int act) {
    switch (act) {
        case SX_ACT_TANH: return tanhf(v);
        case SX_ACT_RELU: return fmaxf(v, 0.f);
        case SX_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        case SX_ACT_ELU: return v > 0.f ? v : expm1f(v);
        case SX_ACT_SOFTPLUS: return v > 20.f ? v : log1pf(expf(v));
        case SX_ACT_LEAKYRELU: return v > 0.f ? v : 0.01f * v;
        case SX_ACT_SILU: return v / (1.f + expf(-v));
        case SX_ACT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
        default: return v;
    }
}

// activations other than ReLU / identity are rare in the hot loop: one out-of-line copy keeps the code (and the compile) small
__device__ __attribute__((noinline)) void rn_act_tile(f32x16 *v, int act) {
    f32x16 t = *v;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = rn_act(t[r], act);
    *v = t;
}

template <int T>
struct rtile {
    f32x16 v[T];
};

// LDS image of one layer: MT x KT A-operand tiles of 1024 floats (tile (m, c), float g*256 + lane*4 + j holds
// W[32m + (lane & 31)][32c + kmap(4g + j, lane >> 5)]), then MT*32 biases.
__device__ __forceinline__ void rn_stage_layer(const float *__restrict__ W, const float *__restrict__ b, int out_dim, int in_dim,
                                               int MT, int KT, int base) {
    const int n_w = MT * KT * 1024;
    for (int e = threadIdx.x; e < n_w; e += SX_RESNET_THREADS) {
        const int tile = e >> 10, rem = e & 1023;
        const int g = rem >> 8, lane = (rem >> 2) & 63, j = rem & 3;
        const int m = tile / KT, c = tile - m * KT;
        const int row = 32 * m + (lane & 31), col = 32 * c + sx_kmap(4 * g + j, lane >> 5);
        rn_smem[base + e] = (row < out_dim && col < in_dim) ? W[(int64_t)row * in_dim + col] : 0.f;
    }
    for (int i = threadIdx.x; i < MT * 32; i += SX_RESNET_THREADS)
        rn_smem[base + n_w + i] = (b != nullptr && i < out_dim) ? b[i] : 0.f;
}

// out[m] = act((W . in)[m] * scale + bias[m]), m < MT; W: the layer image at float offset `base` (KT input tiles)
template <int KT, int MT>
__device__ __forceinline__ void rn_layer(const rtile<KT> &in, rtile<MT> &out, int base, float scale, int act, int lane) {
    const float *wb = rn_smem + base + lane * 4;
    const float *bb = rn_smem + base + MT * KT * 1024 + 4 * (lane >> 5);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        f32x16 acc = {};
#pragma unroll
        for (int c = 0; c < KT; ++c) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(wb + (m * KT + c) * 1024 + g * 256);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, in.v[c][4 * g + 0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, in.v[c][4 * g + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, in.v[c][4 * g + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, in.v[c][4 * g + 3], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] * scale + bb[32 * m + 8 * (r >> 2) + (r & 3)];
        if (act == SX_ACT_RELU) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.f);
        } else if (act != SX_ACT_IDENTITY) {
            rn_act_tile(&acc, act);
        }
        out.v[m] = acc;
    }
}

}  // namespace
