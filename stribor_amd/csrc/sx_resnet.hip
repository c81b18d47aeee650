// Invertible ResNet flows (IResNet / ContinuousIResNet, stribor/flows/iresnet.py:9-99) in one launch per call.
//
// sx_resnet_flow -- the map y = x + s (.) g(x) and its fixed-point inverse x <- y - s (.) g(x) (iresnet.py:38-44, 84-90),
// g = the spectral-normalised MLP of net/mlp.py:6-65, s = 1 (IResNet) or the time embedding time_net(t) (ContinuousIResNet):
//   * one wave = 32 rows.  Rows sit on the MFMA column (lane & 31), features on the C rows: a 32-feature tile of a row's
//     state is one f32x16 C fragment (lane half h owns features sx_kmap(r, h), r = 0..15), and a C tile is directly the
//     B operand of the next layer's GEMM (k-step r <-> feature sx_kmap(r, h); the A fragments are staged in that order).
//     So x -> hidden -> ... -> g(x) -> x' never leaves registers, for all `iterations` steps;
//   * every layer's weights (the UNNORMALISED weight_orig of a wrapped layer) are staged into LDS once per workgroup, in
//     A-fragment order, zero-padded to 32-wide tiles; the workgroup then walks its 32-row groups (grid-stride, one group
//     per wave at a time).  HBM sees the input rows (+ t) once and the output rows once;
//   * spectral normalisation: iteration k scales the output of wrapped layer j by 1 / sigma[k][j] before its bias
//     (W_orig h / sigma == (W_orig / sigma) h up to rounding); sx_spectral_sigma fills the table -- one row per hook call
//     the reference makes (training), or one row (eval / a single call);
//   * arithmetic: exact fp32 everywhere, v_mfma_f32_32x32x2_f32 for the GEMMs (an fma chain; no operand range), fp32-grade
//     library tanhf / expf / sinf / logf for the activations and time nets.  A map iterated 100 times should not inherit
//     the fp16 x 3 split's operand range rules, so this kernel ignores set_gemm_precision (fp16 x 3 is not offered here);
//   * time embedding (kinds 0-4: TimeIdentity / Linear / Tanh / Log / Fourier[Bounded], net/time_net.py) evaluated once
//     per row before the loop; any other time net is evaluated by the caller and passed as [n_rows, dim] rows (kind 5).
//
// Coverage: dim <= 128, up to three hidden layers of <= 128 units (hidden_dims = [] too), any SX_ACT_* activation and
// final activation; feature counts are padded to 1, 2 or 4 tiles of 32 and the padded weights + biases must fit
// SX_RESNET_LDS_BYTES (e.g. dim 64 with [64, 64]: 49.5 KiB; dim 128 with [128]: 129 KiB; dim 128 with [128, 128]: no).
//
// sx_spectral_sigma -- torch.nn.utils.spectral_norm's compute_weight (torch/nn/utils/spectral_norm.py) for every wrapped
// layer of one network, for `n_calls` consecutive calls, in one launch (one workgroup per layer): per call n_power rounds
// of v = normalize(W^T u), u = normalize(W v) (normalize(a) = a / max(|a|, eps)), then sigma = u . (W v); u and v are
// written back in place at the end.
#include "sx_resnet_common.h"

namespace {

struct rn_args {
    sx_resnet_net net;
    int base[SX_RESNET_MAX_LAYERS];    // LDS float offset of each layer's image
    const float *in;
    float *out;
    int64_t n_rows;
    const float *t;
    const float *s_rows;
    const float *time_a;
    const float *time_b;
    const float *sigma;
    int time_kind, time_hidden, sigma_rows, iterations, inverse, lds_floats;
};

// the per-iteration scale of layer l: 1 / sigma[k][col] of a wrapped layer, 1 otherwise
__device__ __forceinline__ float rn_scale(const rn_args &a, int l, int k) {
    const int col = a.net.layer[l].sigma_col;
    if (col < 0) return 1.f;
    const int row = a.sigma_rows == 1 ? 0 : k;
    return 1.f / a.sigma[(int64_t)row * a.net.n_wrapped + col];
}

// s_f of row `row` (net/time_net.py:11, 20, 30, 38, 74-79): once per row, out of line
__device__ __attribute__((noinline)) float rn_time(const rn_args &a, int64_t row, int f, float tv) {
    switch (a.time_kind) {
        case SX_RESNET_TIME_IDENTITY: return tv;
        case SX_RESNET_TIME_LINEAR: return a.time_a[f] * tv;
        case SX_RESNET_TIME_TANH: return tanhf(a.time_a[f] * tv);
        case SX_RESNET_TIME_LOG: return logf(expf(a.time_a[f]) * tv + 1.f);
        case SX_RESNET_TIME_FOURIER: {
            float acc = 0.f;
            for (int q = 0; q < a.time_hidden; ++q) acc += a.time_a[f * a.time_hidden + q] * sinf(a.time_b[f * a.time_hidden + q] * tv);
            return acc;
        }
        default: return a.s_rows[row * a.net.dim + f];
    }
}

template <int DT, int HT>
__global__ __launch_bounds__(SX_RESNET_THREADS) void resnet_flow_kernel(const rn_args a) {
    const int nl = a.net.n_layers;
    for (int l = 0; l < nl; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == nl - 1 ? DT : HT;
        rn_stage_layer(a.net.layer[l].W, a.net.layer[l].b, a.net.layer[l].out_dim, a.net.layer[l].in_dim, MT, KT, a.base[l]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, D = a.net.dim;
    const int act = a.net.act, fact = a.net.final_act;
    const int64_t n_groups = (a.n_rows + 31) >> 5;
    for (int64_t grp = (int64_t)blockIdx.x * SX_RESNET_WAVES + (threadIdx.x >> 6); grp < n_groups;
         grp += (int64_t)gridDim.x * SX_RESNET_WAVES) {
        const int64_t row = grp * 32 + (lane & 31);
        const bool live = row < a.n_rows;
        const float tv = (live && a.t != nullptr) ? a.t[row] : 0.f;
        rtile<DT> y, x, s;
#pragma unroll
        for (int c = 0; c < DT; ++c) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * c + sx_kmap(r, h);
                const bool ok = live && f < D;
                y.v[c][r] = ok ? a.in[row * D + f] : 0.f;
                s.v[c][r] = !ok ? 0.f : a.time_kind == SX_RESNET_TIME_NONE ? 1.f : rn_time(a, row, f, tv);
            }
            x.v[c] = y.v[c];
        }
        const int iters = a.inverse ? a.iterations : 1;
        for (int k = 0; k < iters; ++k) {
            rtile<DT> g;
            if (nl == 1) {
                rn_layer<DT, DT>(x, g, a.base[0], rn_scale(a, 0, k), fact, lane);
            } else {
                rtile<HT> hA, hB;
                rn_layer<DT, HT>(x, hA, a.base[0], rn_scale(a, 0, k), act, lane);
                if (nl >= 3) rn_layer<HT, HT>(hA, hB, a.base[1], rn_scale(a, 1, k), act, lane);
                if (nl >= 4) rn_layer<HT, HT>(hB, hA, a.base[2], rn_scale(a, 2, k), act, lane);
                if (nl == 3) rn_layer<HT, DT>(hB, g, a.base[nl - 1], rn_scale(a, nl - 1, k), fact, lane);
                else rn_layer<HT, DT>(hA, g, a.base[nl - 1], rn_scale(a, nl - 1, k), fact, lane);
            }
            // iresnet.py:39 (x + net(x)), :43 (y - net(x)), :81 / :88 with time_net(t) * net(x): the product is rounded first
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sg = __fmul_rn(s.v[c][r], g.v[c][r]);
                    x.v[c][r] = a.inverse ? __fsub_rn(y.v[c][r], sg) : __fadd_rn(y.v[c][r], sg);
                }
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < DT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * c + sx_kmap(r, h);
                    if (f < D) a.out[row * D + f] = x.v[c][r];
                }
        }
    }
}

// ---- spectral norm ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sn_block_sum(float v, float *red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                   // red[] of the previous sum has been read by every thread
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(SX_RESNET_THREADS) void spectral_sigma_kernel(const sx_sn_job job, int n_calls, float *sigma) {
    const sx_sn_layer L = job.layer[blockIdx.x];
    const int M = L.out_dim, K = L.in_dim, KP = K + 1, tid = threadIdx.x;
    float *W = rn_smem;                    // [M][K + 1]: the odd row stride keeps W v's column walk free of bank conflicts
    float *u = W + M * KP, *v = u + M, *red = v + K;
    for (int e = tid; e < M * K; e += SX_RESNET_THREADS) W[(e / K) * KP + e % K] = L.W[e];
    for (int i = tid; i < M; i += SX_RESNET_THREADS) u[i] = L.u[i];
    for (int j = tid; j < K; j += SX_RESNET_THREADS) v[j] = L.v[j];
    __syncthreads();
    for (int call = 0; call < n_calls; ++call) {
        for (int it = 0; it < L.n_power; ++it) {
            // v = normalize(W^T u)
            float a = 0.f;
            if (tid < K)
                for (int i = 0; i < M; ++i) a = fmaf(W[i * KP + tid], u[i], a);
            float nrm = sqrtf(sn_block_sum(tid < K ? a * a : 0.f, red));
            if (tid < K) v[tid] = a / fmaxf(nrm, L.eps);
            __syncthreads();
            // u = normalize(W v)
            a = 0.f;
            if (tid < M)
                for (int j = 0; j < K; ++j) a = fmaf(W[tid * KP + j], v[j], a);
            nrm = sqrtf(sn_block_sum(tid < M ? a * a : 0.f, red));
            if (tid < M) u[tid] = a / fmaxf(nrm, L.eps);
            __syncthreads();
        }
        // sigma = u . (W v)
        float a = 0.f;
        if (tid < M)
            for (int j = 0; j < K; ++j) a = fmaf(W[tid * KP + j], v[j], a);
        const float sg = sn_block_sum(tid < M ? u[tid] * a : 0.f, red);
        if (tid == 0) sigma[(int64_t)call * job.n_layers + blockIdx.x] = sg;
    }
    if (L.n_power > 0 && n_calls > 0) {
        for (int i = tid; i < M; i += SX_RESNET_THREADS) L.u[i] = u[i];
        for (int j = tid; j < K; j += SX_RESNET_THREADS) L.v[j] = v[j];
    }
}

inline int rn_tiles(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : 4; }

}  // namespace

extern "C" size_t sx_resnet_lds_bytes(const sx_resnet_net *net_host) {
    if (!net_host || net_host->n_layers < 1 || net_host->n_layers > SX_RESNET_MAX_LAYERS) return 0;
    const int DT = rn_tiles(net_host->dim);
    int HT = 1;
    for (int l = 0; l + 1 < net_host->n_layers; ++l) {
        const int t = rn_tiles(net_host->layer[l].out_dim);
        HT = t > HT ? t : HT;
    }
    size_t floats = 0;
    for (int l = 0; l < net_host->n_layers; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == net_host->n_layers - 1 ? DT : HT;
        floats += (size_t)MT * KT * 1024 + (size_t)MT * 32;
    }
    return floats * 4;
}

extern "C" int sx_resnet_flow(const sx_resnet_net *net_host, const float *in, float *out, int64_t n_rows, const float *t,
                              const float *s_rows, int32_t time_kind, const float *time_a, const float *time_b,
                              int32_t time_hidden, const float *sigma, int32_t sigma_rows, int32_t iterations, int32_t inverse,
                              void *stream) {
    SX_REQUIRE(net_host != nullptr, "sx_resnet_flow: null network");
    const sx_resnet_net &net = *net_host;
    SX_REQUIRE(net.n_layers >= 1 && net.n_layers <= SX_RESNET_MAX_LAYERS, "sx_resnet_flow: 1..%d Linear layers (got %d)",
               SX_RESNET_MAX_LAYERS, net.n_layers);
    SX_REQUIRE(net.dim >= 1 && net.dim <= 128, "sx_resnet_flow: dim must be in 1..128 (got %d)", net.dim);
    SX_REQUIRE(n_rows >= 0 && iterations >= 0, "sx_resnet_flow: negative n_rows / iterations");
    SX_REQUIRE(net.act >= 0 && net.act <= SX_ACT_GELU && net.final_act >= 0 && net.final_act <= SX_ACT_GELU,
               "sx_resnet_flow: unknown activation code");
    for (int l = 0; l < net.n_layers; ++l) {
        const sx_resnet_layer &L = net.layer[l];
        SX_REQUIRE(L.W != nullptr, "sx_resnet_flow: layer %d has no weight", l);
        SX_REQUIRE(L.in_dim == (l == 0 ? net.dim : net.layer[l - 1].out_dim), "sx_resnet_flow: layer %d input width", l);
        SX_REQUIRE(L.out_dim >= 1 && L.out_dim <= 128, "sx_resnet_flow: layer %d width must be in 1..128", l);
        SX_REQUIRE(L.sigma_col < net.n_wrapped, "sx_resnet_flow: layer %d sigma column out of range", l);
    }
    SX_REQUIRE(net.layer[net.n_layers - 1].out_dim == net.dim, "sx_resnet_flow: the last layer must map back to dim");
    const bool wrapped = net.n_wrapped > 0;
    SX_REQUIRE(!wrapped || (sigma != nullptr && (sigma_rows == 1 || sigma_rows >= (inverse ? iterations : 1))),
               "sx_resnet_flow: sigma table needs 1 or `iterations` rows");
    SX_REQUIRE(time_kind >= SX_RESNET_TIME_NONE && time_kind <= SX_RESNET_TIME_ROWS, "sx_resnet_flow: unknown time kind %d", time_kind);
    SX_REQUIRE(time_kind == SX_RESNET_TIME_NONE || time_kind == SX_RESNET_TIME_ROWS || t != nullptr, "sx_resnet_flow: t missing");
    SX_REQUIRE(time_kind <= SX_RESNET_TIME_IDENTITY || time_kind == SX_RESNET_TIME_ROWS || time_a != nullptr,
               "sx_resnet_flow: time net parameters missing");
    SX_REQUIRE(time_kind != SX_RESNET_TIME_FOURIER || (time_b != nullptr && time_hidden >= 1), "sx_resnet_flow: Fourier shift missing");
    SX_REQUIRE(time_kind != SX_RESNET_TIME_ROWS || s_rows != nullptr, "sx_resnet_flow: s rows missing");
    SX_REQUIRE(in != nullptr && out != nullptr, "sx_resnet_flow: null input / output");
    const size_t lds = sx_resnet_lds_bytes(net_host);
    SX_REQUIRE(lds <= SX_RESNET_LDS_BYTES, "sx_resnet_flow: the padded weights need %zu bytes of LDS (budget %d)", lds,
               SX_RESNET_LDS_BYTES);
    if (n_rows == 0) return SX_OK;
    rn_args a{};
    a.net = net;
    const int DT = rn_tiles(net.dim);
    int HT = 1;
    for (int l = 0; l + 1 < net.n_layers; ++l) HT = rn_tiles(net.layer[l].out_dim) > HT ? rn_tiles(net.layer[l].out_dim) : HT;
    int off = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        const int KT = l == 0 ? DT : HT, MT = l == net.n_layers - 1 ? DT : HT;
        a.base[l] = off;
        off += MT * KT * 1024 + MT * 32;
    }
    a.in = in; a.out = out; a.n_rows = n_rows; a.t = t; a.s_rows = s_rows; a.time_a = time_a; a.time_b = time_b;
    a.sigma = sigma; a.time_kind = time_kind; a.time_hidden = time_hidden; a.sigma_rows = sigma_rows;
    a.iterations = iterations; a.inverse = inverse ? 1 : 0; a.lds_floats = off;
    const int64_t want = ((n_rows + 31) / 32 + SX_RESNET_WAVES - 1) / SX_RESNET_WAVES;
#define RN_CASE(D_, H_) if (DT == D_ && HT == H_) return sx_launch_capped<resnet_flow_kernel<D_, H_>>("sx_resnet_flow", a, SX_RESNET_THREADS, lds, SX_RESNET_LDS_BYTES, want, stream);
    RN_CASE(1, 1) RN_CASE(1, 2) RN_CASE(1, 4) RN_CASE(2, 1) RN_CASE(2, 2) RN_CASE(2, 4) RN_CASE(4, 1) RN_CASE(4, 2) RN_CASE(4, 4)
#undef RN_CASE
    sx_set_error("sx_resnet_flow: no kernel for %d x %d tiles", DT, HT);
    return SX_E_BADARG;
}

extern "C" int sx_spectral_sigma(const sx_sn_job *job_host, int32_t n_calls, float *sigma, void *stream) {
    SX_REQUIRE(job_host != nullptr && sigma != nullptr, "sx_spectral_sigma: null argument");
    const sx_sn_job &job = *job_host;
    SX_REQUIRE(job.n_layers >= 1 && job.n_layers <= SX_RESNET_MAX_LAYERS, "sx_spectral_sigma: 1..%d layers", SX_RESNET_MAX_LAYERS);
    SX_REQUIRE(n_calls >= 1, "sx_spectral_sigma: n_calls must be >= 1");
    int max_floats = 0;
    for (int l = 0; l < job.n_layers; ++l) {
        const sx_sn_layer &L = job.layer[l];
        SX_REQUIRE(L.W && L.u && L.v, "sx_spectral_sigma: layer %d has a null pointer", l);
        SX_REQUIRE(L.out_dim >= 1 && L.out_dim <= 128 && L.in_dim >= 1 && L.in_dim <= 128,
                   "sx_spectral_sigma: layer %d must be at most 128 x 128", l);
        SX_REQUIRE(L.n_power >= 0, "sx_spectral_sigma: negative power iteration count");
        const int f = L.out_dim * (L.in_dim + 1) + L.out_dim + L.in_dim + 4;
        max_floats = f > max_floats ? f : max_floats;
    }
    const size_t lds = (size_t)max_floats * 4;
    static bool raised_on[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds > 48 * 1024 && !raised_on[dev & 63]) {
        hipError_t e = hipFuncSetAttribute((const void *)spectral_sigma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
        raised_on[dev & 63] = true;
    }
    hipLaunchKernelGGL(spectral_sigma_kernel, dim3(job.n_layers), dim3(SX_RESNET_THREADS), lds, sx_stream(stream), job, (int)n_calls, sigma);
    SX_LAUNCH_CHECK();
    return SX_OK;
}
