// Multi-head attention core of stribor's attention nets (stribor/net/attention.py:8-49, util/safe_softmax.py:3-14), flash-style:
// no [Nq, Nk] score tile ever reaches HBM.
//
// sx_attention_fwd -- one workgroup = W waves (W = 1..4) = 32 W queries of one (batch row r, head); each wave owns 32 queries and
// walks the key / value tiles of 32 keys with an online (running max, running sum) softmax:
//   * swapped Q K^T: S^T = K Q^T on v_mfma_f32_32x32x2_f32 (A = the K tile from LDS, B = the wave's queries, held in registers for
//     the whole walk), so a lane owns ONE query (lane & 31) and 16 of the tile's 32 keys (sx_kmap(r, lane >> 5)) -- the row max
//     and row sum are 15 in-lane ops + one swap with lane ^ 32, no serial-lane softmax;
//   * the probability tile P^T is, register for register, the B operand of O^T += V^T P^T (k-step r <-> key sx_kmap(r, h)),
//     so P never leaves registers either; O^T accumulates in up to four 32 x 32 tiles (dh <= 128);
//   * the contraction over d splits the head into two halves of HALF features, one per lane half (k-step s of lane half h <->
//     feature h HALF + s); HALF = 4, 8, 16, 32 or 64 is a template parameter (dh <= 2 HALF, zero-padded), so every LDS address
//     of the inner loops is a base plus an immediate;
//   * masking (attention.py:35-41): a key is masked iff mask != 1 ((1 - mask).bool()), mask_diagonal drops key == query; a score of
//     -inf contributes exactly 0, and a query whose keys are all masked gets an output of exactly 0 (safe_softmax.py:12-13:
//     nan_to_num of the all-NaN row) and a log-sum-exp of +inf (so the backward's recomputed P is 0 there, too);
//   * when Nq == Nk the output row is multiplied by the raw mask value of its query (attention.py:47-48);
//   * one log-sum-exp per (r, head, query) is written for the backward.
// sx_attention_bwd -- two launches, no float atomics (bit-reproducible): a query-owner pass (layout of the forward) recomputes
// P^T from the saved log-sum-exp and accumulates dq, and writes D = rowsum(dy o y) per query; then a key-owner pass (S with the
// key on the lane, K and V of the wave's 32 keys in registers) walks all query tiles and accumulates dk and dv.
//   dS = P o (dP - D), dP = dy_att V^T, dy_att = dy (* mask of the query when Nq == Nk).
//
// Arithmetic: exact fp32 -- every product is a v_mfma_f32_32x32x2_f32 fma chain (no operand range, no fp16 x 3 split; the
// attention core ignores set_gemm_precision), v_exp_f32 / v_log_f32 for the softmax.
#include "sx_common.h"

#define SX_ATT_MAX_WAVES 4

namespace {

extern __shared__ __attribute__((aligned(16))) float at_smem[];

struct at_args {
    sx_attention_args p;
    const float *y, *dy;
    float *out, *lse, *dq, *dk, *dv, *delta;
    float scale;
    int dh, n_qblk, n_kblk;
};

__device__ __forceinline__ bool at_key_live(const sx_attention_args &p, int64_t r, int key) {
    return key < p.Nk && (p.mask == nullptr || p.mask[r * p.mask_bs + key] == 1.f);
}

// rows row0 .. row0 + 31 of head `head` of a [R, N, E] tensor into an LDS tile [32][WS] (rows >= n and features >= dh stay 0 / are
// zeroed); `mrow`: multiply row i by mrow[r * mask_bs + row0 + i] (NULL: no scaling)
__device__ __forceinline__ void at_stage(float *dst, int WS, const float *src, int64_t bs, int64_t rs, int64_t r, int row0, int n,
                                         int head, int dh, const float *mrow, int64_t mask_bs) {
    for (int e = threadIdx.x; e < 32 * dh; e += blockDim.x) {
        const int i = e / dh, d = e - i * dh;
        const int row = row0 + i;
        float v = 0.f;
        if (row < n) {
            v = src[r * bs + (int64_t)row * rs + (int64_t)head * dh + d];
            if (mrow != nullptr) v *= mrow[r * mask_bs + row];
        }
        dst[i * WS + d] = v;
    }
}

// the lane's half of one row of a head as B-operand registers: b[s] = row[h HALF + s]
template <int HALF>
__device__ __forceinline__ void at_load_half(float (&b)[HALF], const float *row, bool live, int h, int dh) {
#pragma unroll
    for (int s = 0; s < HALF; ++s) {
        const int d = h * HALF + s;
        b[s] = (live && d < dh) ? row[d] : 0.f;
    }
}

// acc = A B over the head's features: A lane (c, h) = tile[c][h HALF + s] from LDS, B = b[s]
template <int HALF>
__device__ __forceinline__ f32x16 at_dot_tile(const float *tile, int WS, const float (&b)[HALF], int c, int h) {
    f32x16 acc = {};
    const float *ap = tile + c * WS + h * HALF;
#pragma unroll
    for (int s = 0; s < HALF; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[s], b[s], acc, 0, 0, 0);
    return acc;
}

// acc[t] += tile^T x for the d tiles t: A lane (c, h) of k-step r = tile[sx_kmap(r, h)][32 t + c], B = x[r]
template <int DT>
__device__ __forceinline__ void at_acc_tiles(f32x16 (&acc)[DT], const float *tile, int WS, const f32x16 &x, int c, int h, int dh) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        if (32 * t >= dh) break;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[sx_kmap(r, h) * WS + 32 * t + c], x[r], acc[t], 0, 0, 0);
    }
}

// out[row][head dh + d] = acc[t][r] * f for d = 32 t + sx_kmap(r, h) < dh (the lane's column is `row`)
template <int DT>
__device__ __forceinline__ void at_store_tiles(float *out, int64_t row, int E, int head, int dh, const f32x16 (&acc)[DT], int h,
                                               float f) {
    float *o = out + row * E + (int64_t)head * dh;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * t + sx_kmap(r, h);
            if (d < dh) o[d] = acc[t][r] * f;
        }
}

__device__ __forceinline__ void at_zero_lds(int n_floats) {
    for (int e = threadIdx.x; e < n_floats; e += blockDim.x) at_smem[e] = 0.f;
    __syncthreads();
}

// ---- forward, and the query-owner pass of the backward (BWD: dq and D) ----------------------------------------------------
template <int HALF, bool BWD>
__global__ __launch_bounds__(SX_ATT_MAX_WAVES * 64) void attention_q_kernel(const at_args a) {
    constexpr int DT = (2 * HALF + 31) / 32, WS = 32 * DT + 1;
    const sx_attention_args &p = a.p;
    float *Ks = at_smem, *Vs = Ks + 32 * WS, *kb = Vs + 32 * WS;
    at_zero_lds(64 * WS);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5, W = blockDim.x >> 6;
    const int H = p.n_heads, E = p.E, dh = a.dh;
    const int64_t n_units = p.R * H * a.n_qblk;
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int qblk = (int)(unit % a.n_qblk);
        const int64_t rh = unit / a.n_qblk;
        const int head = (int)(rh % H);
        const int64_t r = rh / H;
        const int q0 = (qblk * W + (threadIdx.x >> 6)) * 32, qi = q0 + c;
        const bool qlive = qi < p.Nq;
        const bool wave_live = q0 < p.Nq;
        const int64_t qrow = r * p.Nq + qi;                       // row of out / lse / dy / dq
        const float mo = (p.out_mask && qlive) ? p.mask[r * p.mask_bs + qi] : 1.f;
        float qb[HALF];
        at_load_half<HALF>(qb, p.q + r * p.q_bs + (int64_t)qi * p.q_rs + (int64_t)head * dh, qlive, h, dh);
        float gb[BWD ? HALF : 1];
        float lse_q = 0.f, dlt = 0.f;
        if constexpr (BWD) {
            // D = rowsum(dy_att o y_att) = rowsum(dy o y): y = y_att * mask of the query
            float yb[HALF];
            at_load_half<HALF>(gb, a.dy + qrow * E + (int64_t)head * dh, qlive, h, dh);
            at_load_half<HALF>(yb, a.y + qrow * E + (int64_t)head * dh, qlive, h, dh);
#pragma unroll
            for (int s = 0; s < HALF; ++s) dlt = fmaf(gb[s], yb[s], dlt);
            dlt += __shfl_xor(dlt, 32, 64);
#pragma unroll
            for (int s = 0; s < HALF; ++s) gb[s] *= mo;
            lse_q = qlive ? a.lse[(r * H + head) * p.Nq + qi] : INFINITY;
        }
        f32x16 acc[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) acc[t] = f32x16{};
        float m = -INFINITY, l = 0.f;
        for (int k0 = 0; k0 < p.Nk; k0 += 32) {
            __syncthreads();                                      // every wave is done with the previous tile
            at_stage(Ks, WS, p.k, p.k_bs, p.k_rs, r, k0, p.Nk, head, dh, nullptr, 0);
            at_stage(Vs, WS, p.v, p.v_bs, p.v_rs, r, k0, p.Nk, head, dh, nullptr, 0);
            if (threadIdx.x < 32) kb[threadIdx.x] = at_key_live(p, r, k0 + (int)threadIdx.x) ? 0.f : -INFINITY;
            __syncthreads();
            if (!wave_live) continue;
            f32x16 s = at_dot_tile<HALF>(Ks, WS, qb, c, h);      // S^T[key sx_kmap(j, h)][query c]
            if constexpr (!BWD) {
                float tmax = -INFINITY;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int key = sx_kmap(j, h);
                    float v = s[j] * a.scale + kb[key];
                    if (p.mask_diagonal && k0 + key == qi) v = -INFINITY;
                    s[j] = v;
                    tmax = fmaxf(tmax, v);
                }
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
                const float m_new = fmaxf(m, tmax);
                const float m_use = m_new == -INFINITY ? 0.f : m_new;   // all masked so far: every p is exp(-inf) = 0
                const float alpha = __expf(m - m_use);
                float ps = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s[j] = __expf(s[j] - m_use);
                    ps += s[j];
                }
                ps += __shfl_xor(ps, 32, 64);
                l = l * alpha + ps;
                m = m_new;
#pragma unroll
                for (int t = 0; t < DT; ++t) acc[t] *= alpha;
                at_acc_tiles<DT>(acc, Vs, WS, s, c, h, dh);           // O^T += V^T P^T
            } else {
                const f32x16 dp = at_dot_tile<HALF>(Vs, WS, gb, c, h);   // dP^T[key][query]
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int key = sx_kmap(j, h);
                    float pv = __expf(s[j] * a.scale + kb[key] - lse_q);
                    if (p.mask_diagonal && k0 + key == qi) pv = 0.f;
                    s[j] = pv * (dp[j] - dlt);
                }
                at_acc_tiles<DT>(acc, Ks, WS, s, c, h, dh);           // dQ^T += K^T dS^T
            }
        }
        if (!qlive) continue;
        if constexpr (!BWD) {
            const float inv = l > 0.f ? 1.f / l : 0.f;
            // (o / l) * mask, as attention.py:44-48 rounds: softmax, @ value, then * mask
            float *o = a.out + qrow * E + (int64_t)head * dh;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int d = 32 * t + sx_kmap(j, h);
                    if (d < dh) o[d] = (acc[t][j] * inv) * mo;
                }
            if (h == 0) a.lse[(r * H + head) * p.Nq + qi] = l > 0.f ? m + __logf(l) : INFINITY;
        } else {
            at_store_tiles<DT>(a.dq, qrow, E, head, dh, acc, h, a.scale);
            if (h == 0) a.delta[(r * H + head) * p.Nq + qi] = dlt;
        }
    }
}

// ---- the key-owner pass of the backward: dk, dv ---------------------------------------------------------------------------
template <int HALF>
__global__ __launch_bounds__(SX_ATT_MAX_WAVES * 64) void attention_kv_kernel(const at_args a) {
    constexpr int DT = (2 * HALF + 31) / 32, WS = 32 * DT + 1;
    const sx_attention_args &p = a.p;
    float *Qs = at_smem, *Gs = Qs + 32 * WS, *ls = Gs + 32 * WS, *ds = ls + 32;
    at_zero_lds(64 * WS);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5, W = blockDim.x >> 6;
    const int H = p.n_heads, E = p.E, dh = a.dh;
    const int64_t n_units = p.R * H * a.n_kblk;
    const float *mrow = p.out_mask ? p.mask : nullptr;
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int kblk = (int)(unit % a.n_kblk);
        const int64_t rh = unit / a.n_kblk;
        const int head = (int)(rh % H);
        const int64_t r = rh / H;
        const int k0 = (kblk * W + (threadIdx.x >> 6)) * 32, kj = k0 + c;
        const bool klive = kj < p.Nk, wave_live = k0 < p.Nk;
        const float kbias = at_key_live(p, r, kj) ? 0.f : -INFINITY;
        float kr[HALF], vr[HALF];
        at_load_half<HALF>(kr, p.k + r * p.k_bs + (int64_t)kj * p.k_rs + (int64_t)head * dh, klive, h, dh);
        at_load_half<HALF>(vr, p.v + r * p.v_bs + (int64_t)kj * p.v_rs + (int64_t)head * dh, klive, h, dh);
        f32x16 gk[DT], gv[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) gk[t] = gv[t] = f32x16{};
        for (int q0 = 0; q0 < p.Nq; q0 += 32) {
            __syncthreads();
            at_stage(Qs, WS, p.q, p.q_bs, p.q_rs, r, q0, p.Nq, head, dh, nullptr, 0);
            at_stage(Gs, WS, a.dy, (int64_t)p.Nq * E, E, r, q0, p.Nq, head, dh, mrow, p.mask_bs);
            if (threadIdx.x < 32) {
                const int qi = q0 + (int)threadIdx.x;
                const bool ok = qi < p.Nq;
                ls[threadIdx.x] = ok ? a.lse[(r * H + head) * p.Nq + qi] : INFINITY;
                ds[threadIdx.x] = ok ? a.delta[(r * H + head) * p.Nq + qi] : 0.f;
            }
            __syncthreads();
            if (!wave_live) continue;
            f32x16 s = at_dot_tile<HALF>(Qs, WS, kr, c, h);          // S[query sx_kmap(j, h)][key c]
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int qr = sx_kmap(j, h);
                float pv = __expf(s[j] * a.scale + kbias - ls[qr]);
                if (p.mask_diagonal && q0 + qr == kj) pv = 0.f;
                s[j] = pv;
            }
            at_acc_tiles<DT>(gv, Gs, WS, s, c, h, dh);                   // dV^T += dy_att^T P
            const f32x16 dp = at_dot_tile<HALF>(Gs, WS, vr, c, h);   // dP[query][key]
#pragma unroll
            for (int j = 0; j < 16; ++j) s[j] = s[j] * (dp[j] - ds[sx_kmap(j, h)]);
            at_acc_tiles<DT>(gk, Qs, WS, s, c, h, dh);                   // dK^T += Q^T dS
        }
        if (!klive) continue;
        at_store_tiles<DT>(a.dk, r * p.Nk + kj, E, head, dh, gk, h, a.scale);
        at_store_tiles<DT>(a.dv, r * p.Nk + kj, E, head, dh, gv, h, 1.f);
    }
}

inline int at_half(int dh) { return dh <= 8 ? 4 : dh <= 16 ? 8 : dh <= 32 ? 16 : dh <= 64 ? 32 : 64; }
inline int at_dt(int half) { return (2 * half + 31) / 32; }
inline int at_waves(int n) { const int w = (n + 31) / 32; return w < 1 ? 1 : w > SX_ATT_MAX_WAVES ? SX_ATT_MAX_WAVES : w; }

template <typename K>
int at_launch(K kern, const at_args &a, int waves, int64_t n_units, size_t lds, void *stream) {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kern, waves * 64, lds);
    if (cus < 1) cus = 1;
    if (per_cu < 1) per_cu = 1;
    const int64_t cap = (int64_t)cus * per_cu;
    const int grid = (int)(n_units < cap ? n_units : cap);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), lds, sx_stream(stream), a);
    SX_LAUNCH_CHECK();
    return SX_OK;
}

int at_validate(const sx_attention_args *p, const char *who) {
    SX_REQUIRE(p != nullptr, "%s: null arguments", who);
    SX_REQUIRE(p->R >= 0 && p->Nq >= 0 && p->Nk >= 0, "%s: negative R / Nq / Nk", who);
    SX_REQUIRE(p->n_heads >= 1 && p->E >= 1 && p->E % p->n_heads == 0, "%s: E = %d is not a multiple of n_heads = %d", who, p->E,
               p->n_heads);
    const int dh = p->E / p->n_heads;
    SX_REQUIRE(dh >= 1 && dh <= SX_ATTENTION_MAX_HEAD_DIM, "%s: head width %d outside 1..%d", who, dh, SX_ATTENTION_MAX_HEAD_DIM);
    SX_REQUIRE(p->q && p->k && p->v, "%s: null q / k / v", who);
    SX_REQUIRE(p->q_bs >= 0 && p->q_rs >= 0 && p->k_bs >= 0 && p->k_rs >= 0 && p->v_bs >= 0 && p->v_rs >= 0 && p->mask_bs >= 0,
               "%s: negative stride", who);
    SX_REQUIRE(!p->mask_diagonal || p->Nq == p->Nk, "%s: mask_diagonal needs Nq == Nk (got %d, %d)", who, p->Nq, p->Nk);
    SX_REQUIRE(!p->out_mask || (p->mask != nullptr && p->Nq == p->Nk), "%s: out_mask needs a mask and Nq == Nk", who);
    return SX_OK;
}

at_args at_make(const sx_attention_args *p) {
    at_args a{};
    a.p = *p;
    a.dh = p->E / p->n_heads;
    a.scale = (float)sqrt(1.0 / (double)a.dh);                   // attention.py:33: (1 / dh) ** 0.5, a float multiplier
    return a;
}

inline size_t at_lds(int half) { return (size_t)(64 * (32 * at_dt(half) + 1) + 64) * sizeof(float); }

// KERNEL: a function-like macro naming the kernel instance for a HALF
#define AT_DISPATCH(KERNEL, N_UNITS, WAVES)                                                                    \
    switch (at_half(a.dh)) {                                                                                  \
        case 4: return at_launch(KERNEL(4), a, WAVES, N_UNITS, at_lds(4), stream);                            \
        case 8: return at_launch(KERNEL(8), a, WAVES, N_UNITS, at_lds(8), stream);                            \
        case 16: return at_launch(KERNEL(16), a, WAVES, N_UNITS, at_lds(16), stream);                         \
        case 32: return at_launch(KERNEL(32), a, WAVES, N_UNITS, at_lds(32), stream);                         \
        default: return at_launch(KERNEL(64), a, WAVES, N_UNITS, at_lds(64), stream);                         \
    }

#define AT_FWD(H_) attention_q_kernel<H_, false>
#define AT_BWD_Q(H_) attention_q_kernel<H_, true>
#define AT_BWD_KV(H_) attention_kv_kernel<H_>

int at_bwd_q(const at_args &a, int waves, int64_t n_units, void *stream) {
    AT_DISPATCH(AT_BWD_Q, n_units, waves)
}

}  // namespace

extern "C" int sx_attention_fwd(const sx_attention_args *args_host, float *out, float *lse, void *stream) {
    const int rc = at_validate(args_host, "sx_attention_fwd");
    if (rc != SX_OK) return rc;
    SX_REQUIRE(out != nullptr && lse != nullptr, "sx_attention_fwd: null out / lse");
    if (args_host->R == 0 || args_host->Nq == 0) return SX_OK;
    at_args a = at_make(args_host);
    a.out = out;
    a.lse = lse;
    const int waves = at_waves(a.p.Nq);
    a.n_qblk = (a.p.Nq + 32 * waves - 1) / (32 * waves);
    const int64_t n_units = a.p.R * a.p.n_heads * a.n_qblk;
    AT_DISPATCH(AT_FWD, n_units, waves)
}

extern "C" int sx_attention_bwd(const sx_attention_args *args_host, const float *y, const float *dy, const float *lse, float *dq,
                                float *dk, float *dv, float *delta, void *stream) {
    const int rc = at_validate(args_host, "sx_attention_bwd");
    if (rc != SX_OK) return rc;
    SX_REQUIRE(y && dy && lse && dq && dk && dv && delta, "sx_attention_bwd: null y / dy / lse / dq / dk / dv / delta");
    if (args_host->R == 0) return SX_OK;
    at_args a = at_make(args_host);
    a.y = y; a.dy = dy; a.lse = const_cast<float *>(lse); a.dq = dq; a.dk = dk; a.dv = dv; a.delta = delta;
    const int64_t R = a.p.R, H = a.p.n_heads;
    if (a.p.Nq > 0) {                                             // dq and D (every dq row is written, Nk = 0 included)
        const int waves = at_waves(a.p.Nq);
        a.n_qblk = (a.p.Nq + 32 * waves - 1) / (32 * waves);
        const int e = at_bwd_q(a, waves, R * H * a.n_qblk, stream);
        if (e != SX_OK || a.p.Nk == 0) return e;
    }
    if (a.p.Nk == 0) return SX_OK;
    const int waves = at_waves(a.p.Nk);                           // dk, dv (every row is written, Nq = 0 included)
    a.n_kblk = (a.p.Nk + 32 * waves - 1) / (32 * waves);
    const int64_t n_units = R * H * a.n_kblk;
    AT_DISPATCH(AT_BWD_KV, n_units, waves)
}
