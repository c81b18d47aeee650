// What the one-launch CNF kernels (sx_cnf.hip, sx_cnf_adaptive.hip, sx_cnf_exact.hip, sx_cnf_set.hip, sx_cnf_exact_set.hip, sx_cnf_attn.hip,
// sx_cnf_exact_attn.hip), the training kernels of the dense CNF (sx_cnf_train.hip) and the Deep Sets conditioner (sx_equivariant.hip)
// have in common:
//   * the layout: a workgroup of 4 waves, one wave = 32 rows on the MFMA column (lane & 31), features on the C rows, a 32-feature tile
//     of a row = one f32x16 C fragment = the B operand of the next GEMM; feature sx_kmap(r, h) (sx_common.h) sits in register r of
//     lane half h;
//   * the seven activations whose derivative is a function of the activation's OUTPUT, and their sweeps over tiles;
//   * a row's load and store in C-fragment order;
//   * LDS images in A-fragment order, their staging, and the exact-fp32 product against them (v_mfma_f32_32x32x2_f32);
//   * the fixed grid and the euler / midpoint / rk4 (3/8 rule) tableau.  The files that include this header are compiled with
//     -ffp-contract=off: the tableau's parenthesisation is the reference solver's sequence of roundings;
//   * sets: a workgroup's pass over whole sets, where a lane stands in it (cnf_set_pos, cnf_set_pass) and the ordered set sum through
//     LDS (cnf_setsum) -- the set CNF kernels and both Deep Sets kernels;
//   * the per-call argument checks, and cnf_launch: sx_common.h's sx_launch_capped at this family's workgroup size and LDS limit.
// The weight-gradient contraction of the training kernels is not here: sx_train_contract.h.
// sx_cnf.hip, sx_cnf_adaptive.hip and sx_cnf_train.hip take it through sx_cnf_dense.h, which adds what the dense files share with each other alone;
// they use all of it but cnf_act_all (sx_cnf_dense.h's sweep keeps the widest dense kernel free of spills) and cnf_latent_packed.
// sx_cnf_exact.hip, sx_cnf_exact_set.hip and sx_cnf_exact_attn.hip take it through sx_cnf_exact_common.h, which does the same for the
// exact-trace files; the two attention files add sx_cnf_attn_common.h.
// Everything here has internal linkage: ten translation units include it (the nine above, and sx_base.hip for the MFMA layout).
#pragma once
#include "sx_common.h"

#define SX_CNF_WAVES 4
#define SX_CNF_THREADS (SX_CNF_WAVES * 64)
#define SX_CNF_ROWS (SX_CNF_WAVES * 32)          /* row slots of a workgroup */

namespace {

// tiles of 32 that hold n features (the exact-trace and set kernels cap their widths at 64 in their validators: 1 or 2 there); tiles that hold the d_h slots of every dimension, two slots (the two lane halves) per tile
__host__ __device__ constexpr int cnf_tiles(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : 4; }
__host__ __device__ constexpr int cnf_out_tiles(int d_h) { return d_h <= 2 ? 1 : d_h <= 4 ? 2 : 4; }

extern __shared__ __attribute__((aligned(16))) float cnf_smem[];

__device__ __forceinline__ float cnf_act(float v, int act) {
    switch (act) {
        case SX_ACT_TANH: return tanhf(v);
        case SX_ACT_RELU: return fmaxf(v, 0.f);
        case SX_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        case SX_ACT_ELU: return v > 0.f ? v : expm1f(v);
        case SX_ACT_SOFTPLUS: return v > 20.f ? v : log1pf(expf(v));
        case SX_ACT_LEAKYRELU: return v > 0.f ? v : 0.01f * v;
        default: return v;
    }
}

// act'(v) from a = act(v)
__device__ __forceinline__ float cnf_dact(float a, int act) {
    switch (act) {
        case SX_ACT_TANH: return 1.f - a * a;
        case SX_ACT_RELU: return a > 0.f ? 1.f : 0.f;
        case SX_ACT_SIGMOID: return a * (1.f - a);
        case SX_ACT_ELU: return a > 0.f ? 1.f : a + 1.f;
        case SX_ACT_SOFTPLUS: return 1.f - expf(-a);            // sigmoid(v) = 1 - exp(-softplus(v))
        case SX_ACT_LEAKYRELU: return a > 0.f ? 1.f : 0.01f;
        default: return 1.f;
    }
}

template <int T>
struct cnf_tile {
    f32x16 v[T];
};

template <int T>
__device__ __forceinline__ void cnf_act_all(cnf_tile<T> &v, int act) {
    if (act == SX_ACT_IDENTITY) return;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) v.v[m][r] = cnf_act(v.v[m][r], act);
}

// v <- act'(v) from v = act(v): one tile (inlined on purpose: an out-of-line call would spill the live stage vectors around it), T tiles
__device__ __forceinline__ void cnf_dact_tile(f32x16 &v, int act) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = cnf_dact(v[r], act);
}

template <int T>
__device__ __forceinline__ void cnf_dact_all(cnf_tile<T> &v, int act) {
#pragma unroll
    for (int m = 0; m < T; ++m) cnf_dact_tile(v.v[m], act);
}

// feature 32m + kmap(r, h) of a padded vector at `vb` (already offset by 4 * h)
__device__ __forceinline__ float cnf_vec(const float *vb, int m, int r) { return vb[32 * m + 8 * (r >> 2) + (r & 3)]; }

template <int T>
__device__ __forceinline__ void cnf_add_vec(cnf_tile<T> &v, const float *vb) {
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) v.v[m][r] += cnf_vec(vb, m, r);
}

// register i (wave-uniform) of a tile
__device__ __forceinline__ float cnf_pick(const f32x16 &v, int i) {
    float s = v[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) s = (i == r) ? v[r] : s;
    return s;
}

// ---- rows in C-fragment order ------------------------------------------------------------------------------------------------------
// the lane's row of a [n, D] array as a state of T tiles: register r of tile c <- feature 32c + sx_kmap(r, h) (h = lane >> 5), 0
// beyond D and on a row that is not live; and back (a row that is not live is not stored)
template <int T>
__device__ __forceinline__ void cnf_load_row(cnf_tile<T> &v, const float *p, int64_t row, int D, bool live, int h) {
#pragma unroll
    for (int c = 0; c < T; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * c + sx_kmap(r, h);
            v.v[c][r] = (live && f < D) ? p[row * D + f] : 0.f;
        }
}

template <int T>
__device__ __forceinline__ void cnf_store_row(float *p, const cnf_tile<T> &v, int64_t row, int D, bool live, int h) {
    if (!live) return;
#pragma unroll
    for (int c = 0; c < T; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * c + sx_kmap(r, h);
            if (f < D) p[row * D + f] = v.v[c][r];
        }
}

// LDS image of a matrix block: MT x KT A-operand tiles of 1024 floats (tile (m, c), float g*256 + lane*4 + j holds
// W[32m + (lane & 31)][col0 + 32c + kmap(4g + j, lane >> 5)]), W row-major with row stride ld
__device__ __forceinline__ void cnf_stage(const float *__restrict__ W, int out_dim, int in_dim, int ld, int col0, int MT, int KT, int base) {
    const int n_w = MT * KT * 1024;
    for (int e = threadIdx.x; e < n_w; e += SX_CNF_THREADS) {
        const int tile = e >> 10, rem = e & 1023;
        const int g = rem >> 8, lane = (rem >> 2) & 63, j = rem & 3;
        const int m = tile / KT, c = tile - m * KT;
        const int row = 32 * m + (lane & 31), col = 32 * c + sx_kmap(4 * g + j, lane >> 5);
        cnf_smem[base + e] = (row < out_dim && col < in_dim) ? W[(int64_t)row * ld + col0 + col] : 0.f;
    }
}

// a vector of n_pad floats (entries beyond n: 0), element i at stride `stride` of src (NULL: zeros)
__device__ __forceinline__ void cnf_stage_vec(const float *__restrict__ src, int n, int stride, int n_pad, int base) {
    for (int i = threadIdx.x; i < n_pad; i += SX_CNF_THREADS)
        cnf_smem[base + i] = (src != nullptr && i < n) ? src[(int64_t)i * stride] : 0.f;
}

// an image the caller built in the kernel's own order (16-byte aligned, a multiple of 4 floats): a straight copy
__device__ __forceinline__ void cnf_stage_image(const float *__restrict__ image, int floats) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(image);
    f32x4 *dst = reinterpret_cast<f32x4 *>(cnf_smem);
    for (int e = threadIdx.x; e < floats / 4; e += SX_CNF_THREADS) dst[e] = src[e];
}

// THE product: acc += (a tile row of W) . in -- the KT input tiles against the KT A tiles at `wb` (tile (m, 0) of an LDS image,
// already offset by lane * 4)
template <int KT>
__device__ __forceinline__ void cnf_mma(f32x16 &acc, const cnf_tile<KT> &in, const float *wb) {
#pragma unroll
    for (int c = 0; c < KT; ++c) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(wb + c * 1024 + g * 256);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, in.v[c][4 * g + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, in.v[c][4 * g + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, in.v[c][4 * g + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, in.v[c][4 * g + 3], acc, 0, 0, 0);
        }
    }
}

// out[m] = (W . in)[m], m < MT; W: an image at `wb` (already offset by lane * 4), KT input tiles
template <int KT, int MT>
__device__ __forceinline__ void cnf_gemm(const cnf_tile<KT> &in, cnf_tile<MT> &out, const float *wb) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        f32x16 acc = {};
        cnf_mma<KT>(acc, in, wb + m * KT * 1024);
        out.v[m] = acc;
    }
}

// cnf_mma with the 32 matrix rows read from global memory: `W` = row 32m of a row-major matrix of KT * 32 columns, zero-padded (a
// lane's four A values of k-group g are the contiguous columns 32c + 8g + 4h .. + 3 of row lane & 31)
template <int KT>
__device__ __forceinline__ void cnf_mma_global(f32x16 &acc, const cnf_tile<KT> &in, const float *__restrict__ W, int lane) {
    const float *wl = W + (int64_t)(lane & 31) * (KT * 32) + 4 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < KT; ++c) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(wl + 32 * c + 8 * g);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, in.v[c][4 * g + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, in.v[c][4 * g + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, in.v[c][4 * g + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, in.v[c][4 * g + 3], acc, 0, 0, 0);
        }
    }
}

// the latent share of a first layer whose latent columns the caller packed: lat = w_latent . latent_row, once per row (w_latent:
// row-major [HT * 32][32 * ceil(L / 32)], zero-padded; A fragments straight from global memory: once per group, no LDS spent on it)
template <int HT>
__device__ __forceinline__ void cnf_latent_packed(cnf_tile<HT> &lat, const float *__restrict__ w_latent, const float *__restrict__ latent,
                                                  int64_t row, bool live, int L, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int m = 0; m < HT; ++m) lat.v[m] = f32x16{};
    if (L > 0) {
        const int LT = (L + 31) >> 5;
        for (int c = 0; c < LT; ++c) {
            f32x16 lb;          // (sx_kmap(r, h) by hand: with the call, or a shared tile load, every exact-trace kernel is allocated differently)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h;
                lb[r] = (live && f < L) ? latent[row * L + f] : 0.f;
            }
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                const float *wr = w_latent + (int64_t)(32 * m + (lane & 31)) * (LT * 32) + 32 * c + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 av = *reinterpret_cast<const f32x4 *>(wr + 8 * g);
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, lb[4 * g + 0], lat.v[m], 0, 0, 0);
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, lb[4 * g + 1], lat.v[m], 0, 0, 0);
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, lb[4 * g + 2], lat.v[m], 0, 0, 0);
                    lat.v[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, lb[4 * g + 3], lat.v[m], 0, 0, 0);
                }
            }
        }
    }
}

// ---- the fixed-grid solver ---------------------------------------------------------------------------------------------------------
// step i of the grid: t_i = t0 +- i * step_size, the last point replaced by t1 (A: a kernel's argument struct)
template <class A>
__device__ __forceinline__ void cnf_grid(const A &a, float sgn, int i, float &ta, float &tb) {
    ta = i == 0 ? a.t0 : a.t0 + sgn * ((float)i * a.step_size);
    tb = i + 1 == a.n_steps ? a.t1 : a.t0 + sgn * ((float)(i + 1) * a.step_size);
}

__device__ __forceinline__ int cnf_stages(int solver) { return solver == SX_CNF_EULER ? 1 : solver == SX_CNF_MIDPOINT ? 2 : 4; }

// stage `st` of a step [ta, tb] after the evaluation k = f(ts, xs), q = tr df/dx: the next stage's point (xs, ts), or -- after the
// last stage -- the step itself (y, and the log-det l).  k1 / k2 and q1 / q2 live across the stages of one step (rk4: after stage 3,
// k1 holds k1 + 3 (k2 + k3)).  One state = T tiles; the order of the operations is the reference solver's and must stay as written.
template <int T>
__device__ __forceinline__ void cnf_tableau(int solver, int st, float ta, float tb, float dt, float half, float third, float two_thirds,
                                            const cnf_tile<T> &k, float q, cnf_tile<T> &k1, cnf_tile<T> &k2, float &q1, float &q2,
                                            cnf_tile<T> &xs, float &ts, cnf_tile<T> &y, float &l) {
    if (solver == SX_CNF_EULER) {                       // y += dt f(t, y)
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) y.v[c][r] = y.v[c][r] + dt * k.v[c][r];
        l = l + dt * q;
    } else if (solver == SX_CNF_MIDPOINT) {             // y += dt f(t + dt/2, y + f(t, y) dt/2)
        if (st == 0) {
#pragma unroll
            for (int c = 0; c < T; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) xs.v[c][r] = y.v[c][r] + k.v[c][r] * half;
            ts = ta + half;
        } else {
#pragma unroll
            for (int c = 0; c < T; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) y.v[c][r] = y.v[c][r] + dt * k.v[c][r];
            l = l + dt * q;
        }
    } else if (st == 0) {                                 // rk4, the 3/8 rule
        k1 = k; q1 = q;
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) xs.v[c][r] = y.v[c][r] + (dt * k1.v[c][r]) * third;
        ts = ta + dt * third;
    } else if (st == 1) {
        k2 = k; q2 = q;
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) xs.v[c][r] = y.v[c][r] + dt * (k2.v[c][r] - k1.v[c][r] * third);
        ts = ta + dt * two_thirds;
    } else if (st == 2) {
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                xs.v[c][r] = y.v[c][r] + dt * ((k1.v[c][r] - k2.v[c][r]) + k.v[c][r]);
                k1.v[c][r] = k1.v[c][r] + 3.f * (k2.v[c][r] + k.v[c][r]);
            }
        q1 = q1 + 3.f * (q2 + q);
        ts = tb;
    } else {
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) y.v[c][r] = y.v[c][r] + ((k1.v[c][r] + k.v[c][r]) * dt) * 0.125f;
        l = l + ((q1 + q) * dt) * 0.125f;
    }
}

// ---- sets --------------------------------------------------------------------------------------------------------------------------
// A workgroup's 128 row slots take floor(128 / N) WHOLE sets of N = set_size contiguous rows per pass: sets never straddle
// workgroups, they may straddle waves.  Slots past the last set are padding: they compute on zeros and are never stored.
__host__ __device__ inline int cnf_rows_per_pass(int set_size) { return (SX_CNF_ROWS / set_size) * set_size; }
__device__ __forceinline__ int64_t cnf_set_passes(int N, int64_t n_rows) {
    const int rows_per_pass = cnf_rows_per_pass(N);
    return (n_rows + rows_per_pass - 1) / rows_per_pass;
}

// where a lane stands in its workgroup's pass
struct cnf_set_pos {
    int rho;            // row slot 0 .. SX_CNF_ROWS - 1
    int first;          // the first slot of the row's set (a padding slot: itself)
    int n_here;         // rows of this pass
    int n_sets;         // whole sets of this pass (n_here / N)
    bool live;          // the slot holds a row
    int64_t row;        // that row
};

// the lane's row slot: the same in every pass
__device__ __forceinline__ int cnf_set_slot(int lane) { return (threadIdx.x >> 6) * 32 + (lane & 31); }

// the lane's place in pass `pass`, from p.rho = cnf_set_slot(lane) (for pass = blockIdx.x; pass < cnf_set_passes(); pass += gridDim.x:
// every bound of that loop is uniform over the workgroup, so all four waves make every pass and meet at every barrier); -> the rows
// of the pass
__device__ __forceinline__ void cnf_set_pass(cnf_set_pos &p, int64_t pass, int N, int64_t n_rows) {
    const int rows_per_pass = cnf_rows_per_pass(N);
    const int64_t base = pass * rows_per_pass, left = n_rows - base;
    p.n_here = left < rows_per_pass ? (int)left : rows_per_pass;
    p.live = p.rho < p.n_here;
    p.row = base + p.rho;
    p.first = p.live ? (p.rho / N) * N : p.rho;
    p.n_sets = p.n_here / N;
}

// The ordered set sum: out = the sum of `in` over the rows of the lane's set, e_out = that of the per-row scalar e_in (both lane
// halves pass the same e_in).  Every lane writes its row's features to the LDS scratch at float offset `scratch`, [SX_CNF_ROWS][LD]
// with LD >= 32 T + 4 (the column after the features carries the scalar along), one thread per (set, column) adds the set's N rows
// IN ROW ORDER into the set's first row, and every lane reads its set's first row back.  The order of the additions depends on the
// position inside the set only, so a set's result depends neither on its slot nor on its neighbours.
//   * three workgroup barriers: EVERY thread of the workgroup must call it, padding waves included, under workgroup-uniform control;
//   * `out` may alias `in`;
//   * N == 1 needs no exchange (and meets no barrier).
template <int T, int LD>
__device__ __forceinline__ void cnf_setsum(int scratch, int N, const cnf_set_pos &p, const cnf_tile<T> &in, cnf_tile<T> &out, float e_in, float &e_out,
                                           int lane) {
    if (N == 1) {
        out = in;
        e_out = e_in;
        return;
    }
    float *xs = cnf_smem + scratch;
    const int h = lane >> 5;
    __syncthreads();                    // the reads of the previous exchange are over
    float *mine = xs + p.rho * LD + 4 * h;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4 *>(mine + 32 * m + 8 * g) = f32x4{in.v[m][4 * g], in.v[m][4 * g + 1], in.v[m][4 * g + 2], in.v[m][4 * g + 3]};
    if (h == 0) xs[p.rho * LD + 32 * T] = e_in;
    __syncthreads();
    constexpr int COLS = 32 * T + 1;
    const int n_pairs = p.n_sets * COLS;
    for (int q = threadIdx.x; q < n_pairs; q += SX_CNF_THREADS) {
        const int s = q / COLS, f = q - s * COLS;
        float *col = xs + (s * N) * LD + f;
        float acc = col[0];
        for (int j = 1; j < N; ++j) acc = acc + col[j * LD];
        col[0] = acc;
    }
    __syncthreads();
    const float *src = xs + p.first * LD + 4 * h;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(src + 32 * m + 8 * g);
            out.v[m][4 * g] = v.x; out.v[m][4 * g + 1] = v.y; out.v[m][4 * g + 2] = v.z; out.v[m][4 * g + 3] = v.w;
        }
    e_out = xs[p.first * LD + 32 * T];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// workgroups that cover n_rows: independent rows (a wave per 32), or whole sets (a pass each)
inline int64_t cnf_row_blocks(int64_t n_rows) { return ((n_rows + 31) / 32 + SX_CNF_WAVES - 1) / SX_CNF_WAVES; }
inline int64_t cnf_set_blocks(int64_t n_rows, int set_size) { return (n_rows + cnf_rows_per_pass(set_size) - 1) / cnf_rows_per_pass(set_size); }

// the per-call arguments every flow call takes; `fn`: the entry point's name (set_size 1: rows are independent)
inline int cnf_check_call(const char *fn, int solver, int64_t n_rows, int set_size, int n_steps, float step_size, const float *x, const float *y) {
    SX_REQUIRE(solver >= SX_CNF_EULER && solver <= SX_CNF_RK4, "%s: solver must be euler (0), midpoint (1) or rk4 (2), got %d", fn, solver);
    SX_REQUIRE(n_rows >= 0 && n_steps >= 0, "%s: negative n_rows / n_steps", fn);
    SX_REQUIRE(n_rows % set_size == 0, "%s: n_rows (%lld) is not a multiple of set_size (%d)", fn, (long long)n_rows, set_size);
    SX_REQUIRE(n_steps <= 1 || step_size > 0.f, "%s: a grid of %d steps needs step_size > 0", fn, n_steps);
    SX_REQUIRE(x != nullptr && y != nullptr, "%s: null input / output", fn);
    return SX_OK;
}

// sx_common.h's launcher at this family's workgroup size and LDS limit.  `fn`: the entry point's name, for the messages.
template <auto KERN, class A>
int cnf_launch(const char *fn, const A &a, size_t lds, int64_t want, void *stream, int *grid_out = nullptr) {
    return sx_launch_capped<KERN>(fn, a, SX_CNF_THREADS, lds, SX_CNF_LDS_BYTES, want, stream, grid_out);
}

}  // namespace
