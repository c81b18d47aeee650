// Training backward of one rational-quadratic SPLINE COUPLING (inverse direction, the one log_prob evaluates) with the
// [N, n_live * (3K-1)] parameter tensor of the reference (stribor/flows/spline.py:76-87, coupling.py:69-95) never in HBM.
//
// The layer-wise path used to materialise the conditioner's output (1,504 floats per row on cfg 3: 1.6 GB per layer and
// 2^18 rows) and move it five times: written by the last Linear, read by the spline forward, read + written (as gradients)
// by the spline backward, read by each of the two library GEMMs of the Linear's backward (dW2 = dp^T h, dh = dp W2).
// Here ONE kernel does all of that per layer, tiled the other way round:
//
//   * a workgroup owns a SLAB of the last Linear: the 3K-1 parameter rows of TWO transformed columns (94 rows at K = 16,
//     padded to three 32-row MFMA tiles: widths | heights | derivatives) and walks a range of the rows.  The slab's
//     weights sit in LDS in both orientations (W2 slab as the A operand of  p = W2 h + b2,  its transpose as the A operand
//     of  dh = W2^T dp) for the whole launch: 48 KB at hidden = 64;
//   * a wave takes 32 rows at a time: h (the last hidden activation, 256 B per row, the only per-row input besides x and
//     the two adjoints) -> fp16 x 3 split -> the slab's parameters by MFMA.  Tile row R carries parameter (R&3) + 4(R>>3)
//     of column (R>>2)&1, so in C-fragment order lane (sample, half) receives, in 3 x 16 registers, exactly the 3K-1
//     parameters of ITS element (sample, column 2 slab + half): the spline's reverse mode (sx_rqs_bwd.h) runs on registers
//     with static indices and leaves the parameter gradients in the same registers;
//   * those three tiles are, unchanged, the B operand of dh_partial = W2_slab^T dp (C tile -> next MFMA's operand), and --
//     turned by the matrix pipe against a 0/1 selection operand, as in the layer-major affine backward
//     (sx_flow_kernel.h, `turn_tile` / `contract`) -- the A operand of dW2_slab += dp^T h, accumulated in 6 accumulator
//     tiles (96 registers) over all the rows the wave visits.  One partial per workgroup leaves at the end.
//   * dh is a sum over the slabs: each slab writes its partial in fragment order (1 KB per store instruction) and a small
//     second kernel adds the n_slabs partials into the row-major dL/dh the conditioner's own backward consumes.
//
// HBM per row and layer: x, dL/dout (2 columns x 4 B each per slab), h 256 B (L2-resident across the slabs), and
// 2 x n_slabs x 256 B of dh partials -- 8 KB at 16 slabs against 30 KB for the five crossings of the parameter tensor.
#define SX_F16X3
#include <type_traits>
#include "sx_flow_kernel.h"
#include "sx_rqs_bwd.h"
#include "sx_cubic_core.h"

namespace {
using namespace sx_f16x3;

struct slab_args {
    const float *x, *gout, *gldj, *h;   // x, gout [N, dim]; gldj [N]; h [N, ld_h] (H valid features)
    const float *xout;                  // cubic splines: the inverse pass's output [N, dim] (the solve is differentiated there)
    const float *wf;                    // sx_pack_linear(W2 rows by slot): [3 n_slabs][HT][1024] + bias [3 n_slabs][32]
    const float *wb;                    // sx_pack_linear(transpose): [HT][3 n_slabs][1024]
    float *gx;                          // [N, dim]: the transformed columns are written
    float *dh_part;                     // [n_slabs][n_chunks][HT][1024], fragment order
    float *w_part;                      // [n_slabs][n_ranges][96 * 32 HT + 96]
    const int32_t *live_idx;
    const float *scale;                 // max |adjoint| (device scalar) or null: see slab_scale_in / sx_rqs_slab_bwd
    uint32_t *flags;
    int64_t n_rows, ld_h;
    int l0, n_live, K, dim, H, n_slabs, n_chunks, n_groups, n_ranges, xcd_map;
    float left, right, bottom, top, ldj_scale;
};

// Power-of-two scale of the adjoints from their largest magnitude (a device scalar the caller reduced): S = 2^-ilogb(gmax),
// so that S * gmax is in [1, 2).  Exact, and the same value in every kernel that derives it.
__device__ __forceinline__ float slab_scale_in(const float *gmax) {
    if (gmax == nullptr) return 1.f;
    const float g = gmax[0];
    if (!(g > 0.f) || !(g < 3.0e38f)) return 1.f;
    return ldexpf(1.f, -ilogbf(g));
}
__device__ __forceinline__ float slab_scale_out(const float *gmax) {
    if (gmax == nullptr) return 1.f;
    const float g = gmax[0];
    if (!(g > 0.f) || !(g < 3.0e38f)) return 1.f;
    return ldexpf(1.f, ilogbf(g));
}

// A-operand fragments of one 32 x 32 tile for k16-step s (hi, lo), read from LDS
struct afrag { h8 hi, lo; };
__device__ __forceinline__ afrag load_afrag(const char *wb, int a_off, int s) {
    afrag a;
    a.hi = __builtin_bit_cast(h8, *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s) * 256) * 4));
    a.lo = __builtin_bit_cast(h8, *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s + 1) * 256) * 4));
    return a;
}
__device__ __forceinline__ f32x16 mfma(const h8 &a, const h8 &b, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Pairwise hand-over through LDS flags (monotone pass counters): the two waves of a slab pair meet once per pass to exchange
// a dh tile; a workgroup barrier there would also tie the four independent pairs (and the two waves that share a SIMD) to
// one another's memory latencies.
__device__ __forceinline__ void flag_wait_ge(int *flag, int target) {
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
}
__device__ __forceinline__ void flag_set(int *flag, int v) {
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// HFULL: h rows are 16-byte aligned and exactly 32 HT wide (vector loads, no column guards).
// SPW slabs per workgroup (4 waves each, the same 4 chunks of rows per pass): with SPW = 2 the two slabs' waves exchange one
// dh tile each through LDS, so only ONE partial per slab pair goes to HBM (the dh partials are the kernel's HBM traffic).
// Workgroup id -> (slab group, row range) is XCD-aware: ids are dealt round-robin to the 8 XCDs, so the n_groups workgroups
// that walk the same rows (and re-read the same h / x lines) are given ids 8 apart -- the same XCD, the same L2.
// CUBIC: monotone cubic splines (2K + 2 parameters per element: widths | heights | two boundary derivatives in the third tile).
// HT = 3, 4 (hidden layers of 65 .. 128 units, round 5): the 3 HT accumulator tiles of dW2 (144 / 192 registers) leave no room for two
// waves per SIMD -- SPW = 1, one 4-wave workgroup per CU, the whole 512-register file per wave; 72 / 96 KB of LDS.
// HTF > HT (hidden layers of 129 .. 256 units, HTF = 5 .. 8 tiles; round 5): the launch covers hidden tiles [M0, M0 + HT) of the HTF --
// the parameters need every tile (the slab's forward weights: 3 HTF tiles), dh and dW2 only this launch's (its transposed weights
// and accumulators: 3 HT tiles); two launches (HT = ceil(HTF / 2) and the rest) cover the layer, each repeating the spline's
// reverse mode.  The registers are those of the HT = 3 / 4 form.
template <int HT, int KC, bool HFULL, int SPW, bool CUBIC, int HTF = HT, int M0 = 0>
__global__ __launch_bounds__(256 * SPW, (SPW == 1 && HT <= 2 && HTF == HT) ? 2 : 1) void rqs_slab_bwd_kernel(const slab_args k) {
    static_assert(M0 + HT <= HTF && (HTF == HT || SPW == 1), "hidden-tile window");
    constexpr int SLAB_F = 3 * (HTF + HT) * 1024;                       // per slab: W2 slab (every hidden tile) | its transpose (this launch's tiles)
    constexpr int FWo = 0, BWo = 3 * HTF * 1024;
    constexpr int BI = SPW * SLAB_F, XB = BI + SPW * 128;               // bias [SPW][128] | exchange [4 SPW][1024] | flags [32]
    constexpr int FL = XB + (SPW == 2 ? 8 * 1024 : 0);
    constexpr int N2 = 32 * HT, E = 96 * N2 + 96, N2T = 32 * HTF, ET = 96 * N2T + 96;
    // (the wave index through readfirstlane: everything derived from it -- slab, chunk, base pointers, the sl branches -- is then
    //  provably wave-uniform: scalar registers and scalar branches instead of 64-bit per-lane addresses and exec masks)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // partners (same q, the two slabs) sit on DIFFERENT SIMDs (wave w runs on SIMD w % 4): the two waves that share a SIMD
    // then belong to different pairs and drift apart, so one's VALU phase overlaps the other's MFMA phase
    const int sl = SPW == 1 ? 0 : wave >> 2, q = (wave + sl) & 3;
    int group, range;
    {
        const int L = blockIdx.x, G = k.n_groups;
        if (k.xcd_map) { const int i = L >> 3; group = i % G; range = (i / G) * 8 + (L & 7); }
        else { group = L % G; range = L / G; }
    }
    const int slab = group * SPW + sl;
    const bool slab_ok = slab < k.n_slabs;
    {
        const int tid = threadIdx.x & 255;
        f32x4 *dst = reinterpret_cast<f32x4 *>(smem + sl * SLAB_F + FWo);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 *src = reinterpret_cast<const f32x4 *>(k.wf + (size_t)(slab_ok ? slab : 0) * 3 * HTF * 1024);
        for (int i = tid; i < 3 * HTF * 256; i += 256) dst[i] = slab_ok ? src[i] : zero;
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            const f32x4 *s2 = reinterpret_cast<const f32x4 *>(k.wb + ((size_t)(M0 + m) * 3 * k.n_slabs + 3 * (slab_ok ? slab : 0)) * 1024);
            f32x4 *d2 = reinterpret_cast<f32x4 *>(smem + sl * SLAB_F + BWo + m * 3 * 1024);
            for (int i = tid; i < 3 * 256; i += 256) d2[i] = slab_ok ? s2[i] : zero;
        }
        if (SPW == 2 && threadIdx.x < 32) reinterpret_cast<int *>(smem + FL)[threadIdx.x] = 0;
        if (tid < 96)
            smem[BI + sl * 128 + tid] = slab_ok ? k.wf[(size_t)k.n_slabs * 3 * HTF * 1024 + slab * 96 + tid] : 0.f;
    }
    __syncthreads();
    const wptr w = make_wptr(sl * SLAB_F, lane);
    const int bias_off = BI + sl * 128 - sl * SLAB_F;                   // relative to w
    const sel_t sel = make_sel(lane);
    const int j = lane & 31, hh = lane >> 5;
    f32x16 A[3][HT];
    float bsum[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int m = 0; m < HT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) A[t][m][r] = 0.f;
    const int ci = 2 * slab + hh;                                       // this lane's transformed column (index into live)
    const bool col_ok = ci < k.n_live;
    const int col = col_ok ? (k.live_idx ? k.live_idx[ci] : k.l0 + ci) : 0;
    uint64_t any_bad = 0;
    const float sc_in = slab_scale_in(k.scale), sc_out = slab_scale_out(k.scale);
    const int c_begin = (int)((int64_t)k.n_chunks * range / k.n_ranges), c_end = (int)((int64_t)k.n_chunks * (range + 1) / k.n_ranges);
    const int iters = (c_end - c_begin + 3) >> 2;                      // passes: uniform over the workgroup
    for (int it = 0; it < iters; ++it) {
        const int c = c_begin + q + 4 * it;
        const bool chunk_ok = c < c_end;
        rng_t rg{0};
        // chunk base pointers are wave-uniform; lanes add 32-bit offsets.  A row past the end reads the chunk's last real row
        // instead (an absent chunk: the range's first): its parameter gradients are forced to zero below, so whatever
        // finite h it carries contributes nothing, and its dh is never stored by the reduce kernel.
        const int cc = chunk_ok ? c : c_begin;
        const int64_t row0 = (int64_t)cc * 32;
        const int n_here = (int)((k.n_rows - row0) < 32 ? (k.n_rows - row0) : 32);
        const bool row_ok = chunk_ok && j < n_here;
        const bool valid = row_ok && col_ok;
        const int jc = j < n_here ? j : n_here - 1;
        const float *hb = k.h + row0 * k.ld_h;
        const float *xb_ = k.x + row0 * k.dim, *gb_ = k.gout + row0 * k.dim, *lb_ = k.gldj + row0;
        const uint32_t hoff = (uint32_t)jc * (uint32_t)k.ld_h + 4u * hh, xoff = (uint32_t)jc * (uint32_t)k.dim + (uint32_t)col;
        // ---- h -> fp16 x 3 fragments; the slab's parameters ----------------------------------------------------------
        btile<1> bh[HT];
        tile<1> acc[3];
        float xv, Ao, Al;
        [[maybe_unused]] float xo = 0.f;
        if constexpr (HTF == HT) {
    #pragma unroll
            for (int m = 0; m < HT; ++m) {
                tile<1> hid;
    #pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f0 = 32 * m + 8 * g + 4 * hh;
                    const float *p = hb + (hoff + 32u * m + 8u * g);
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (HFULL) v = *reinterpret_cast<const f32x4 *>(p);
                    else {
                        if (f0 + 0 < k.H) v.x = p[0];
                        if (f0 + 1 < k.H) v.y = p[1];
                        if (f0 + 2 < k.H) v.z = p[2];
                        if (f0 + 3 < k.H) v.w = p[3];
                    }
                    hid.v[0][4 * g + 0] = v.x; hid.v[0][4 * g + 1] = v.y; hid.v[0][4 * g + 2] = v.z; hid.v[0][4 * g + 3] = v.w;
                }
                bh[m] = make_btile<1>(hid, rg);
            }
            const float xl = xb_[xoff], gol = gb_[xoff], gll = lb_[jc];
            if constexpr (CUBIC) xo = (k.xout + row0 * k.dim)[xoff];
            xv = valid ? xl : k.bottom;
            Ao = valid ? gol * sc_in : 0.f;
            Al = valid ? gll * (k.ldj_scale * sc_in) : 0.f;
            // p = W2_slab h + b2: the three tiles (widths | heights | derivatives) are independent accumulation chains, issued
            // round-robin -- an MFMA onto the previous one's result waits for it, and the A fragments come from LDS
    #pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = load_cfrag<1>(w.cb, bias_off + t * 32);
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    afrag a[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) a[t] = load_afrag(w.wb, FWo + (t * HT + m) * 1024, sx);
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].lo, bh[m].hi[0][sx], acc[t].v[0]);      // smallest terms first
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bh[m].lo[0][sx], acc[t].v[0]);
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bh[m].hi[0][sx], acc[t].v[0]);
                    __builtin_amdgcn_sched_barrier(0);
                }
        } else {
            const float xl = xb_[xoff], gol = gb_[xoff], gll = lb_[jc];
            if constexpr (CUBIC) xo = (k.xout + row0 * k.dim)[xoff];
            xv = valid ? xl : k.bottom;
            Ao = valid ? gol * sc_in : 0.f;
            Al = valid ? gll * (k.ldj_scale * sc_in) : 0.f;
            // p = W2_slab h + b2: the three tiles (widths | heights | derivatives) are independent accumulation chains, issued
            // round-robin -- an MFMA onto the previous one's result waits for it, and the A fragments come from LDS.  One hidden tile at a
            // time: its fragments stay (bh) only when this launch also forms dh / dW2 for it
    #pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = load_cfrag<1>(w.cb, bias_off + t * 32);
    #pragma unroll
            for (int mf = 0; mf < HTF; ++mf) {
                tile<1> hid;
    #pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f0 = 32 * mf + 8 * g + 4 * hh;
                    const float *p = hb + (hoff + 32u * mf + 8u * g);
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (HFULL) v = *reinterpret_cast<const f32x4 *>(p);
                    else {
                        if (f0 + 0 < k.H) v.x = p[0];
                        if (f0 + 1 < k.H) v.y = p[1];
                        if (f0 + 2 < k.H) v.z = p[2];
                        if (f0 + 3 < k.H) v.w = p[3];
                    }
                    hid.v[0][4 * g + 0] = v.x; hid.v[0][4 * g + 1] = v.y; hid.v[0][4 * g + 2] = v.z; hid.v[0][4 * g + 3] = v.w;
                }
                const btile<1> bcur = make_btile<1>(hid, rg);
                if (mf >= M0 && mf < M0 + HT) bh[(mf >= M0 && mf < M0 + HT) ? mf - M0 : 0] = bcur;      // (mf is a constant once unrolled)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    afrag a[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) a[t] = load_afrag(w.wb, FWo + (t * HTF + mf) * 1024, sx);
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].lo, bcur.hi[0][sx], acc[t].v[0]);      // smallest terms first
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bcur.lo[0][sx], acc[t].v[0]);
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bcur.hi[0][sx], acc[t].v[0]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // ---- the spline's reverse mode on the lane's own element: parameters -> their gradients, in place ---------------
        float gxe;
        if constexpr (CUBIC)
            gxe = cubic_inverse_bwd_regs<KC>(acc[0].v[0], acc[1].v[0], acc[2].v[0], k.K, xv, xo, Ao, Al, k.left, k.right, valid);
        else
            gxe = rqs_inverse_bwd_regs<KC>(acc[0].v[0], acc[1].v[0], acc[2].v[0], k.K, xv, Ao, Al, k.left, k.right, k.bottom, k.top, valid);
        btile<1> bd[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bd[t] = make_btile<1>(acc[t], rg);
        if (valid) (k.gx + row0 * k.dim)[xoff] = rng_bad_sample(rg, lane) ? __builtin_nanf("") : gxe * sc_out;
        any_bad |= rg.bad;
        __builtin_amdgcn_sched_barrier(0);
        // ---- dh partial = W2_slab^T dp ---------------------------------------------------------------------------
        float *dst = k.dh_part + ((size_t)group * k.n_chunks + cc) * (HTF * 1024) + M0 * 1024;
        tile<1> dh[HT];
#pragma unroll
        for (int m = 0; m < HT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) dh[m].v[0][r] = 0.f;
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {              // the HT chains round-robin, as in the parameter GEMM
                afrag a[HT];
#pragma unroll
                for (int m = 0; m < HT; ++m) a[m] = load_afrag(w.wb, BWo + (m * 3 + t) * 1024, sx);
#pragma unroll
                for (int m = 0; m < HT; ++m) dh[m].v[0] = mfma(a[m].lo, bd[t].hi[0][sx], dh[m].v[0]);
#pragma unroll
                for (int m = 0; m < HT; ++m) dh[m].v[0] = mfma(a[m].hi, bd[t].lo[0][sx], dh[m].v[0]);
#pragma unroll
                for (int m = 0; m < HT; ++m) dh[m].v[0] = mfma(a[m].hi, bd[t].hi[0][sx], dh[m].v[0]);
                __builtin_amdgcn_sched_barrier(0);
            }
        if constexpr (SPW == 1) {
            if (chunk_ok) {
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 v = {dh[m].v[0][4 * g], dh[m].v[0][4 * g + 1], dh[m].v[0][4 * g + 2], dh[m].v[0][4 * g + 3]};
                        reinterpret_cast<f32x4 *>(dst + m * 1024)[g * 64 + lane] = v;
                    }
            }
        } else {
            // the pair (slab 2g, slab 2g+1) of a chunk: wave `sl` hands the tile it does NOT own to its partner and owns
            // hidden tile (sl % HT): with HT = 2 each wave adds and stores one tile, with HT = 1 the first slab's wave does
            constexpr int OWN_SPLIT = HT == 2;
            const int own = sl * 4 + q, oth = (1 - sl) * 4 + q;
            f32x4 *xb = reinterpret_cast<f32x4 *>(smem + XB + own * 1024);
            f32x4 *xp = reinterpret_cast<f32x4 *>(smem + XB + oth * 1024);
            int *ready = reinterpret_cast<int *>(smem + FL), *ack = ready + 8;
            const int give = OWN_SPLIT ? 1 - sl : 0;            // tile handed over (HT = 1: slab 1 gives its only tile)
            if (OWN_SPLIT || sl == 1) {
                flag_wait_ge(ack + own, it);                    // the partner has read the tile of the previous pass
#pragma unroll
                for (int m = 0; m < HT; ++m)
                    if (m == give) {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            xb[g * 64 + lane] = f32x4{dh[m].v[0][4 * g], dh[m].v[0][4 * g + 1], dh[m].v[0][4 * g + 2], dh[m].v[0][4 * g + 3]};
                    }
                flag_set(ready + own, it + 1);
            }
            if (OWN_SPLIT || sl == 0) {
                flag_wait_ge(ready + oth, it + 1);
#pragma unroll
                for (int m = 0; m < HT; ++m)
                    if (m == (OWN_SPLIT ? sl : 0)) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 o = xp[g * 64 + lane];
                            const f32x4 v = {dh[m].v[0][4 * g] + o.x, dh[m].v[0][4 * g + 1] + o.y, dh[m].v[0][4 * g + 2] + o.z,
                                             dh[m].v[0][4 * g + 3] + o.w};
                            if (chunk_ok) reinterpret_cast<f32x4 *>(dst + m * 1024)[g * 64 + lane] = v;
                        }
                    }
                flag_set(ack + oth, it + 1);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- dW2_slab += dp^T h (contraction over this wave's 32 rows on the matrix pipe) --------------------------------
        tfrag th[HT];
        float dummy = 0.f;
#pragma unroll
        for (int m = 0; m < HT; ++m) th[m] = turn_tile(bh[m], sel, dummy);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const tfrag td = turn_tile(bd[t], sel, bsum[t]);
#pragma unroll
            for (int m = 0; m < HT; ++m) contract(td, th[m], A[t][m]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (any_bad != 0 && lane == 0 && k.flags != nullptr)
        __hip_atomic_fetch_or(k.flags, SX_FLAG_F16_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // ---- one partial per slab and workgroup: its 4 waves add their tiles in LDS by turns (row-major [96][32 HT] | [96]) ----
    __syncthreads();
    float *red = smem + sl * SLAB_F;
    for (int wv = 0; wv < 4; ++wv) {
        if (q == wv) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int e = (32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh) * N2 + 32 * m + j;
                        red[e] = (wv == 0 ? 0.f : red[e]) + A[t][m][r];
                    }
                const float tb = bsum[t] + __shfl_xor(bsum[t], 32, 64);
                if (hh == 0) { const int e = 96 * N2 + 32 * t + j; red[e] = (wv == 0 ? 0.f : red[e]) + tb; }
            }
        }
        __syncthreads();
    }
    if (slab_ok) {
        float *dst = k.w_part + ((size_t)slab * k.n_ranges + range) * ET;
        if constexpr (HTF == HT) {
            for (int e = threadIdx.x & 255; e < E; e += 256) dst[e] = red[e];
        } else {
            // this launch's hidden columns of the [96][32 HTF] rows; the bias sums once (they do not depend on the hidden tile)
            for (int e = threadIdx.x & 255; e < 96 * N2; e += 256) dst[(e / N2) * N2T + 32 * M0 + (e % N2)] = red[e];
            if (M0 == 0)
                for (int e = threadIdx.x & 255; e < 96; e += 256) dst[96 * N2T + e] = red[96 * N2 + e];
        }
    }
}

// dW2 / db2 rows of the slabs: sum of the per-range partials, scattered to the parameter's rows (slot_rows < 0: padding)
__global__ __launch_bounds__(256) void rqs_slab_w_reduce_kernel(const float *__restrict__ part, int n_ranges, int N2, int H,
                                                                const int32_t *__restrict__ slot_rows, float *__restrict__ dW,
                                                                int64_t ldw, float *__restrict__ db,
                                                                const float *__restrict__ scale) {
    const int E = 96 * N2 + 96;
    const int e = blockIdx.x * 256 + threadIdx.x, slab = blockIdx.y;
    if (e >= E) return;
    const float *src = part + (size_t)slab * n_ranges * E + e;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = 0;
    for (; p + 3 < n_ranges; p += 4) {
        s0 += src[(size_t)p * E];
        s1 += src[(size_t)(p + 1) * E];
        s2 += src[(size_t)(p + 2) * E];
        s3 += src[(size_t)(p + 3) * E];
    }
    for (; p < n_ranges; ++p) s0 += src[(size_t)p * E];
    const float t = ((s0 + s1) + (s2 + s3)) * slab_scale_out(scale);
    if (e < 96 * N2) {
        const int row = slot_rows[slab * 96 + e / N2], colh = e % N2;
        if (row >= 0 && colh < H) dW[(int64_t)row * ldw + colh] = t;
    } else {
        const int row = slot_rows[slab * 96 + (e - 96 * N2)];
        if (row >= 0) db[row] = t;
    }
}

// dL/dh [N, H] row-major = sum over the slabs of the fragment-order partials
template <int HT>
__global__ __launch_bounds__(256) void rqs_slab_dh_reduce_kernel(const float *__restrict__ part, int n_slabs, int n_chunks,
                                                                 int64_t n_rows, int H, float *__restrict__ gh, int64_t ld,
                                                                 const float *__restrict__ scale, const float *__restrict__ h_tanh,
                                                                 int64_t ld_h) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;         // one 16 B piece: (chunk, m, g, lane)
    const int64_t total = (int64_t)n_chunks * HT * 256;
    if (idx >= total) return;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(part) + idx;
    f32x4 s = src[0];
    for (int p = 1; p < n_slabs; ++p) {
        const f32x4 v = src[(size_t)p * total];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float us = slab_scale_out(scale);
    s.x *= us; s.y *= us; s.z *= us; s.w *= us;
    const int lane = (int)(idx & 63), g = (int)((idx >> 6) & 3), m = (int)((idx >> 8) % HT);
    const int64_t c = idx / (HT * 256);
    const int64_t row = c * 32 + (lane & 31);
    const int f0 = 32 * m + 8 * g + 4 * (lane >> 5);
    if (row >= n_rows) return;
    float *dst = gh + row * ld + f0;
    const bool vec = f0 + 3 < H && ((ld | ld_h) & 3) == 0 && ((reinterpret_cast<uintptr_t>(gh) | reinterpret_cast<uintptr_t>(h_tanh)) & 15) == 0;
    if (vec) {                                  // whole 16-byte pieces (H a multiple of 4, aligned rows): one load, one store
        if (h_tanh != nullptr) {                // h = tanh(a): dL/da = dL/dh (1 - h^2)
            const f32x4 hv = *reinterpret_cast<const f32x4 *>(h_tanh + row * ld_h + f0);
            s.x *= 1.f - hv.x * hv.x; s.y *= 1.f - hv.y * hv.y; s.z *= 1.f - hv.z * hv.z; s.w *= 1.f - hv.w * hv.w;
        }
        *reinterpret_cast<f32x4 *>(dst) = s;
        return;
    }
    if (h_tanh != nullptr) {
        const float *hp = h_tanh + row * ld_h + f0;
        if (f0 + 0 < H) s.x *= 1.f - hp[0] * hp[0];
        if (f0 + 1 < H) s.y *= 1.f - hp[1] * hp[1];
        if (f0 + 2 < H) s.z *= 1.f - hp[2] * hp[2];
        if (f0 + 3 < H) s.w *= 1.f - hp[3] * hp[3];
    }
    if (f0 + 0 < H) dst[0] = s.x;
    if (f0 + 1 < H) dst[1] = s.y;
    if (f0 + 2 < H) dst[2] = s.z;
    if (f0 + 3 < H) dst[3] = s.w;
}

// ------------------------------------------------------------------------------------------------------------------------
// Backward of the conditioner's FIRST layer behind the slab kernel, for Linear - Tanh - Linear conditioners without a
// latent input (cfg 3):  a = W1m x + b1 (W1m = W1 with the coupling mask folded into its columns), h = tanh(a).
// One pass over the rows does what took a reduce kernel, a tanh backward, two library GEMMs, a weight-gradient kernel, a
// clone and an add: per 32-row chunk it sums the slab groups' dh partials (fragment order = C tiles), applies 1 - h^2,
// forms dz = W1m^T da by MFMA and writes  gx[:, conditioning columns] = gout + dz  (the transformed columns were written by
// the slab kernel), and contracts dW1m += da x^T over the rows on the matrix pipe (turn / contract, as the slab kernel).
// Everything stays in the power-of-two scaled domain of the slab kernel until it is stored.
struct l1_args {
    const float *part;            // [n_groups][n_chunks][HT][1024] dh partials
    const float *h, *x, *gout;    // [N, ld_h], [N, dim], [N, dim]
    const float *w1t;             // sx_pack_linear(W1m, transpose = 1): [XT][HT][1024]
    float *gx;                    // [N, dim]
    float *w_part;                // [gridDim][32 HT * 32 XT + 32 HT]
    const float *scale;
    uint32_t *flags;
    int64_t n_rows, ld_h;
    int n_groups, n_chunks, dim, H;
    uint32_t cond_mask[2];        // bit c of word t: column 32 t + c is a conditioning column (receives gout + dz)
};
// (HT = 3, 4: the HT x XT accumulator tiles + the partial sums need more than 256 registers -- one workgroup per CU)
template <int HT, int XT>
__global__ __launch_bounds__(256, HT <= 2 ? 2 : 1) void rqs_slab_l1_bwd_kernel(const l1_args k) {
    constexpr int N1 = 32 * XT, E1 = 32 * HT * N1 + 32 * HT;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(k.w1t);
        f32x4 *dst = reinterpret_cast<f32x4 *>(smem);
        for (int i = threadIdx.x; i < XT * HT * 256; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const wptr w = make_wptr(0, lane);
    const sel_t sel = make_sel(lane);
    const int j = lane & 31, hh = lane >> 5;
    f32x16 Aw[HT][XT];
    float bsum[HT];
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        bsum[m] = 0.f;
#pragma unroll
        for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Aw[m][xt][r] = 0.f;
    }
    const float sc_out = slab_scale_out(k.scale);
    const bool vec = (k.dim % 4 == 0) && (k.ld_h % 4 == 0) && k.H == 32 * HT && k.dim == 32 * XT &&
                     ((reinterpret_cast<uintptr_t>(k.h) | reinterpret_cast<uintptr_t>(k.x) | reinterpret_cast<uintptr_t>(k.gout) |
                       reinterpret_cast<uintptr_t>(k.gx)) & 15) == 0;
    uint64_t any_bad = 0;
    const size_t gstride = (size_t)k.n_chunks * HT * 1024;
    for (int c = blockIdx.x * 4 + wave; c < k.n_chunks; c += gridDim.x * 4) {
        rng_t rg{0};
        const int64_t row0 = (int64_t)c * 32;
        const int n_here = (int)((k.n_rows - row0) < 32 ? (k.n_rows - row0) : 32);
        const bool row_ok = j < n_here;
        const int jc = row_ok ? j : n_here - 1;
        // ---- da = (sum of the groups' dh partials) (1 - h^2), C-fragment tiles (hidden x samples) ---------------------------------
        btile<1> bga[HT];
        if (k.n_groups <= 8) {
            // up to eight groups (cfg 3: exactly eight): the 4 HT batches of a chunk -- one 16-byte piece of every group's partial
            // plus the matching piece of h -- are software-pipelined: batch b + 1 is requested before batch b is summed, so two
            // batches (16 KB per wave) are always in flight instead of one with a full drain in between (the kernel is a stream
            // of 64 KB per chunk; 0.196 -> see DESIGN.md 4.3.1)
            // GROUP-major: a group's partial tile of this chunk is 4 HT KB contiguous -- a half-batch is four of its 1 KB pieces
            // (one DRAM-friendly run instead of one piece from each of eight tiles 64 MB apart), summed into 4 HT running pieces;
            // the next half-batch is requested before the current one is added (no drain between them)
            constexpr int NP = 4 * HT;                         // 16-byte pieces per lane and group tile
            f32x4 v[2][4], sum[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) sum[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *src0 = k.part + (size_t)c * HT * 1024 + lane * 4;
            auto issue = [&](int hb, f32x4 (&vv)[4]) {          // hb = p * (NP / 4) + quarter
                const int p = hb / (NP / 4), q0 = 4 * (hb % (NP / 4));
                const float *src = src0 + (size_t)(p < k.n_groups ? p : k.n_groups - 1) * gstride;
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) vv[qq] = *reinterpret_cast<const f32x4 *>(src + (q0 + qq) * 256);
            };
            constexpr int NHB = 8 * (NP / 4);
            issue(0, v[0]);
#pragma unroll
            for (int hb = 0; hb < NHB; ++hb) {
                if (hb + 1 < NHB) issue(hb + 1, v[(hb + 1) & 1]);
                const int p = hb / (NP / 4), q0 = 4 * (hb % (NP / 4));
                if (p < k.n_groups) {
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        sum[q0 + qq].x += v[hb & 1][qq].x; sum[q0 + qq].y += v[hb & 1][qq].y;
                        sum[q0 + qq].z += v[hb & 1][qq].z; sum[q0 + qq].w += v[hb & 1][qq].w;
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                tile<1> ga;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f0 = 32 * m + 8 * g + 4 * hh;
                    const float *hp = k.h + (row0 + jc) * k.ld_h + f0;
                    f32x4 hv = {0.f, 0.f, 0.f, 0.f};
                    if (vec) hv = *reinterpret_cast<const f32x4 *>(hp);
                    else {
                        if (f0 + 0 < k.H) hv.x = hp[0];
                        if (f0 + 1 < k.H) hv.y = hp[1];
                        if (f0 + 2 < k.H) hv.z = hp[2];
                        if (f0 + 3 < k.H) hv.w = hp[3];
                    }
                    const f32x4 sm = sum[4 * m + g];
                    ga.v[0][4 * g + 0] = row_ok ? sm.x * (1.f - hv.x * hv.x) : 0.f;
                    ga.v[0][4 * g + 1] = row_ok ? sm.y * (1.f - hv.y * hv.y) : 0.f;
                    ga.v[0][4 * g + 2] = row_ok ? sm.z * (1.f - hv.z * hv.z) : 0.f;
                    ga.v[0][4 * g + 3] = row_ok ? sm.w * (1.f - hv.w * hv.w) : 0.f;
                }
                bga[m] = make_btile<1>(ga, rg);
            }
        } else
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            tile<1> ga;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // eight groups' pieces in flight at a time (a rolled loop would wait for each load before the next: the kernel
                // is a stream of 64 KB per chunk and nothing else hides the latency); groups past the end re-read the last one
                const float *src = k.part + ((size_t)c * HT + m) * 1024 + (g * 64 + lane) * 4;
                f32x4 sum = {0.f, 0.f, 0.f, 0.f};
                for (int p0 = 0; p0 < k.n_groups; p0 += 8) {
                    f32x4 v[8];
#pragma unroll
                    for (int pp = 0; pp < 8; ++pp) {
                        const int p = p0 + pp < k.n_groups ? p0 + pp : k.n_groups - 1;
                        v[pp] = *reinterpret_cast<const f32x4 *>(src + (size_t)p * gstride);
                    }
#pragma unroll
                    for (int pp = 0; pp < 8; ++pp)
                        if (p0 + pp < k.n_groups) { sum.x += v[pp].x; sum.y += v[pp].y; sum.z += v[pp].z; sum.w += v[pp].w; }
                }
                const int f0 = 32 * m + 8 * g + 4 * hh;
                const float *hp = k.h + (row0 + jc) * k.ld_h + f0;
                f32x4 hv = {0.f, 0.f, 0.f, 0.f};
                if (vec) hv = *reinterpret_cast<const f32x4 *>(hp);
                else {
                    if (f0 + 0 < k.H) hv.x = hp[0];
                    if (f0 + 1 < k.H) hv.y = hp[1];
                    if (f0 + 2 < k.H) hv.z = hp[2];
                    if (f0 + 3 < k.H) hv.w = hp[3];
                }
                ga.v[0][4 * g + 0] = row_ok ? sum.x * (1.f - hv.x * hv.x) : 0.f;
                ga.v[0][4 * g + 1] = row_ok ? sum.y * (1.f - hv.y * hv.y) : 0.f;
                ga.v[0][4 * g + 2] = row_ok ? sum.z * (1.f - hv.z * hv.z) : 0.f;
                ga.v[0][4 * g + 3] = row_ok ? sum.w * (1.f - hv.w * hv.w) : 0.f;
            }
            bga[m] = make_btile<1>(ga, rg);
        }
        // ---- x chunk as C tiles (columns x samples): the B side of the contraction ----------------------------------------------
        tfrag tx[XT];
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) {
            tile<1> xv;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * xt + 8 * g + 4 * hh;
                const float *xp = k.x + (row0 + jc) * k.dim + c0;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (vec) v = *reinterpret_cast<const f32x4 *>(xp);
                else {
                    if (c0 + 0 < k.dim) v.x = xp[0];
                    if (c0 + 1 < k.dim) v.y = xp[1];
                    if (c0 + 2 < k.dim) v.z = xp[2];
                    if (c0 + 3 < k.dim) v.w = xp[3];
                }
                xv.v[0][4 * g + 0] = v.x; xv.v[0][4 * g + 1] = v.y; xv.v[0][4 * g + 2] = v.z; xv.v[0][4 * g + 3] = v.w;
            }
            float dummy = 0.f;
            tx[xt] = turn_tile(make_btile<1>(xv, rg), sel, dummy);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- dz = W1m^T da;  gx[:, conditioning columns] = gout + dz ------------------------------------------------------------
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) {
            tile<1> dz;
#pragma unroll
            for (int r = 0; r < 16; ++r) dz.v[0][r] = 0.f;
#pragma unroll
            for (int m = 0; m < HT; ++m) gemm_tile<1>(w.wb, (xt * HT + m) * 1024, bga[m], dz);
            const uint32_t cm = k.cond_mask[xt];
            if (cm != 0u && row_ok) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c0 = 32 * xt + 8 * g + 4 * hh;
                    const uint32_t bits = (cm >> (8 * g + 4 * hh)) & 15u;
                    const size_t off = (size_t)(row0 + j) * k.dim + c0;
                    const bool bad = rng_bad_sample(rg, lane);
                    const float nanv = __builtin_nanf("");
                    if (vec && bits == 15u) {
                        const f32x4 go = *reinterpret_cast<const f32x4 *>(k.gout + off);
                        f32x4 o = {go.x + dz.v[0][4 * g] * sc_out, go.y + dz.v[0][4 * g + 1] * sc_out, go.z + dz.v[0][4 * g + 2] * sc_out,
                                   go.w + dz.v[0][4 * g + 3] * sc_out};
                        if (bad) o = f32x4{nanv, nanv, nanv, nanv};
                        *reinterpret_cast<f32x4 *>(k.gx + off) = o;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (((bits >> e) & 1u) && c0 + e < k.dim) k.gx[off + e] = bad ? nanv : k.gout[off + e] + dz.v[0][4 * g + e] * sc_out;
                    }
                }
            }
        }
        any_bad |= rg.bad;
        __builtin_amdgcn_sched_barrier(0);
        // ---- dW1m += da x^T, db1 += sum da (over this wave's rows) -----------------------------------------------------------------
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            const tfrag ta = turn_tile(bga[m], sel, bsum[m]);
#pragma unroll
            for (int xt = 0; xt < XT; ++xt) contract(ta, tx[xt], Aw[m][xt]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (any_bad != 0 && lane == 0 && k.flags != nullptr)
        __hip_atomic_fetch_or(k.flags, SX_FLAG_F16_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // ---- one partial per workgroup, wgrad_reduce_kernel's layout: [32 HT x 32 XT | 32 HT], already unscaled ------------------------
    __syncthreads();
    float *red = smem;
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int m = 0; m < HT; ++m) {
#pragma unroll
                for (int xt = 0; xt < XT; ++xt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int e = (32 * m + (r & 3) + 8 * (r >> 2) + 4 * hh) * N1 + 32 * xt + j;
                        red[e] = (wv == 0 ? 0.f : red[e]) + Aw[m][xt][r];
                    }
                const float tb = bsum[m] + __shfl_xor(bsum[m], 32, 64);
                if (hh == 0) { const int e = 32 * HT * N1 + 32 * m + j; red[e] = (wv == 0 ? 0.f : red[e]) + tb; }
            }
        }
        __syncthreads();
    }
    float *dst = k.w_part + (size_t)blockIdx.x * E1;
    for (int e = threadIdx.x; e < E1; e += 256) dst[e] = red[e] * sc_out;
}

// ------------------------------------------------------------------------------------------------------------------------
// FORWARD slab pass (inference and the training forward): (y, row log-det) of a rational-quadratic spline COUPLING from the
// conditioner's last hidden activation h [N, H], H <= 256 -- the tier that answers where the one-launch flow program does not reach
// (hidden layers beyond 128 units: stribor/net/mlp.py:48-58 and flows/spline.py:76-87 take any width).  The layer-by-layer tier
// materialised the [N, n_live (3K-1)] parameter tensor (1.6 GB per layer and 2^18 rows on a cfg-3-shaped coupling: written by one MLP
// program, read and re-written by the program of the next hidden chunk, read by the spline kernel: 1.7 ms per layer); here, tiled like
// the slab backward above, it never exists:
//   * a workgroup (8 waves, two per SIMD) owns a SLAB -- the 3K-1 parameter rows of TWO transformed columns, three 32-row MFMA tiles
//     (widths | heights | derivatives) x HT hidden tiles, 12 KB x HT of LDS for the whole launch -- and walks a range of the rows;
//   * a wave takes 32 rows at a time and streams h through the k loop one 32-unit tile at a time (load -> fp16 x 3 split -> 18 MFMAs
//     into the three accumulator tiles; the next tile's loads are issued before the current tile's MFMAs), so the hidden width is a
//     RUN-TIME loop count: one kernel for every width;
//   * in C-fragment order lane (sample, half) then holds exactly the 3K-1 parameters of its element (sample, column 2 slab + half)
//     and evaluates the spline on registers with static indices (the forward part of rqs_inverse_bwd_regs' arithmetic: hardware
//     exp / rcp / log, selects for the bin; rational_quadratic_spline.py:101-107,180-248, search_sorted.py:4-5);
//   * the row's log-det is a sum over the slabs: each slab writes one partial per row, a second kernel adds them in slab order
//     (deterministic; n_slabs x 4 B per row).
// HBM per row and layer: h (128 B x HT, L2-resident across the slabs of an XCD), x and y of the transformed columns, 4 B per slab.
struct slabf_args {
    const float *x, *h;                 // x [N, dim]; h [N, ld_h] (H valid features)
    const float *wf;                    // sx_pack_linear(W2 rows by slot): [3 n_slabs][HT][1024] + bias [3 n_slabs][32]
    float *y;                           // [N, dim]: the transformed columns are written
    float *ldj_part;                    // [n_slabs][N] or null
    const int32_t *live_idx;
    const int32_t *pass_idx;            // the n_pass columns the coupling leaves alone (y = x there), or null: the caller fills them
    uint32_t *flags;
    int64_t n_rows, ld_h;
    int l0, n_live, n_pass, K, dim, H, HT, n_slabs, n_chunks, n_ranges, xcd_map, ref_ldj;
    float left, right, bottom, top, log_span;
};

// One element on registers: Sp = the SEARCHED side's K bin parameters (REV: heights, else widths), Op = the other side's, Dp the
// K - 1 knot derivatives; [slo, shi] / [olo, ohi] the two sides' intervals.  -> out, log|d out / d in| (REV: of the inverse).
// `hk.at<H>(ties...)`, H = 0..49, is called every ~8 vector instructions (three times in the max loop, once per exp and per knot, five
// times in the derivative pick, ten times in the rational-quadratic itself): the pipelined kernel issues ONE MFMA of the NEXT chunk's
// parameter GEMM -- 32 cycles of the matrix pipe = 8 vector issue slots -- from each, and the MFMAs the evaluation cannot cover
// behind it.  (An MFMA that finds the matrix pipe busy holds the SIMD's vector issue port until the pipe frees -- for the other wave of
// the SIMD as well --, so MFMAs issued back to back with vector work behind them overlap with a third of it at best: SLABF_NE.)
#define SLABF_NE 50
// (`tie`: a value the evaluation has just produced.  It passes through an empty volatile asm in front of the unit's MFMAs and the
//  accumulators through one behind them: volatile asms keep their order, so neither the optimizer nor the scheduler can gather the
//  MFMAs into one clump and the vector work into another -- which is what both do with independent instruction streams.)
struct slabf_nohook {
    template <int H, class... T> __device__ __forceinline__ void at(T &...) {}
};
template <int N, class Hook>
struct slabf_hook_seq {           // hk.at<B>(), hk.at<B + 1>() ... from an unrolled loop (the index must be a constant expression)
    template <int B, class... T> static __device__ __forceinline__ void call(Hook &hk, int k, T &...tie) {
        if constexpr (N > 0) {
            if (k == 0) hk.template at<B>(tie...);
            else slabf_hook_seq<N - 1, Hook>::template call<B + 1>(hk, k - 1, tie...);
        }
    }
};
// rqs_close's points -> the slots 43..46 of a slabf hook
template <class Hook>
struct slabf_close_hook {
    Hook &hk;
    template <int Y, class... T> __device__ __forceinline__ void at(float &v, T &...) {
        constexpr int slot = (Y == RQS_Y_DISC || Y == RQS_Y_THETA) ? 43 : (Y == RQS_Y_ROOT || Y == RQS_Y_NUM) ? 44 : Y == RQS_Y_DEN ? 45 : Y == RQS_Y_DNUM ? 46 : -1;
        if constexpr (slot >= 0) hk.template at<slot>(v);
    }
};
template <int KC, bool REV, class Hook>
__device__ __forceinline__ void rqs_slab_eval(rqsb_f16v &Sp, rqsb_f16v &Op, const rqsb_f16v &Dp, int K, float xv, float slo, float shi,
                                              float olo, float ohi, float &out, float &ljd, Hook &hk) {
    constexpr float LOG2E = 1.44269504088896341f, LN2 = 0.69314718055994531f;
    const int Kn = KC ? KC : K;
    const float norm = 1.f - RQS_MIN_BIN * (float)Kn;
    const float span_s = shi - slo, span_o = ohi - olo;
    const bool inside = (xv >= slo) && (xv <= shi);                 // :71 closed interval
    const float xin = inside ? xv : slo;
    float ms = Sp[0], mo = Op[0];
#pragma unroll
    for (int k = 1; k < 16; ++k)
        if (KC ? (k < KC) : true) {
            const bool used = KC ? true : (k < K);
            ms = used ? fmaxf(ms, Sp[k]) : ms;
            mo = used ? fmaxf(mo, Op[k]) : mo;
            if (k % 5 == 0) slabf_hook_seq<3, Hook>::template call<0>(hk, k / 5 - 1, ms, mo);
        }
    float ss = 0.f, so = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (KC ? (k < KC) : true) {
            const bool used = KC ? true : (k < K);
            const float es = used ? __builtin_amdgcn_exp2f((Sp[k] - ms) * LOG2E) : 0.f;
            const float eo = used ? __builtin_amdgcn_exp2f((Op[k] - mo) * LOG2E) : 0.f;
            Sp[k] = es;
            Op[k] = eo;
            ss += es;
            so += eo;
            slabf_hook_seq<16, Hook>::template call<3>(hk, k, ss, so);
        }
    const float ns = norm * __builtin_amdgcn_rcpf(ss), no = norm * __builtin_amdgcn_rcpf(so);    // bin size_k = MIN + e_k n (:101-105)
    // one sweep over the knots: the searched side's are compared with the input (search_sorted.py:4-5: the last knot carries + eps),
    // both sides' cumulative sums at the bin (last knot <= input) and behind it (first knot > input) are kept
    int b = 0;
    float cs = 0.f, co = 0.f, co_b = 0.f, co_n = 0.f, ks_b = slo, ks_n = shi;
    bool have_next = false;
#pragma unroll
    for (int j = 1; j <= 16; ++j)
        if (KC ? (j <= KC) : true) {
            const bool used = KC ? true : (j <= K);
            const bool last = (j == Kn);
            cs += fmaf(Sp[j - 1], ns, RQS_MIN_BIN);
            co += fmaf(Op[j - 1], no, RQS_MIN_BIN);
            const float ks = last ? shi : fmaf(span_s, cs, slo);    // ends pinned (:186-192)
            const bool ge = xin >= (last ? ks + RQS_EPS : ks);
            const bool take = used && ge && !last;
            const bool nxt = used && !ge && !have_next;
            b = take ? j : b;
            co_b = take ? co : co_b;
            ks_b = take ? ks : ks_b;
            co_n = nxt ? co : co_n;
            ks_n = nxt ? ks : ks_n;
            have_next = have_next || nxt;
            slabf_hook_seq<16, Hook>::template call<19>(hk, j - 1, cs, co, co_b, ks_b, co_n, ks_n, b);
        }
    const bool first = (b == 0), lastbin = (b + 1 == Kn);
    const float ko_b = first ? olo : fmaf(span_o, co_b, olo);
    const float ko_n = lastbin ? ohi : fmaf(span_o, co_n, olo);
    float u_b = RQS_BOUNDARY_DERIV, u_n = RQS_BOUNDARY_DERIV;
#pragma unroll
    for (int k = 0; k < 15; ++k)
        if (KC ? (k < KC - 1) : true) {
            const bool used = KC ? true : (k < Kn - 1);
            u_n = (used && b == k) ? Dp[k] : u_n;
            u_b = (used && b == k + 1) ? Dp[k] : u_b;
            if (k % 3 == 2) slabf_hook_seq<5, Hook>::template call<35>(hk, k / 3, u_n, u_b);
        }
    float d_b = rqs_knot_deriv(u_b);                                                                                      // :107
    hk.template at<40>(d_b);
    float d_n = rqs_knot_deriv(u_n);
    hk.template at<41>(d_n);
    const float cw_b = REV ? ko_b : ks_b, w_b = REV ? ko_n - ko_b : ks_n - ks_b;
    const float ch_b = REV ? ks_b : ko_b, h_b = REV ? ks_n - ks_b : ko_n - ko_b;
    float s_b = h_b * fast_rcp(w_b);
    hk.template at<42>(s_b);
    // the closing form of the one-launch tier with its clamps (sx_rqs_core.h); the two logs are combined BEFORE the ln 2 scaling here
    slabf_close_hook<Hook> ch{hk};
    const rqs_closed c = rqs_close<REV>(d_b, d_n, s_b, cw_b, w_b, ch_b, h_b, xin, ch);
    float l1 = __builtin_amdgcn_logf(REV ? c.den : c.dnum);
    hk.template at<47>(l1);
    float l2 = __builtin_amdgcn_logf(REV ? c.dnum : c.den);
    hk.template at<48>(l2);
    float l = REV ? (2.f * l1 - l2) * LN2 : (l1 - 2.f * l2) * LN2;
    hk.template at<49>(l);
    out = inside ? c.out : xv;                                      // :86-87 linear tails
    ljd = inside ? l : 0.f;
}

// The WIDE form, 17 <= K <= 32 bins: ONE transformed column per slab, its element in a lane PAIR -- lane (sample, half hh) holds bins
// 16 hh .. 16 hh + 15 of both sides in Sp / Op and knot derivatives 16 hh .. 16 hh + 15 (of the K - 1) in Dp.  rqs_slab_eval's
// arithmetic, split where the two halves meet:
//   * the soft-max maximum and sum are taken over both halves (max and + commute: both lanes hold the same bits);
//   * half 1's cumulative sums START from half 0's total, so every knot is the sequential cumsum's (a first sweep forms the totals);
//   * each half sweeps its own 16 knots with selects; the pair then exchanges b, co_b, ks_b, co_n, ks_n (the sweep's `have_next`
//     rides in b's bit 8) and the two derivatives each half picked for the combined bin -- thirteen 32-lane exchanges in all --,
//     and BOTH lanes run the closing form on identical values.
// The hooks are rqs_slab_eval's, at the same points.
template <bool REV, class Hook>
__device__ __forceinline__ void rqs_slab_eval_wide(rqsb_f16v &Sp, rqsb_f16v &Op, const rqsb_f16v &Dp, int K, int hh, float xv, float slo,
                                                   float shi, float olo, float ohi, float &out, float &ljd, Hook &hk) {
    constexpr float LOG2E = 1.44269504088896341f, LN2 = 0.69314718055994531f;
    const int k0 = 16 * hh;                                         // this half's first bin (and first knot derivative)
    const float norm = 1.f - RQS_MIN_BIN * (float)K;
    const float span_s = shi - slo, span_o = ohi - olo;
    const bool inside = (xv >= slo) && (xv <= shi);                 // :71 closed interval
    const float xin = inside ? xv : slo;
    float ms = Sp[0], mo = Op[0];                                   // (bin 16 exists: K >= 17)
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const bool used = k0 + k < K;
        ms = used ? fmaxf(ms, Sp[k]) : ms;
        mo = used ? fmaxf(mo, Op[k]) : mo;
        if (k % 5 == 0) slabf_hook_seq<3, Hook>::template call<0>(hk, k / 5 - 1, ms, mo);
    }
    ms = fmaxf(ms, __shfl_xor(ms, 32, 64));
    mo = fmaxf(mo, __shfl_xor(mo, 32, 64));
    float ss = 0.f, so = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool used = k0 + k < K;
        const float es = used ? __builtin_amdgcn_exp2f((Sp[k] - ms) * LOG2E) : 0.f;
        const float eo = used ? __builtin_amdgcn_exp2f((Op[k] - mo) * LOG2E) : 0.f;
        Sp[k] = es;
        Op[k] = eo;
        ss += es;
        so += eo;
        slabf_hook_seq<16, Hook>::template call<3>(hk, k, ss, so);
    }
    ss += __shfl_xor(ss, 32, 64);
    so += __shfl_xor(so, 32, 64);
    const float ns = norm * __builtin_amdgcn_rcpf(ss), no = norm * __builtin_amdgcn_rcpf(so);    // bin size_k = MIN + e_k n (:101-105)
    // where this half's cumulative sums start: half 0's total over its 16 bins, in the order the sweep below adds them
    float cs = 0.f, co = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        cs += fmaf(Sp[k], ns, RQS_MIN_BIN);
        co += fmaf(Op[k], no, RQS_MIN_BIN);
    }
    {
        const float cs0 = __shfl_xor(cs, 32, 64), co0 = __shfl_xor(co, 32, 64);
        cs = hh ? cs0 : 0.f;
        co = hh ? co0 : 0.f;
    }
    // this half's knots 16 hh + 1 .. 16 hh + 16: rqs_slab_eval's sweep
    int b = 0;
    float co_b = 0.f, co_n = 0.f, ks_b = slo, ks_n = shi;
    bool have_next = false;
#pragma unroll
    for (int j = 1; j <= 16; ++j) {
        const bool used = k0 + j <= K;
        const bool last = (k0 + j == K);
        cs += fmaf(Sp[j - 1], ns, RQS_MIN_BIN);
        co += fmaf(Op[j - 1], no, RQS_MIN_BIN);
        const float ks = last ? shi : fmaf(span_s, cs, slo);        // ends pinned (:186-192)
        const bool ge = xin >= (last ? ks + RQS_EPS : ks);
        const bool take = used && ge && !last;
        const bool nxt = used && !ge && !have_next;
        b = take ? k0 + j : b;
        co_b = take ? co : co_b;
        ks_b = take ? ks : ks_b;
        co_n = nxt ? co : co_n;
        ks_n = nxt ? ks : ks_n;
        have_next = have_next || nxt;
        slabf_hook_seq<16, Hook>::template call<19>(hk, j - 1, cs, co, co_b, ks_b, co_n, ks_n, b);
    }
    // the pair: the bin is the LAST knot taken (half 1's where it took one), the knot behind it the FIRST not taken (half 0's where it
    // has one) -- what one sweep over all the knots keeps
    {
        const int bx = b | (have_next ? 256 : 0);
        const int bx_o = __shfl_xor(bx, 32, 64);
        const float cob_o = __shfl_xor(co_b, 32, 64), ksb_o = __shfl_xor(ks_b, 32, 64);
        const float con_o = __shfl_xor(co_n, 32, 64), ksn_o = __shfl_xor(ks_n, 32, 64);
        const int bx0 = hh ? bx_o : bx, bx1 = hh ? bx : bx_o;
        const bool took1 = (bx1 & 255) != 0, next0 = (bx0 & 256) != 0;
        const bool b_own = took1 ? hh != 0 : hh == 0, n_own = next0 ? hh == 0 : hh != 0;
        b = (took1 ? bx1 : bx0) & 255;
        co_b = b_own ? co_b : cob_o;
        ks_b = b_own ? ks_b : ksb_o;
        co_n = n_own ? co_n : con_o;
        ks_n = n_own ? ks_n : ksn_o;
    }
    const bool first = (b == 0), lastbin = (b + 1 == K);
    const float ko_b = first ? olo : fmaf(span_o, co_b, olo);
    const float ko_n = lastbin ? ohi : fmaf(span_o, co_n, olo);
    // knot derivatives b - 1 and b of the K - 1: each from the half that holds it (index >> 4), the boundary value where there is none
    float u_b = RQS_BOUNDARY_DERIV, u_n = RQS_BOUNDARY_DERIV;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool used = k0 + k < K - 1;
        u_n = (used && b == k0 + k) ? Dp[k] : u_n;
        u_b = (used && b == k0 + k + 1) ? Dp[k] : u_b;
        if (k % 3 == 2) slabf_hook_seq<5, Hook>::template call<35>(hk, k / 3, u_n, u_b);
    }
    {
        const float un_o = __shfl_xor(u_n, 32, 64), ub_o = __shfl_xor(u_b, 32, 64);
        u_n = ((b >> 4) == hh) ? u_n : un_o;
        u_b = (((b - 1) >> 4) == hh) ? u_b : ub_o;
    }
    float d_b = rqs_knot_deriv(u_b);                                                                                      // :107
    hk.template at<40>(d_b);
    float d_n = rqs_knot_deriv(u_n);
    hk.template at<41>(d_n);
    const float cw_b = REV ? ko_b : ks_b, w_b = REV ? ko_n - ko_b : ks_n - ks_b;
    const float ch_b = REV ? ks_b : ko_b, h_b = REV ? ks_n - ks_b : ko_n - ko_b;
    float s_b = h_b * fast_rcp(w_b);
    hk.template at<42>(s_b);
    slabf_close_hook<Hook> ch{hk};
    const rqs_closed c = rqs_close<REV>(d_b, d_n, s_b, cw_b, w_b, ch_b, h_b, xin, ch);
    float l1 = __builtin_amdgcn_logf(REV ? c.den : c.dnum);
    hk.template at<47>(l1);
    float l2 = __builtin_amdgcn_logf(REV ? c.dnum : c.den);
    hk.template at<48>(l2);
    float l = REV ? (2.f * l1 - l2) * LN2 : (l1 - 2.f * l2) * LN2;
    hk.template at<49>(l);
    out = inside ? c.out : xv;                                      // :86-87 linear tails
    ljd = inside ? l : 0.f;
}

// The monotone CUBIC spline (util/cubic_spline.py:21-251, the reference's default spline_type) of one element on registers: Wp / Hp
// hold its K widths / heights (K <= 16, entries beyond K ignored), Dp[0..1] its two boundary-derivative parameters -- cubic_kernel's
// arithmetic (sx_rqs.hip, sx_cubic_core.h) with the parameters in MFMA accumulators: one sweep with selects keeps the sizes of
// bins b - 1, b, b + 1 (the Steffen slopes need the neighbours, :117-132), then the bin's cubic forward or its inverse (closed forms +
// Newton steps).  ref_ldj (a coupling's inverse_and_log_det_jacobian): the log-det is MINUS the FORWARD log-derivative re-evaluated
// at the inverted point (flow.py:42-47), as cubic_kernel's reference mode.
template <bool REV>
__device__ __forceinline__ void cubic_slab_eval(rqsb_f16v &Wp, rqsb_f16v &Hp, const rqsb_f16v &Dp, int K, float xv, float lower, float upper,
                                                float log_span, bool ref_ldj, bool valid, float &out, float &ljd) {
    const float norm = 1.f - CUBIC_MIN_BIN * (float)K;          // :104, :111
    const float span = upper - lower, inv_span = 1.0f / span;
    const bool inside = (xv >= lower) && (xv <= upper);          // :40 closed interval
    const float xin = ((inside ? xv : lower) - lower) * inv_span;        // :98-101
    float mw = Wp[0], mh = Hp[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const bool used = k < K;
        mw = used ? fmaxf(mw, Wp[k]) : mw;
        mh = used ? fmaxf(mh, Hp[k]) : mh;
    }
    float sw = 0.f, sh = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool used = k < K;
        const float ew = used ? fast_exp(Wp[k] - mw) : 0.f, eh = used ? fast_exp(Hp[k] - mh) : 0.f;
        Wp[k] = ew; Hp[k] = eh;
        sw += ew; sh += eh;
    }
    const float nw = norm * fast_rcp(sw), nh = norm * fast_rcp(sh);
    // normalised sizes, running cumsums (:103-115) and the bin search (search_sorted.py:4-5) in one sweep that also keeps the sizes of
    // bins b - 1, b, b + 1: the lower knot of bin k is compared (knot 0 = 0: the knots only grow)
    int b = 0;
    float cw_b = 0.f, ch_b = 0.f, w_b = 0.f, h_b = 0.f, w_m = 1.f, h_m = 1.f, w_p = 1.f, h_p = 1.f;
    float cw = 0.f, ch = 0.f, w_last = 1.f, h_last = 1.f;
    bool need_next = false;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool used = k < K;
        const float wk = CUBIC_MIN_BIN + nw * Wp[k];
        const float hk = CUBIC_MIN_BIN + nh * Hp[k];
        const bool ge = used && xin >= (REV ? ch : cw);
        const bool nx = used && !ge && need_next;
        b = ge ? k : b; cw_b = ge ? cw : cw_b; ch_b = ge ? ch : ch_b; w_b = ge ? wk : w_b; h_b = ge ? hk : h_b;
        w_m = ge ? w_last : w_m; h_m = ge ? h_last : h_m;
        w_p = nx ? wk : w_p; h_p = nx ? hk : h_p;
        need_next = used ? ge : need_next;
        w_last = wk; h_last = hk;
        cw += wk; ch += hk;
    }
    const float dpar0 = Dp[0], dpar1 = Dp[1];
    const float rcw = (b == K - 1) ? 1.f : cw_b + w_b;                                     // :107 (last knot pinned)
    const cubic_coef cf = cubic_bin_coef(b, K, w_b, h_b, w_m, h_m, w_p, h_p, dpar0, dpar1);
    const float a = cf.a, bb = cf.bb, c = cf.c, d = ch_b;                                  // :134-137
    if constexpr (REV) {
        const float so = cubic_invert(a, bb, c, d, xin, cw_b, rcw);
        const float o = so + cw_b;
        ljd = -fast_log(3.f * a * (so * so) + 2.f * bb * so + c);                        // :225-227
        out = fminf(fmaxf(o * span + lower, lower), upper);                                // :235 (see cubic_kernel)
        ljd = (ljd - log_span) + log_span;                                                 // :236
        if (ref_ldj) {
            const bool in2 = inside && (out >= lower) && (out <= upper);
            const float xin2 = ((in2 ? out : lower) - lower) * inv_span;
            const bool same_bin = (xin2 >= cw_b) && (b == K - 1 || xin2 < cw_b + w_b);
            const float t2 = xin2 - cw_b;
            float lf = fast_log(3.f * a * (t2 * t2) + 2.f * bb * t2 + c);
            const bool slow = valid && in2 && !same_bin;
            if (__builtin_amdgcn_ballot_w64(slow)) {
                if (slow) lf = cubic_select_forward_logderiv<true>([&](int k) { return Wp[k]; }, [&](int k) { return Hp[k]; }, nw, nh, dpar0, dpar1, K, xin2);
            }
            lf = (lf + log_span) - log_span;                                               // :239
            ljd = in2 ? -lf : 0.f;                                                         // :46-48 tails; flow.py:47 negation
        }
    } else {
        const float t = xin - cw_b;                                                        // :229
        out = a * (t * t * t) + bb * (t * t) + c * t + d;                                  // :230-233
        ljd = fast_log(3.f * a * (t * t) + 2.f * bb * t + c);                            // :235-237
        out = out * span + lower;                                                          // :238
        ljd = (ljd + log_span) - log_span;                                                 // :239
    }
    if (!inside) { out = xv; ljd = 0.f; }                                                  // :46-48 linear tails
}

// The NEXT chunk's parameter GEMM, issued one MFMA per hook of the current chunk's evaluation -- a wave's vector work only overlaps
// the matrix pipe between its OWN MFMAs (profiles/r05_coexec_probe.txt: two waves of a SIMD in different phases do not).  MFMA H:
// hidden tile H / 18, k16-step (H % 18) / 9, fp16 product term (H % 9) / 3, accumulator tile H % 3: every operand register and LDS
// offset is static; `H < total` (18 HT, or 0 without a next chunk) is the one run-time test.  Fragments of even / odd tiles and the
// A fragments of the two k16-steps alternate between two register sets, requested nine to eighteen MFMAs ahead of their first use.
struct slabf_pipe {
    const u32x4 *hf;            // the next chunk's fragments (+ lane)
    const char *wb;             // A operands (LDS, + lane * 16)
    int HT;
    u32x4 f0[4], f1[4];
    afrag a0[3], a1[3];
    f32x16 acc[3];
    // (loads never sit behind a branch: a tile index past the end is clamped to the last tile -- a redundant load of valid memory --, so
    //  the compiler's wait counts stay exact; a load behind `if (m + 1 < HT)` made every later s_waitcnt a full one)
    __device__ __forceinline__ void begin(const u32x4 *frags, const char *wbase, const char *cbase, int ht, int bias_off) {
        hf = frags; wb = wbase; HT = ht;
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = load_cfrag1(cbase, bias_off + t * 32);
#pragma unroll
        for (int p = 0; p < 4; ++p) f0[p] = hf[p * 64];
#pragma unroll
        for (int t = 0; t < 3; ++t) a0[t] = load_afrag(wb, (t * HT) * 1024, 0);
    }
    // MFMA H of the chunk (no guard: the caller knows that hidden tile H / 18 exists)
    template <int H> __device__ __forceinline__ void mfma_at() {
        constexpr int m = H / 18, v = H % 18, sx = v / 9, ph = (v % 9) / 3, t = v % 3;
        if constexpr (v == 0) {
            const int mn = m + 1 < HT ? m + 1 : HT - 1;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if constexpr ((m + 1) & 1) f1[p] = hf[mn * 256 + p * 64]; else f0[p] = hf[mn * 256 + p * 64];
            }
#pragma unroll
            for (int tt = 0; tt < 3; ++tt) a1[tt] = load_afrag(wb, (tt * HT + m) * 1024, 1);
        }
        if constexpr (v == 9) {
            const int mn = m + 1 < HT ? m + 1 : HT - 1;
#pragma unroll
            for (int tt = 0; tt < 3; ++tt) a0[tt] = load_afrag(wb, (tt * HT + mn) * 1024, 0);
        }
        const h8 bhi = __builtin_bit_cast(h8, (m & 1) ? f1[2 * sx] : f0[2 * sx]);
        const h8 blo = __builtin_bit_cast(h8, (m & 1) ? f1[2 * sx + 1] : f0[2 * sx + 1]);
        const afrag &a = sx ? a1[t] : a0[t];
        if constexpr (ph == 0) acc[t] = mfma(a.lo, bhi, acc[t]);          // smallest terms first
        else if constexpr (ph == 1) acc[t] = mfma(a.hi, blo, acc[t]);
        else acc[t] = mfma(a.hi, bhi, acc[t]);
        asm volatile("" : "+v"(acc[t]));
    }
    // hook of the evaluation: MFMAs 0 .. SLABF_NE - 1 (hidden tiles 0 .. 2: the pipelined stage runs for HT >= 3)
    template <int H, class... T> __device__ __forceinline__ void at(T &...tie) {
        (tie_one(tie), ...);
        mfma_at<H>();
    }
    template <class T> static __device__ __forceinline__ void tie_one(T &v) { asm volatile("" : "+v"(v)); }
    template <int H, int END> __device__ __forceinline__ void run() {          // MFMAs H .. END - 1, back to back
        if constexpr (H < END) {
            mfma_at<H>();
            run<H + 1, END>();
        }
    }
    // what the evaluation's hooks did not reach: the rest of tile 2, then ONE test per further hidden tile
    template <int M = 3> __device__ __forceinline__ void drain_tiles() {
        if constexpr (M < 8) {
            if (M < HT) {
                run<18 * M, 18 * M + 18>();
                drain_tiles<M + 1>();
            }
        }
    }
    __device__ __forceinline__ void drain() {
        run<SLABF_NE, 54>();
        drain_tiles<3>();
    }
};

// HFRAG: h arrives as fp16 hi / lo B fragments ([chunk][hidden tile][2 k16-step + (hi, lo)][64 lanes] x 16 B, written by
// rqs_slab_hidden_kernel): four 1 KB loads per tile, no split here -- every slab re-reads h, so the split's 36 vector instructions
// per tile were paid n_slabs times (a third of this kernel's vector work at 160 hidden units).
// PIPE (HFRAG only, HT >= 3: the evaluation's hooks reach into hidden tile 2): the software-pipelined chunk loop.
// CUBIC: monotone cubic splines (2K + 2 parameters per element, the two boundary derivatives in the third tile), unpipelined.
// WIDE: 17 .. 32 bins, ONE transformed column per slab and its element in a lane pair (rqs_slab_eval_wide; slab_slot_rows_wide is the
// slot map), unpipelined: both halves read the element's x, half 0 writes y and the slab's log-det partial -- the element's own value.
template <int KC, bool HFULL, bool REV, bool HFRAG, bool PIPE, bool CUBIC, bool WIDE = false>
__global__ __launch_bounds__(512, 1) void rqs_slab_fwd_kernel(const slabf_args k) {
    static_assert(!WIDE || (KC == 0 && !PIPE && !CUBIC), "the wide form: run-time bin count, unpipelined, rational-quadratic");
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HT = k.HT;
    int slab, range;
    {
        const int L = blockIdx.x, G = k.n_slabs;
        if (k.xcd_map) { const int i = L >> 3; slab = i % G; range = (i / G) * 8 + (L & 7); }
        else { slab = L % G; range = L / G; }
    }
    const int BI = 3 * HT * 1024;                                    // bias [96] behind the slab's tiles
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(k.wf + (size_t)slab * 3 * HT * 1024);
        f32x4 *dst = reinterpret_cast<f32x4 *>(smem);
        for (int i = threadIdx.x; i < 3 * HT * 256; i += 512) dst[i] = src[i];
        if (threadIdx.x < 96) smem[BI + threadIdx.x] = k.wf[(size_t)k.n_slabs * 3 * HT * 1024 + slab * 96 + threadIdx.x];
    }
    __syncthreads();
    const wptr w = make_wptr(0, lane);
    const int j = lane & 31, hh = lane >> 5;
    const int ci = WIDE ? slab : 2 * slab + hh;                         // this lane's transformed column (index into live)
    [[maybe_unused]] const int pi = WIDE ? 2 * slab + hh : ci;                     // ... and the first pass-through column it copies
    const bool col_ok = ci < k.n_live;
    const int col = col_ok ? (k.live_idx ? k.live_idx[ci] : k.l0 + ci) : 0;
    uint64_t any_bad = 0;
    const int c_begin = (int)((int64_t)k.n_chunks * range / k.n_ranges), c_end = (int)((int64_t)k.n_chunks * (range + 1) / k.n_ranges);
    if constexpr (PIPE) {
        // software pipeline over the wave's chunks: while chunk c is evaluated (vector pipe) the parameters of chunk c + 8 are formed
        // (matrix pipe), one MFMA per hook of the evaluation.  The first pass evaluates nothing real (no chunk yet): its stores
        // are masked.
        slabf_pipe pp;
        const u32x4 *hf0 = reinterpret_cast<const u32x4 *>(k.h) + lane;
        int ce = -1, cn = c_begin + wave;
        // every pass evaluates one chunk and prepares the next.  The first pass has no chunk to evaluate (its stores are masked), the
        // last prepares the range's first chunk once more (valid memory, result unused): one extra pass in ~64, no guard in the code
        auto stage = [&](f32x16 (&accE)[3]) {
            const bool have = ce >= 0;
            const int cc = have ? ce : c_begin;
            const int64_t row0 = (int64_t)cc * 32;
            const int n_here = (int)((k.n_rows - row0) < 32 ? (k.n_rows - row0) : 32);
            const bool valid = have && j < n_here && col_ok;
            const int jc = j < n_here ? j : n_here - 1;
            const uint32_t xoff = (uint32_t)jc * (uint32_t)k.dim + (uint32_t)col;
            const float xl = (k.x + row0 * k.dim)[xoff];
            // pass-through columns: lane (row, half) of slab s copies columns pass_idx[2 s + half], + 2 n_slabs, ... of its row (the row's
            // lines are in L2 for the slabs of this range anyway; a separate streaming copy of x was 20 us per layer)
            // The first one is loaded here and stored with the chunk's results (a store right behind its load would expose the load's
            // latency); masks with more pass-through than transformed columns: the rest in a loop at the end.
            const bool pdo = k.pass_idx != nullptr && have && j < n_here && ci < k.n_pass;
            const uint32_t po = pdo ? (uint32_t)j * (uint32_t)k.dim + (uint32_t)k.pass_idx[ci] : 0u;
            const float pv = pdo ? (k.x + row0 * k.dim)[po] : 0.f;
            const bool has_next = cn < c_end;
            pp.begin(hf0 + ((size_t)(has_next ? cn : c_begin) * HT) * 256, w.wb, w.cb, HT, BI);
            const float xv = valid ? xl : (REV ? k.bottom : k.left);
            const bool nan_h = accE[0][0] != accE[0][0];
            float out, ljd;
            if constexpr (REV) rqs_slab_eval<KC, true>(accE[1], accE[0], accE[2], k.K, xv, k.bottom, k.top, k.left, k.right, out, ljd, pp);
            else rqs_slab_eval<KC, false>(accE[0], accE[1], accE[2], k.K, xv, k.left, k.right, k.bottom, k.top, out, ljd, pp);
            pp.drain();
            if (valid) (k.y + row0 * k.dim)[xoff] = nan_h ? __builtin_nanf("") : out;
            if (pdo) {
                (k.y + row0 * k.dim)[po] = pv;
                for (int q = ci + 2 * k.n_slabs; q < k.n_pass; q += 2 * k.n_slabs) {
                    const uint32_t pq = (uint32_t)j * (uint32_t)k.dim + (uint32_t)k.pass_idx[q];
                    (k.y + row0 * k.dim)[pq] = (k.x + row0 * k.dim)[pq];
                }
            }
            if (k.ldj_part != nullptr) {
                float lsum = valid ? ljd : 0.f;
                lsum += __shfl_xor(lsum, 32, 64);
                if (have && hh == 0 && j < n_here) k.ldj_part[(size_t)slab * k.n_rows + row0 + j] = nan_h ? __builtin_nanf("") : lsum;
            }
            ce = has_next ? cn : -1;
            cn += 8;
        };
        f32x16 accA[3], accB[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) accA[t] = load_cfrag1(w.cb, BI + t * 32);
        while (true) {
            stage(accA);                      // evaluates accA (chunk ce), forms the next chunk's parameters in pp.acc
            if (ce < 0) break;
#pragma unroll
            for (int t = 0; t < 3; ++t) accB[t] = pp.acc[t];
            stage(accB);
            if (ce < 0) break;
#pragma unroll
            for (int t = 0; t < 3; ++t) accA[t] = pp.acc[t];
        }
    } else {
    for (int c = c_begin + wave; c < c_end; c += 8) {
        rng_t rg{0};
        const int64_t row0 = (int64_t)c * 32;
        const int n_here = (int)((k.n_rows - row0) < 32 ? (k.n_rows - row0) : 32);
        const bool valid = j < n_here && col_ok;
        const int jc = j < n_here ? j : n_here - 1;                     // a row past the end reads the chunk's last real row
        const float *hb = k.h + row0 * k.ld_h;
        const uint32_t hoff = (uint32_t)jc * (uint32_t)k.ld_h + 4u * hh, xoff = (uint32_t)jc * (uint32_t)k.dim + (uint32_t)col;
        const float xl = (k.x + row0 * k.dim)[xoff];
        const bool pdo = k.pass_idx != nullptr && j < n_here && pi < k.n_pass;      // pass-through columns: see the pipelined loop
        const uint32_t po = pdo ? (uint32_t)j * (uint32_t)k.dim + (uint32_t)k.pass_idx[pi] : 0u;
        const float pv = pdo ? (k.x + row0 * k.dim)[po] : 0.f;
        auto load_h = [&](int m, f32x4 (&v)[4]) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int f0 = 32 * m + 8 * g + 4 * hh;
                const float *p = hb + (hoff + 32u * m + 8u * g);
                v[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (HFULL) v[g] = *reinterpret_cast<const f32x4 *>(p);
                else {
                    if (f0 + 0 < k.H) v[g].x = p[0];
                    if (f0 + 1 < k.H) v[g].y = p[1];
                    if (f0 + 2 < k.H) v[g].z = p[2];
                    if (f0 + 3 < k.H) v[g].w = p[3];
                }
            }
        };
        // p = W2_slab h + b2: three independent accumulation chains (widths | heights | derivatives), issued round-robin
        tile<1> acc[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = load_cfrag<1>(w.cb, BI + t * 32);
        if constexpr (HFRAG) {      // (fewer than three hidden tiles: no pipeline)
            const u32x4 *hf = reinterpret_cast<const u32x4 *>(k.h) + ((size_t)c * HT) * 256 + lane;
            u32x4 fr[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) fr[p] = hf[p * 64];
            for (int m = 0; m < HT; ++m) {
                u32x4 cu[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) cu[p] = fr[p];
                if (m + 1 < HT) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) fr[p] = hf[(m + 1) * 256 + p * 64];     // in flight across this tile's MFMAs
                }
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    const h8 bhi = __builtin_bit_cast(h8, cu[2 * sx]), blo = __builtin_bit_cast(h8, cu[2 * sx + 1]);
                    afrag a[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) a[t] = load_afrag(w.wb, (t * HT + m) * 1024, sx);
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].lo, bhi, acc[t].v[0]);      // smallest terms first
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, blo, acc[t].v[0]);
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bhi, acc[t].v[0]);
                }
            }
        } else {
        f32x4 hv[4];
        load_h(0, hv);
        for (int m = 0; m < HT; ++m) {
            tile<1> hid;
#pragma unroll
            for (int g = 0; g < 4; ++g) { hid.v[0][4 * g + 0] = hv[g].x; hid.v[0][4 * g + 1] = hv[g].y; hid.v[0][4 * g + 2] = hv[g].z; hid.v[0][4 * g + 3] = hv[g].w; }
            if (m + 1 < HT) load_h(m + 1, hv);                          // in flight across this tile's split and MFMAs
            const btile<1> bh = make_btile<1>(hid, rg);
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                afrag a[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) a[t] = load_afrag(w.wb, (t * HT + m) * 1024, sx);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].lo, bh.hi[0][sx], acc[t].v[0]);      // smallest terms first
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bh.lo[0][sx], acc[t].v[0]);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t].v[0] = mfma(a[t].hi, bh.hi[0][sx], acc[t].v[0]);
            }
        }
        }
        const float xv = valid ? xl : (REV ? k.bottom : k.left);
        const bool nan_h = acc[0].v[0][0] != acc[0].v[0][0];
        float out, ljd;
        slabf_nohook nh;
        if constexpr (CUBIC) cubic_slab_eval<REV>(acc[0].v[0], acc[1].v[0], acc[2].v[0], k.K, xv, k.left, k.right, k.log_span, k.ref_ldj != 0, valid, out, ljd);
        else if constexpr (WIDE && REV) rqs_slab_eval_wide<true>(acc[1].v[0], acc[0].v[0], acc[2].v[0], k.K, hh, xv, k.bottom, k.top, k.left, k.right, out, ljd, nh);
        else if constexpr (WIDE) rqs_slab_eval_wide<false>(acc[0].v[0], acc[1].v[0], acc[2].v[0], k.K, hh, xv, k.left, k.right, k.bottom, k.top, out, ljd, nh);
        else if constexpr (REV) rqs_slab_eval<KC, true>(acc[1].v[0], acc[0].v[0], acc[2].v[0], k.K, xv, k.bottom, k.top, k.left, k.right, out, ljd, nh);
        else rqs_slab_eval<KC, false>(acc[0].v[0], acc[1].v[0], acc[2].v[0], k.K, xv, k.left, k.right, k.bottom, k.top, out, ljd, nh);
        // (HFRAG: a row whose h left fp16's range carries NaN fragments -- flagged by the kernel that wrote them)
        const bool bad = HFRAG ? nan_h : rng_bad_sample(rg, lane);
        any_bad |= rg.bad;
        if (valid && (!WIDE || hh == 0)) (k.y + row0 * k.dim)[xoff] = bad ? __builtin_nanf("") : out;
        if (pdo) {
            (k.y + row0 * k.dim)[po] = pv;
            for (int q = pi + 2 * k.n_slabs; q < k.n_pass; q += 2 * k.n_slabs) {
                const uint32_t pq = (uint32_t)j * (uint32_t)k.dim + (uint32_t)k.pass_idx[q];
                (k.y + row0 * k.dim)[pq] = (k.x + row0 * k.dim)[pq];
            }
        }
        if (k.ldj_part != nullptr) {
            float lsum = valid ? ljd : 0.f;
            if constexpr (!WIDE) lsum += __shfl_xor(lsum, 32, 64);
            if (hh == 0 && j < n_here) k.ldj_part[(size_t)slab * k.n_rows + row0 + j] = bad ? __builtin_nanf("") : lsum;
        }
    }
    }
    if (any_bad != 0 && lane == 0 && k.flags != nullptr)
        __hip_atomic_fetch_or(k.flags, SX_FLAG_F16_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The conditioner's hidden layer for the forward slab pass, single-hidden-layer conditioners (net/mlp.py:48-58 with one hidden
// layer; coupling.py:61-65: the layer sees cat[x * mask, latent]):  h = act(W1 z + b1), written ONCE as the fp16 hi / lo B fragments
// the slab kernel's MFMAs consume (4 B per value, like fp32; 1 KB per store).  The mask is folded into the pack (a masked column has
// no slot).  Input slot q: column q of x (q < dim), then column q - dim of latent.
// Operand range (round 6; ADVICE r5, VERDICT r5 #4c): the reference takes any finite fp32 here (net/mlp.py:65; coupling.py:61
// multiplies the transformed columns by mask = 0).  The inputs a slot's mask bit rules out are ZEROED before the fp16 split (they
// used to enter it raw: a transformed column of 1e6 -- weight 0 in the pack -- turned the row into NaN), and a sample whose
// conditioning input leaves fp16's range is rescaled by a power of two like the fused tier's hidden layer (rng_pow2_of: the wave
// evaluates the layer once more with every sample's inputs times 2^-e, accumulated from zero, restored as bias + 2^e acc -- exact
// scalings, wave-uniform, never taken on ordinary data).  What still gives NaN fragments + SX_FLAG_F16_RANGE: a hidden ACTIVATION
// beyond 65504 (unbounded activations only: the fragments are fp16 pairs).
struct slabh_args {
    const float *x, *latent;            // [N, dim], [N, latent_dim] | null
    const float *w1;                    // sx_pack_linear(W1, b1, hidden slots, input slots, m_tiles = HT, k_tiles = CT)
    float *hfrag;                       // [n_chunks][HT][1024]
    uint32_t *flags;
    int64_t n_rows;
    int dim, latent_dim, HT, act, n_chunks;
    uint32_t cmask[4];                  // bit q: input slot q feeds the layer (a conditioning column / a latent column)
};
// TANH: the activation inline (the generic one is an out-of-line call on the tile's ADDRESS: the tile then lives in scratch, 8 KB of
// scratch traffic per tile and wave -- measured as 100 MB of extra HBM writes per launch)
template <int CT, bool TANH>
__global__ __launch_bounds__(512) void rqs_slab_hidden_kernel(const slabh_args k) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HT = k.HT;
    {
        const int n4 = (HT * CT * 1024 + HT * 32) / 4;
        const f32x4 *src = reinterpret_cast<const f32x4 *>(k.w1);
        f32x4 *dst = reinterpret_cast<f32x4 *>(smem);
        for (int i = threadIdx.x; i < n4; i += 512) dst[i] = src[i];
    }
    __syncthreads();
    const wptr w = make_wptr(0, lane);
    const int j = lane & 31, hh = lane >> 5;
    const int bias = HT * CT * 1024;
    const bool xvec = (k.dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(k.x) & 15) == 0);
    uint64_t any_bad = 0;
    for (int c = blockIdx.x * 8 + wave; c < k.n_chunks; c += gridDim.x * 8) {
        rng_t rg{0};
        const int64_t row0 = (int64_t)c * 32;
        const int n_here = (int)((k.n_rows - row0) < 32 ? (k.n_rows - row0) : 32);
        const int64_t row = row0 + (j < n_here ? j : n_here - 1);
        btile<1> bx[CT];
        tile<1> zs[CT];
        float mx = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            tile<1> &z = zs[ct];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q0 = 32 * ct + 8 * g + 4 * hh;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (xvec && q0 + 3 < k.dim) v = *reinterpret_cast<const f32x4 *>(k.x + row * k.dim + q0);
                else {
                    float e[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int q = q0 + i;
                        e[i] = q < k.dim ? k.x[row * k.dim + q] : (q < k.dim + k.latent_dim ? k.latent[row * k.latent_dim + (q - k.dim)] : 0.f);
                    }
                    v = f32x4{e[0], e[1], e[2], e[3]};
                }
                const uint32_t live = (k.cmask[ct] >> (8 * g + 4 * hh)) & 15u;          // slots q0 .. q0 + 3
                z.v[0][4 * g + 0] = (live & 1u) ? v.x : 0.f; z.v[0][4 * g + 1] = (live & 2u) ? v.y : 0.f;
                z.v[0][4 * g + 2] = (live & 4u) ? v.z : 0.f; z.v[0][4 * g + 3] = (live & 8u) ? v.w : 0.f;
            }
            bx[ct] = make_btile_mx<1>(z, mx);
        }
        const bool over = rng_over(mx);                 // wave-uniform; see slabh_args
        rng_pow2 p2{1.f, 1.f};
        if (over) {
            p2 = rng_pow2_of(mx);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) bx[ct] = make_btile_scaled<1>(zs[ct], p2.sc);
        }
        u32x4 *dst = reinterpret_cast<u32x4 *>(k.hfrag) + ((size_t)c * HT) * 256 + lane;
        for (int m = 0; m < HT; ++m) {
            tile<1> acc = load_cfrag<1>(w.cb, bias + m * 32);
            if (!over) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) gemm_tile<1>(w.wb, (m * CT + ct) * 1024, bx[ct], acc);
            } else {
                tile<1> a0;
#pragma unroll
                for (int r = 0; r < 16; ++r) a0.v[0][r] = 0.f;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) gemm_tile<1>(w.wb, (m * CT + ct) * 1024, bx[ct], a0);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc.v[0][r] = __builtin_fmaf(a0.v[0][r], p2.inv, acc.v[0][r]);
            }
            if constexpr (TANH) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc.v[0][r] = fast_tanh(acc.v[0][r]);
            } else activate<1>(acc, k.act);
            const btile<1> bh = make_btile<1>(acc, rg);
            const bool bad = rng_bad_sample(rg, lane);
            const u32x4 nanv = {0x7e007e00u, 0x7e007e00u, 0x7e007e00u, 0x7e007e00u};
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                dst[m * 256 + (2 * sx) * 64] = bad ? nanv : __builtin_bit_cast(u32x4, bh.hi[0][sx]);
                dst[m * 256 + (2 * sx + 1) * 64] = bad ? nanv : __builtin_bit_cast(u32x4, bh.lo[0][sx]);
            }
        }
        any_bad |= rg.bad;
    }
    if (any_bad != 0 && lane == 0 && k.flags != nullptr)
        __hip_atomic_fetch_or(k.flags, SX_FLAG_F16_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// row log-det = ldj_scale * (sum of the slabs' partials, in slab order) [+ what ldj already holds]
__global__ __launch_bounds__(256) void rqs_slab_ldj_reduce_kernel(const float *__restrict__ part, int n_slabs, int64_t n_rows,
                                                                  float ldj_scale, int accumulate, float *__restrict__ ldj) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    float s = 0.f;
    for (int p = 0; p < n_slabs; ++p) s += part[(size_t)p * n_rows + i];
    s *= ldj_scale;
    ldj[i] = accumulate ? ldj[i] + s : s;
}

// launch shape: slabs per workgroup, slab groups, row ranges (one 8-wave workgroup per CU, or two 4-wave ones)
struct slab_shape { int spw, n_groups, n_ranges; };
slab_shape slab_plan(int n_slabs, int n_chunks, int ht = 2) {
    slab_shape p;
    p.spw = (ht > 2) ? 1 : (n_slabs >= 2 ? 2 : 1);
    p.n_groups = (n_slabs + p.spw - 1) / p.spw;
    int r = ((p.spw == 2 || ht > 2 ? 256 : 512) + p.n_groups - 1) / p.n_groups;      // workgroups per CU: 1 (8 waves, or HT > 2) | 2
    const int cap = (n_chunks + 3) / 4;              // at least one 32-row chunk per wave where the rows allow
    if (r > cap) r = cap;
    if (r >= 8) r &= ~7;                             // multiples of 8: the XCD-aware id mapping
    p.n_ranges = r < 1 ? 1 : r;
    return p;
}
}  // namespace

// (a size query takes any argument: 0 outside the widths a slab pass exists for -- the host sanitizer job found the int overflow at
//  n_live = INT_MAX)
extern "C" int32_t sx_rqs_slab_slots(int32_t n_live) { return (n_live < 1 || n_live > (1 << 20)) ? 0 : ((n_live + 1) / 2) * 96; }

extern "C" size_t sx_rqs_slab_scratch_floats(int64_t n_rows, int32_t n_live, int32_t hidden) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 36) || n_live < 1 || n_live > (1 << 20) || hidden < 1 || hidden > 256) return 0;
    const int n_slabs = (n_live + 1) / 2, HT = (hidden + 31) / 32;
    const int64_t n_chunks = (n_rows + 31) / 32;
    const slab_shape p = slab_plan(n_slabs, (int)n_chunks, HT);
    return (size_t)p.n_groups * (size_t)n_chunks * HT * 1024 + (size_t)n_slabs * p.n_ranges * (96 * 32 * HT + 96);
}

extern "C" int sx_rqs_slab_bwd(const float *x, const float *gout, const float *gldj, const float *xout, const float *h, int64_t ld_h,
                               int32_t hidden, const float *w_fwd, const float *w_bwd, const int32_t *slot_rows, float *gx,
                               float *gh, int64_t ld_gh, float *dW, int64_t ldw, float *db, const int32_t *live_idx,
                               int32_t live_start, int32_t n_live, int32_t n_bins, float left, float right, float bottom,
                               float top, int64_t n_rows, int32_t dim, float ldj_scale, int32_t tanh_hidden, const float *scale,
                               float *scratch, uint32_t *err_flag, void *stream) {
    SX_REQUIRE(x && gout && gldj && h && w_fwd && w_bwd && slot_rows && gx && dW && db && scratch, "sx_rqs_slab_bwd: null pointer");
    SX_REQUIRE(dim > 0 && n_live > 0 && n_live <= dim && n_rows >= 0, "sx_rqs_slab_bwd: bad sizes");
    SX_REQUIRE(n_bins >= 1 && n_bins <= 16, "sx_rqs_slab_bwd: n_bins must be in 1..16 (got %d)", n_bins);
    SX_REQUIRE(hidden >= 1 && hidden <= 256, "sx_rqs_slab_bwd: hidden width must be in 1..256 (got %d)", hidden);
    SX_REQUIRE(gh != nullptr || hidden <= 128, "sx_rqs_slab_bwd: sx_rqs_slab_l1_bwd (gh = NULL) holds hidden layers of up to 128 units");
    SX_REQUIRE(n_rows < ((int64_t)1 << 36), "sx_rqs_slab_bwd: too many rows");
    SX_REQUIRE(right > left && top > bottom, "sx_rqs_slab_bwd: empty domain");
    SX_REQUIRE(((uintptr_t)w_fwd & 15) == 0 && ((uintptr_t)w_bwd & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
               "sx_rqs_slab_bwd: packed weights and scratch must be 16-byte aligned");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const int n_slabs = (n_live + 1) / 2, HT = (hidden + 31) / 32;
    const int n_chunks = (int)((n_rows + 31) / 32);
    const slab_shape pl = slab_plan(n_slabs, n_chunks, HT);
    const int n_ranges = pl.n_ranges, n_groups = pl.n_groups;
    slab_args k;
    k.x = x; k.gout = gout; k.gldj = gldj; k.xout = xout; k.h = h; k.wf = w_fwd; k.wb = w_bwd; k.gx = gx;
    k.dh_part = scratch;
    k.w_part = scratch + (size_t)n_groups * n_chunks * HT * 1024;
    k.live_idx = live_idx; k.scale = scale; k.flags = err_flag; k.n_rows = n_rows; k.ld_h = ld_h; k.l0 = live_start; k.n_live = n_live;
    k.K = n_bins; k.dim = dim; k.H = hidden; k.n_slabs = n_slabs; k.n_chunks = n_chunks; k.n_groups = n_groups; k.n_ranges = n_ranges;
    k.xcd_map = n_ranges % 8 == 0;
    k.left = left; k.right = right; k.bottom = bottom; k.top = top; k.ldj_scale = ldj_scale;
    const int HTa = HT <= 4 ? HT : (HT + 1) / 2;                // hidden tiles of the (first) launch; beyond four: two launches
    const size_t lds = (size_t)(pl.spw * (3 * (HT + HTa) * 1024 + 128) + (pl.spw == 2 ? 8 * 1024 + 32 : 0)) * sizeof(float);
    int dev = 0;
    (void)hipGetDevice(&dev);
#define SX_SLAB2(HT_, KC_, HF_, SPW_)                                                                              \
    do {                                                                                                           \
        auto kern = xout ? rqs_slab_bwd_kernel<HT_, KC_, HF_, SPW_, true> : rqs_slab_bwd_kernel<HT_, KC_, HF_, SPW_, false>;                                                      \
        /* the attribute is set to the launch's own need: at a blanket 160 KiB the SPW = 1 form ran one workgroup  */  \
        /* per CU less (measured: 1.16 vs 0.92 ms)                                                                */  \
        static int lds_allowed[2][64];                                                                             \
        if (lds > 48 * 1024 && !lds_allowed[xout != nullptr][dev & 63]) {                                          \
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; } \
            lds_allowed[xout != nullptr][dev & 63] = 1;                                                            \
        }                                                                                                          \
        hipLaunchKernelGGL(kern, dim3(n_groups * n_ranges), dim3(256 * SPW_), lds, st, k);                         \
    } while (0)
#define SX_SLAB(HT_, KC_, HF_) do { if (pl.spw == 2) SX_SLAB2(HT_, KC_, HF_, 2); else SX_SLAB2(HT_, KC_, HF_, 1); } while (0)
    const bool hfull = hidden == 32 * HT && ld_h % 4 == 0 && ((uintptr_t)h & 15) == 0;
    if (HT == 1) {
        if (n_bins == 16 && hfull) SX_SLAB(1, 16, true); else if (hfull) SX_SLAB(1, 0, true); else SX_SLAB(1, 0, false);
    } else if (HT == 2) {
        if (n_bins == 16 && hfull) SX_SLAB(2, 16, true); else if (hfull) SX_SLAB(2, 0, true); else SX_SLAB(2, 0, false);
    } else if (HT == 3) {           // (one workgroup shape, two bin-count forms: the wide kernels are long compiles)
        if (n_bins == 16 && hfull) SX_SLAB2(3, 16, true, 1); else SX_SLAB2(3, 0, false, 1);
    } else if (HT == 4) {
        if (n_bins == 16 && hfull) SX_SLAB2(4, 16, true, 1); else SX_SLAB2(4, 0, false, 1);
    } else {
        // 129 .. 256 hidden units: two launches, each over half of the hidden tiles (kernel comment)
#define SX_SLAB3(HT_, KC_, HF_, HTF_, M0_)                                                                         \
    do {                                                                                                           \
        auto kern = xout ? rqs_slab_bwd_kernel<HT_, KC_, HF_, 1, true, HTF_, M0_> : rqs_slab_bwd_kernel<HT_, KC_, HF_, 1, false, HTF_, M0_>; \
        static int lds_allowed[2][64];                                                                             \
        if (lds > 48 * 1024 && !lds_allowed[xout != nullptr][dev & 63]) {                                          \
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; } \
            lds_allowed[xout != nullptr][dev & 63] = 1;                                                            \
        }                                                                                                          \
        hipLaunchKernelGGL(kern, dim3(n_groups * n_ranges), dim3(256), lds, st, k);                                \
    } while (0)
#define SX_SLAB3P(HTA_, HTB_, HTF_) do { if (n_bins == 16 && hfull) { SX_SLAB3(HTA_, 16, true, HTF_, 0); SX_SLAB3(HTB_, 16, true, HTF_, HTA_); } \
                                         else { SX_SLAB3(HTA_, 0, false, HTF_, 0); SX_SLAB3(HTB_, 0, false, HTF_, HTA_); } } while (0)
        if (HT == 5) SX_SLAB3P(3, 2, 5); else if (HT == 6) SX_SLAB3P(3, 3, 6); else if (HT == 7) SX_SLAB3P(4, 3, 7); else SX_SLAB3P(4, 4, 8);
#undef SX_SLAB3P
#undef SX_SLAB3
    }
#undef SX_SLAB2
#undef SX_SLAB
    SX_LAUNCH_CHECK();
    const int N2 = 32 * HT, E = 96 * N2 + 96;
    hipLaunchKernelGGL(rqs_slab_w_reduce_kernel, dim3((E + 255) / 256, n_slabs), dim3(256), 0, st, k.w_part, n_ranges, N2,
                       (int)hidden, slot_rows, dW, ldw, db, scale);
    SX_LAUNCH_CHECK();
    if (gh == nullptr) return SX_OK;            // the caller reduces the dh partials itself (sx_rqs_slab_l1_bwd)
    const int64_t pieces = (int64_t)n_chunks * HT * 256;
#define SX_DHRED(HT_) hipLaunchKernelGGL(rqs_slab_dh_reduce_kernel<HT_>, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, k.dh_part, \
                                         n_groups, n_chunks, n_rows, (int)hidden, gh, ld_gh, scale, tanh_hidden ? h : nullptr, ld_h)
    switch (HT) { case 1: SX_DHRED(1); break; case 2: SX_DHRED(2); break; case 3: SX_DHRED(3); break; case 4: SX_DHRED(4); break;
                  case 5: SX_DHRED(5); break; case 6: SX_DHRED(6); break; case 7: SX_DHRED(7); break; default: SX_DHRED(8); break; }
#undef SX_DHRED
    SX_LAUNCH_CHECK();
    return SX_OK;
}

extern "C" size_t sx_rqs_slab_fwd_scratch_floats(int64_t n_rows, int32_t n_live) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 36) || n_live < 1 || n_live > (1 << 20)) return 0;
    return (size_t)((n_live + 1) / 2) * (size_t)n_rows;
}

extern "C" int sx_rqs_slab_fwd(const float *x, const float *h, int64_t ld_h, int32_t hidden, const float *w_fwd, float *y, float *ldj,
                               const int32_t *live_idx, int32_t live_start, int32_t n_live, const int32_t *pass_idx, int32_t n_pass,
                               int32_t n_bins, float left, float right,
                               float bottom, float top, int64_t n_rows, int32_t dim, int32_t reverse, float ldj_scale,
                               int32_t ldj_accumulate, int32_t h_fragments, int32_t cubic, float *scratch, uint32_t *err_flag,
                               void *stream) {
    SX_REQUIRE(x && h && w_fwd && y, "sx_rqs_slab_fwd: null pointer");
    SX_REQUIRE(!h_fragments || ((uintptr_t)h & 15) == 0, "sx_rqs_slab_fwd: h fragments must be 16-byte aligned");
    SX_REQUIRE(ldj == nullptr || scratch != nullptr, "sx_rqs_slab_fwd: the row log-det needs the scratch buffer");
    SX_REQUIRE(dim > 0 && n_live > 0 && n_live <= dim && n_rows >= 0, "sx_rqs_slab_fwd: bad sizes");
    SX_REQUIRE(n_pass >= 0 && n_pass <= dim - n_live && (n_pass == 0 || pass_idx != nullptr), "sx_rqs_slab_fwd: bad pass-through columns");
    SX_REQUIRE(n_bins >= 1 && n_bins <= 16, "sx_rqs_slab_fwd: n_bins must be in 1..16 (got %d)", n_bins);
    SX_REQUIRE(hidden >= 1 && hidden <= 256, "sx_rqs_slab_fwd: hidden width must be in 1..256 (got %d)", hidden);
    SX_REQUIRE(h_fragments || ld_h >= hidden, "sx_rqs_slab_fwd: ld_h < hidden");
    SX_REQUIRE(n_rows < ((int64_t)1 << 36), "sx_rqs_slab_fwd: too many rows");
    SX_REQUIRE(right > left && top > bottom, "sx_rqs_slab_fwd: empty domain");
    SX_REQUIRE(reverse >= 0 && reverse <= (cubic ? 2 : 1), "sx_rqs_slab_fwd: reverse must be 0 | 1 (cubic: | 2)");
    SX_REQUIRE(!cubic || (left == bottom && right == top), "sx_rqs_slab_fwd: cubic splines map [left, right] onto itself");
    SX_REQUIRE(((uintptr_t)w_fwd & 15) == 0, "sx_rqs_slab_fwd: packed weights must be 16-byte aligned");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const int n_slabs = (n_live + 1) / 2, HT = (hidden + 31) / 32;
    const int n_chunks = (int)((n_rows + 31) / 32);
    // one 8-wave workgroup per CU at a time; two rounds of them so that the tail of the launch is short
    int r = (512 + n_slabs - 1) / n_slabs;
    const int cap = (n_chunks + 7) / 8;              // at least one 32-row chunk per wave where the rows allow
    if (r > cap) r = cap;
    if (r >= 8) r &= ~7;                             // multiples of 8: the XCD-aware id mapping
    const int n_ranges = r < 1 ? 1 : r;
    slabf_args k;
    k.x = x; k.h = h; k.wf = w_fwd; k.y = y; k.ldj_part = ldj ? scratch : nullptr; k.live_idx = live_idx; k.pass_idx = n_pass > 0 ? pass_idx : nullptr; k.flags = err_flag;
    k.n_rows = n_rows; k.ld_h = ld_h; k.l0 = live_start; k.n_live = n_live; k.n_pass = n_pass; k.K = n_bins; k.dim = dim; k.H = hidden; k.HT = HT;
    k.n_slabs = n_slabs; k.n_chunks = n_chunks; k.n_ranges = n_ranges; k.xcd_map = (n_ranges % 8 == 0);
    k.left = left; k.right = right; k.bottom = bottom; k.top = top;
    k.log_span = logf(right - left); k.ref_ldj = reverse == 2;
    const size_t lds = (size_t)(3 * HT * 1024 + 128) * sizeof(float);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool hfull = hidden == 32 * HT && ld_h % 4 == 0 && ((uintptr_t)h & 15) == 0;
#define SX_SLABF(KC_, HF_, REV_, ID_) do { if (h_fragments && HT >= 3) SX_SLABF2(KC_, true, REV_, true, true, false, ID_ + 12); else if (h_fragments) SX_SLABF2(KC_, true, REV_, true, false, false, ID_ + 6); else SX_SLABF2(KC_, HF_, REV_, false, false, false, ID_); } while (0)
#define SX_SLABC(REV_, ID_) do { if (h_fragments) SX_SLABF2(0, true, REV_, true, false, true, ID_); else SX_SLABF2(0, false, REV_, false, false, true, ID_ + 1); } while (0)
#define SX_SLABF2(KC_, HF_, REV_, FR_, PI_, CU_, ID_)                                                              \
    do {                                                                                                           \
        auto kern = rqs_slab_fwd_kernel<KC_, HF_, REV_, FR_, PI_, CU_>;                                            \
        static int lds_allowed[22][64];                                                                            \
        if (lds > 48 * 1024 && lds_allowed[ID_][dev & 63] < (int)lds) {                                            \
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; } \
            lds_allowed[ID_][dev & 63] = (int)lds;                                                                 \
        }                                                                                                          \
        hipLaunchKernelGGL(kern, dim3(n_slabs * n_ranges), dim3(512), lds, st, k);                                 \
    } while (0)
    if (cubic) {
        if (reverse) SX_SLABC(true, 18); else SX_SLABC(false, 20);
    } else if (reverse) {
        if (n_bins == 16 && hfull) SX_SLABF(16, true, true, 0); else if (hfull) SX_SLABF(0, true, true, 1); else SX_SLABF(0, false, true, 2);
    } else {
        if (n_bins == 16 && hfull) SX_SLABF(16, true, false, 3); else if (hfull) SX_SLABF(0, true, false, 4); else SX_SLABF(0, false, false, 5);
    }
#undef SX_SLABC
#undef SX_SLABF
#undef SX_SLABF2
    SX_LAUNCH_CHECK();
    if (ldj != nullptr) {
        hipLaunchKernelGGL(rqs_slab_ldj_reduce_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, scratch, n_slabs,
                           n_rows, ldj_scale, (int)(ldj_accumulate != 0), ldj);
        SX_LAUNCH_CHECK();
    }
    return SX_OK;
}

// ---- the wide form: 17 .. 32 bins, one transformed column per slab (rqs_slab_fwd_kernel<..., WIDE>) ----
extern "C" int32_t sx_rqs_slab_wide_slots(int32_t n_live) { return (n_live < 1 || n_live > (1 << 20)) ? 0 : n_live * 96; }

extern "C" size_t sx_rqs_slab_wide_fwd_scratch_floats(int64_t n_rows, int32_t n_live) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 36) || n_live < 1 || n_live > (1 << 20)) return 0;
    return (size_t)n_live * (size_t)n_rows;
}

extern "C" int sx_rqs_slab_wide_fwd(const float *x, const float *h, int64_t ld_h, int32_t hidden, const float *w_fwd, float *y, float *ldj,
                                    const int32_t *live_idx, int32_t live_start, int32_t n_live, const int32_t *pass_idx, int32_t n_pass,
                                    int32_t n_bins, float left, float right, float bottom, float top, int64_t n_rows, int32_t dim,
                                    int32_t reverse, float ldj_scale, int32_t ldj_accumulate, int32_t h_fragments, float *scratch,
                                    uint32_t *err_flag, void *stream) {
    SX_REQUIRE(x && h && w_fwd && y, "sx_rqs_slab_wide_fwd: null pointer");
    SX_REQUIRE(!h_fragments || ((uintptr_t)h & 15) == 0, "sx_rqs_slab_wide_fwd: h fragments must be 16-byte aligned");
    SX_REQUIRE(ldj == nullptr || scratch != nullptr, "sx_rqs_slab_wide_fwd: the row log-det needs the scratch buffer");
    SX_REQUIRE(dim > 0 && n_live > 0 && n_live <= dim && n_rows >= 0, "sx_rqs_slab_wide_fwd: bad sizes");
    SX_REQUIRE(n_pass >= 0 && n_pass <= dim - n_live && (n_pass == 0 || pass_idx != nullptr), "sx_rqs_slab_wide_fwd: bad pass-through columns");
    SX_REQUIRE(n_bins >= 17 && n_bins <= 32, "sx_rqs_slab_wide_fwd: n_bins must be in 17..32 (got %d)", n_bins);
    SX_REQUIRE(hidden >= 1 && hidden <= 256, "sx_rqs_slab_wide_fwd: hidden width must be in 1..256 (got %d)", hidden);
    SX_REQUIRE(h_fragments || ld_h >= hidden, "sx_rqs_slab_wide_fwd: ld_h < hidden");
    SX_REQUIRE(n_rows < ((int64_t)1 << 36), "sx_rqs_slab_wide_fwd: too many rows");
    SX_REQUIRE(right > left && top > bottom, "sx_rqs_slab_wide_fwd: empty domain");
    SX_REQUIRE(reverse >= 0 && reverse <= 1, "sx_rqs_slab_wide_fwd: reverse must be 0 | 1");
    SX_REQUIRE(((uintptr_t)w_fwd & 15) == 0, "sx_rqs_slab_wide_fwd: packed weights must be 16-byte aligned");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const int n_slabs = n_live, HT = (hidden + 31) / 32;
    const int n_chunks = (int)((n_rows + 31) / 32);
    // the launch shape of sx_rqs_slab_fwd: one 8-wave workgroup per CU at a time, two rounds of them, ranges in multiples of 8
    int r = (512 + n_slabs - 1) / n_slabs;
    const int cap = (n_chunks + 7) / 8;
    if (r > cap) r = cap;
    if (r >= 8) r &= ~7;
    const int n_ranges = r < 1 ? 1 : r;
    slabf_args k;
    k.x = x; k.h = h; k.wf = w_fwd; k.y = y; k.ldj_part = ldj ? scratch : nullptr; k.live_idx = live_idx; k.pass_idx = n_pass > 0 ? pass_idx : nullptr; k.flags = err_flag;
    k.n_rows = n_rows; k.ld_h = ld_h; k.l0 = live_start; k.n_live = n_live; k.n_pass = n_pass; k.K = n_bins; k.dim = dim; k.H = hidden; k.HT = HT;
    k.n_slabs = n_slabs; k.n_chunks = n_chunks; k.n_ranges = n_ranges; k.xcd_map = (n_ranges % 8 == 0);
    k.left = left; k.right = right; k.bottom = bottom; k.top = top;
    k.log_span = logf(right - left); k.ref_ldj = 0;
    const size_t lds = (size_t)(3 * HT * 1024 + 128) * sizeof(float);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool hfull = hidden == 32 * HT && ld_h % 4 == 0 && ((uintptr_t)h & 15) == 0;
#define SX_SLABW(HF_, REV_, FR_, ID_)                                                                              \
    do {                                                                                                           \
        auto kern = rqs_slab_fwd_kernel<0, HF_, REV_, FR_, false, false, true>;                                    \
        static int lds_allowed[6][64];                                                                             \
        if (lds > 48 * 1024 && lds_allowed[ID_][dev & 63] < (int)lds) {                                            \
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; } \
            lds_allowed[ID_][dev & 63] = (int)lds;                                                                 \
        }                                                                                                          \
        hipLaunchKernelGGL(kern, dim3(n_slabs * n_ranges), dim3(512), lds, st, k);                                 \
    } while (0)
    if (reverse) {
        if (h_fragments) SX_SLABW(true, true, true, 0); else if (hfull) SX_SLABW(true, true, false, 1); else SX_SLABW(false, true, false, 2);
    } else {
        if (h_fragments) SX_SLABW(true, false, true, 3); else if (hfull) SX_SLABW(true, false, false, 4); else SX_SLABW(false, false, false, 5);
    }
#undef SX_SLABW
    SX_LAUNCH_CHECK();
    if (ldj != nullptr) {
        hipLaunchKernelGGL(rqs_slab_ldj_reduce_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, scratch, n_slabs,
                           n_rows, ldj_scale, (int)(ldj_accumulate != 0), ldj);
        SX_LAUNCH_CHECK();
    }
    return SX_OK;
}

extern "C" size_t sx_rqs_slab_hidden_floats(int64_t n_rows, int32_t hidden) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 36) || hidden < 1 || hidden > 256) return 0;
    return (size_t)((n_rows + 31) / 32) * (size_t)((hidden + 31) / 32) * 1024;
}

extern "C" int sx_rqs_slab_hidden(const float *x, const float *latent, const float *w1, const uint32_t *cond_mask, float *h_frag,
                                  int64_t n_rows, int32_t dim, int32_t latent_dim, int32_t hidden, int32_t act, uint32_t *err_flag,
                                  void *stream) {
    SX_REQUIRE(x && w1 && h_frag, "sx_rqs_slab_hidden: null pointer");
    SX_REQUIRE(dim > 0 && latent_dim >= 0 && dim + latent_dim <= 128 && n_rows >= 0, "sx_rqs_slab_hidden: bad sizes (inputs of up to 128 columns)");
    SX_REQUIRE(latent_dim == 0 || latent != nullptr, "sx_rqs_slab_hidden: null latent");
    SX_REQUIRE(hidden >= 1 && hidden <= 256, "sx_rqs_slab_hidden: hidden width must be in 1..256 (got %d)", hidden);
    SX_REQUIRE(act >= 0 && act <= SX_ACT_GELU, "sx_rqs_slab_hidden: unknown activation %d", act);
    SX_REQUIRE(n_rows < ((int64_t)1 << 36), "sx_rqs_slab_hidden: too many rows");
    SX_REQUIRE(((uintptr_t)w1 & 15) == 0 && ((uintptr_t)h_frag & 15) == 0, "sx_rqs_slab_hidden: packed weights and h must be 16-byte aligned");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const int HT = (hidden + 31) / 32, CT = (dim + latent_dim + 31) / 32;
    const int n_chunks = (int)((n_rows + 31) / 32);
    slabh_args k;
    k.x = x; k.latent = latent; k.w1 = w1; k.hfrag = h_frag; k.flags = err_flag; k.n_rows = n_rows; k.dim = dim; k.latent_dim = latent_dim;
    k.HT = HT; k.act = act; k.n_chunks = n_chunks;
    for (int i = 0; i < 4; ++i) k.cmask[i] = cond_mask ? cond_mask[i] : 0xffffffffu;      // (host words: read here, passed by value)
    const size_t lds = (size_t)(HT * CT * 1024 + HT * 32) * sizeof(float);
    // two 8-wave workgroups per CU (one copy of the layer in LDS each), several chunks per wave
    int grid = (n_chunks + 7) / 8;
    if (grid > 512) grid = 512;
    int dev = 0;
    (void)hipGetDevice(&dev);
#define SX_SLABH(CT_)                                                                                              \
    do {                                                                                                           \
        auto kern = act == SX_ACT_TANH ? rqs_slab_hidden_kernel<CT_, true> : rqs_slab_hidden_kernel<CT_, false>;          \
        static int lds_allowed[64];                                                                                \
        if (lds > 48 * 1024 && lds_allowed[dev & 63] < (int)lds) {                                                 \
            hipError_t e = hipFuncSetAttribute((const void *)rqs_slab_hidden_kernel<CT_, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e == hipSuccess) e = hipFuncSetAttribute((const void *)rqs_slab_hidden_kernel<CT_, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; } \
            lds_allowed[dev & 63] = (int)lds;                                                                      \
        }                                                                                                          \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, k);                                               \
    } while (0)
    switch (CT) { case 1: SX_SLABH(1); break; case 2: SX_SLABH(2); break; case 3: SX_SLABH(3); break; default: SX_SLABH(4); break; }
#undef SX_SLABH
    SX_LAUNCH_CHECK();
    return SX_OK;
}

extern "C" size_t sx_rqs_slab_l1_scratch_floats(int32_t dim, int32_t hidden) {
    if (dim < 1 || dim > 64 || hidden < 1 || hidden > 128) return 0;
    const int HT = (hidden + 31) / 32, XT = (dim + 31) / 32;
    return (size_t)512 * (32 * HT * 32 * XT + 32 * HT);
}

extern "C" int sx_rqs_slab_l1_bwd(const float *slab_scratch, const float *h, int64_t ld_h, int32_t hidden, const float *x,
                                  const float *gout, const float *w1t, const uint32_t *cond_mask, float *gx, float *dW1,
                                  int64_t ldw, float *db1, const int32_t *col_map, int32_t n_live, int64_t n_rows, int32_t dim,
                                  const float *scale, float *scratch, uint32_t *err_flag, void *stream) {
    SX_REQUIRE(slab_scratch && h && x && gout && w1t && cond_mask && gx && dW1 && db1 && scratch, "sx_rqs_slab_l1_bwd: null pointer");
    SX_REQUIRE(dim >= 1 && dim <= 64 && hidden >= 1 && hidden <= 128 && n_live >= 1 && n_rows >= 0,
               "sx_rqs_slab_l1_bwd: dim must be in 1..64, hidden in 1..128");
    SX_REQUIRE(((uintptr_t)w1t & 15) == 0 && ((uintptr_t)slab_scratch & 15) == 0, "sx_rqs_slab_l1_bwd: 16-byte alignment");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const int HT = (hidden + 31) / 32, XT = (dim + 31) / 32;
    const int n_slabs = (n_live + 1) / 2;
    const int n_chunks = (int)((n_rows + 31) / 32);
    const slab_shape pl = slab_plan(n_slabs, n_chunks, HT);
    l1_args k;
    k.part = slab_scratch; k.h = h; k.x = x; k.gout = gout; k.w1t = w1t; k.gx = gx; k.w_part = scratch; k.scale = scale;
    k.flags = err_flag; k.n_rows = n_rows; k.ld_h = ld_h; k.n_groups = pl.n_groups; k.n_chunks = n_chunks; k.dim = dim; k.H = hidden;
    k.cond_mask[0] = cond_mask[0]; k.cond_mask[1] = cond_mask[1];
    int grid = (n_chunks + 3) / 4;
    if (grid > 512) grid = 512;
    const size_t lds_need = (size_t)XT * HT * 1024 * sizeof(float);
    const int E1 = 32 * HT * 32 * XT + 32 * HT;
    const size_t lds = lds_need > (size_t)E1 * sizeof(float) ? lds_need : (size_t)E1 * sizeof(float);
#define SX_L1(HT_, XT_) hipLaunchKernelGGL((rqs_slab_l1_bwd_kernel<HT_, XT_>), dim3(grid), dim3(256), lds, st, k)
    if (HT == 1 && XT == 1) SX_L1(1, 1); else if (HT == 1) SX_L1(1, 2); else if (HT == 2 && XT == 1) SX_L1(2, 1); else if (HT == 2) SX_L1(2, 2);
    else if (HT == 3 && XT == 1) SX_L1(3, 1); else if (HT == 3) SX_L1(3, 2); else if (XT == 1) SX_L1(4, 1); else SX_L1(4, 2);
#undef SX_L1
    SX_LAUNCH_CHECK();
    return sx_wgrad_reduce(scratch, grid, 32 * HT, 32 * XT, dW1, ldw, db1, hidden, dim, nullptr, col_map, stream);
}
