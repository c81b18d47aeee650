// Rational-quadratic spline, element-wise kernel (parameters already in HBM).
//
// Replaces unconstrained_rational_quadratic_spline + rational_quadratic_spline
// (stribor/util/rational_quadratic_spline.py:11-251) and searchsorted (util/search_sorted.py:3-5):
// ~30 torch passes over [M, K]-sized temporaries (boolean compaction, 2 softmax, softplus, 2 cumsum,
// pad, rescale, pin, re-difference, bin search, 8 gathers, rational formula / quadratic root, scatter)
// become one pass: one lane = one (row, live column) element.
//
// CDNA4 mapping: the 3K-1 parameters of the 64 elements a wave owns are one contiguous span of HBM
// (64*(3K-1)*4 B = 12 KiB at K = 16).  The wave copies that span into ITS OWN slice of LDS with coalesced
// loads, then each lane walks its element's parameters at stride 3K-1 dwords — an odd stride, so the 32
// lanes of a ds_read_b32 group hit 32 different banks.  No compaction: tails are predicated.  The per-row
// log-det is a shuffle sum when a row's live columns sit inside one wave, float atomics otherwise.
#include "sx_stream.h"
#include "sx_rqs_core.h"

extern __shared__ __attribute__((aligned(16))) float rqs_smem[];

// A wave's parameter span HBM -> its LDS slice by LDS-DMA (global_load_lds_dwordx4: lane-linear 1 KiB pieces, no VGPRs on the
// way, asynchronous -- counted by vmcnt).  BYTES is a multiple of 16; the last piece runs with the upper lanes masked off.
// The spline kernels issue the NEXT group's copy as soon as the current group's parameters sit in registers, so the HBM
// latency of a group hides under the arithmetic of the one before it.
typedef __attribute__((address_space(3))) void rqs_lds_void;
// cache policy of the parameter stream's LDS-DMA (aux bits of global_load_lds: 0 default, 2 = nt): the [N, n_live (3K-1)] tensor is read
// exactly once (MI355X_MICROARCH.md, nt-weights: once-read streams land 18 % sooner under nt) -- measured in DESIGN 6
#define SX_RQS_DMA_AUX 2
template <int BYTES>
__device__ __forceinline__ void rqs_dma_span(const float *__restrict__ g, float *lds_slice, int lane) {
    const char *gs = reinterpret_cast<const char *>(g) + lane * 16;
    char *ld = reinterpret_cast<char *>(lds_slice);      // wave-uniform (the LDS base of the copy travels in m0)
#pragma unroll
    for (int off = 0; off < BYTES; off += 1024) {
        if (off + 1024 <= BYTES || off + lane * 16 < BYTES)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(gs + off), (rqs_lds_void *)(ld + off), 16, 0, SX_RQS_DMA_AUX);
    }
}

// ---- straight-line evaluation for K = 16 (the BASELINE configuration): parameters in registers, selects only ----
// softmax numerators in place; returns the factor turning them into bin sizes (size_k = MIN + e_k * inv), :101-105
__device__ __forceinline__ float rqs16_softmax(float (&u)[16]) {
    float mx = u[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, u[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        u[k] = fast_exp(u[k] - mx);
        sum += u[k];
    }
    return (1.f - RQS_MIN_BIN * 16.f) * __builtin_amdgcn_rcpf(sum);
}

// the element's 47 parameters in registers (read up front: the LDS slice is then free for the next group's copy)
struct rqs16_regs { float us[16], uo[16], ud[15]; };
template <bool INVERSE>
__device__ __forceinline__ void rqs16_load(rqs16_regs &r, const float *__restrict__ p) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        r.us[k] = p[(INVERSE ? 16 : 0) + k];      // searched block: widths forward, heights inverse
        r.uo[k] = p[(INVERSE ? 0 : 16) + k];
    }
#pragma unroll
    for (int k = 0; k < 15; ++k) r.ud[k] = p[32 + k];
}
struct rqs16_disc_hook {      // for the error flag: a negative (or NaN) discriminant
    bool neg = false;
    template <int Y, class... T> __device__ __forceinline__ void at(float &v, T &...) { if constexpr (Y == RQS_Y_DISC) neg = !(v >= 0.f); }
};
template <bool INVERSE>
__device__ __forceinline__ void rqs16_eval(rqs16_regs &r, float xv, float left, float right, float bottom,
                                           float top, float &out, float &ljd, bool &bad_disc) {
    const float lo = INVERSE ? bottom : left, hi = INVERSE ? top : right;        // searched (input-side) interval
    const float lo2 = INVERSE ? left : bottom, hi2 = INVERSE ? right : top;      // the other block's interval
    const bool inside = (xv >= lo) && (xv <= hi);                                // :71
    const float xin = inside ? xv : lo;
    float (&us)[16] = r.us, (&uo)[16] = r.uo;
    // search sweep (:180-197): knots increase and x >= knot_j holds for a prefix of j
    const float inv_s = rqs16_softmax(us);
    int b = 0;
    float a_b = lo, a_n = hi, cs = 0.f;
#pragma unroll
    for (int j = 1; j <= 16; ++j) {
        cs += RQS_MIN_BIN + us[j - 1] * inv_s;
        const bool last = j == 16;
        const float knot = last ? hi : (hi - lo) * cs + lo;
        const bool ge = xin >= (last ? knot + RQS_EPS : knot);
        const bool take = ge && !last;
        b = take ? j : b;
        a_b = take ? knot : a_b;
        a_n = fminf(a_n, ge ? hi : knot);
    }
    // the other block at the found bin
    const float inv_o = rqs16_softmax(uo);
    float c_b = lo2, c_n = hi2;
    cs = 0.f;
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        cs += RQS_MIN_BIN + uo[j - 1] * inv_o;
        const float knot = (hi2 - lo2) * cs + lo2;
        c_b = (j == b) ? knot : c_b;
        c_n = (j == b + 1) ? knot : c_n;
    }
    float r_b = RQS_BOUNDARY_DERIV, r_n = RQS_BOUNDARY_DERIV;
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        const float v = r.ud[k];
        r_b = (k == b - 1) ? v : r_b;
        r_n = (k == b) ? v : r_n;
    }
    const float d_b = rqs_knot_deriv(r_b), d_n = rqs_knot_deriv(r_n);
    const float cw_b = INVERSE ? c_b : a_b, w_b = INVERSE ? c_n - c_b : a_n - a_b;
    const float ch_b = INVERSE ? a_b : c_b, h_b = INVERSE ? a_n - a_b : c_n - c_b;
    const float s_b = h_b * fast_rcp(w_b);
    bad_disc = false;
    if constexpr (INVERSE) {
        rqs16_disc_hook hk;
        const rqs_closed c = rqs_close<true>(d_b, d_n, s_b, cw_b, w_b, ch_b, h_b, xin, hk);
        bad_disc = inside && hk.neg;
        out = c.out;
        ljd = rqs_log_deriv<true>(c.dnum, c.den);
    } else {
        // rqs_close<false>'s expressions, kept in place: behind a call this kernel's SLP packing comes out differently and the dense
        // forward kernel goes from 141 to 163 VGPRs
        const float theta = (xin - cw_b) * fast_rcp(w_b);
        const float tomt = theta * (1.f - theta), omt = 1.f - theta;
        const float num = h_b * (s_b * (theta * theta) + d_b * tomt);
        const float den = s_b + (d_b + d_n - 2.f * s_b) * tomt;
        out = ch_b + num * fast_rcp(den);
        const float dnum = (s_b * s_b) * (d_n * (theta * theta) + 2.f * s_b * tomt + d_b * (omt * omt));
        ljd = rqs_log_deriv<false>(dnum, den);
    }
    out = inside ? out : xv;                     // :86-87
    ljd = inside ? ljd : 0.f;
}

template <bool BF16, bool INVERSE, bool ALIGNED>
__global__ __launch_bounds__(256) void rqs_kernel(const void *__restrict__ x, void *__restrict__ y,
                                                  float *__restrict__ ldj, float *__restrict__ ldiag,
                                                  const float *__restrict__ params, int64_t pstride,
                                                  const int32_t *__restrict__ live_idx, int l0, int n_live, int K,
                                                  float left, float right, float bottom, float top, int64_t n_rows,
                                                  int dim, int ldj_mode /*0 none, 1 direct (group), 2 row-aligned units*/,
                                                  int ldj_acc, float ldj_scale, uint32_t *__restrict__ err_flag) {
    const int P = 3 * K - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    float *sp = rqs_smem + (size_t)__builtin_amdgcn_readfirstlane(wave) * 64 * P;               // this wave's staging slice
    const int64_t n_elem = n_rows * n_live;
    // ALIGNED (ldj_mode 2): row-aligned work units, per-row sums without atomics; the dense variant is compiled without
    // any of it (its software-pipelined staging sits at 163 VGPRs = 3 waves per SIMD)
    const sx_units units = sx_make_units(n_rows, n_live, ALIGNED);
    const int64_t n_groups = units.n_units;
    const float lo_in = INVERSE ? bottom : left, hi_in = INVERSE ? top : right;
    const float bconst = logf(expf(1.f - RQS_MIN_DERIV) - 1.f);  // :81 boundary derivative constant (RQS_BOUNDARY_DERIV as libm rounds it)
    const float norm = 1.f - RQS_MIN_BIN * (float)K;
    // rows of parameters back to back (stride = n_live * P) and a 16-byte aligned base: 64 elements = 64*P floats
    const bool contig = (pstride == (int64_t)n_live * P) && ((reinterpret_cast<uintptr_t>(params) & 15) == 0);

    bool have_pf = false;       // this group's span is already on its way into the slice (K = 16 contiguous case)
    float x_pf = 0.f;           // ... and so is its input element (loads return in order: a load issued behind the copy would wait for it)
    auto load_x = [&](int64_t e) {
        const int64_t row = e / n_live;
        const int i = (int)(e - row * n_live);
        return sx_ld<BF16>(x, row * dim + (live_idx ? live_idx[i] : l0 + i));
    };
    for (int64_t grp = (int64_t)blockIdx.x * waves_per_block + wave; grp < n_groups;
         grp += (int64_t)gridDim.x * waves_per_block) {
      sx_row_ldj rl{ldj, ldj_acc, ldj_scale};
      for (int chunk = 0; chunk < (ALIGNED ? units.chunks : 1); ++chunk) {
        int64_t e0;
        int n_here;
        sx_unit_span(units, grp, chunk, n_rows, n_live, &e0, &n_here);      // dense units unless ALIGNED
        // ---- stage the elements' parameters: consecutive idx -> consecutive HBM addresses inside a row ----
        const int total = n_here * P;
        [[maybe_unused]] rqs16_regs pr;
        [[maybe_unused]] float x_dense = 0.f;
        const bool dense16 = !ALIGNED && contig && n_here == 64 && P == 47;
        if (dense16) {
            // the 64 elements' parameters are one contiguous, 16-byte aligned span of 12,032 B.  Software pipeline on
            // LDS-DMA: the span was requested one iteration ago; lift it into registers (47 conflict-free ds_read_b32 at the
            // odd stride), then request the NEXT group's span into the same slice: its latency hides under this group's
            // arithmetic, no VGPR holds data in flight (the register-prefetch form of round 1 sat at 163 VGPRs).
            if (!have_pf) { x_pf = load_x(e0 + lane); rqs_dma_span<64 * 47 * 4>(params + e0 * P, sp, lane); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            x_dense = x_pf;
            rqs16_load<INVERSE>(pr, sp + lane * P);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int64_t gnext = grp + (int64_t)gridDim.x * waves_per_block;
            have_pf = gnext < n_groups && ((gnext << 6) + 64 <= n_elem);      // dense units only (checked above)
            if (have_pf) { x_pf = load_x((gnext << 6) + lane); rqs_dma_span<64 * 47 * 4>(params + (gnext << 6) * P, sp, lane); }
        } else if (contig && n_here == 64 && (!ALIGNED || ((e0 * P) & 3) == 0)) {
            have_pf = false;
            const f32x4 *src = reinterpret_cast<const f32x4 *>(params + e0 * P);
            f32x4 *dst = reinterpret_cast<f32x4 *>(sp);
            for (int idx = lane; idx < 16 * P; idx += 64) dst[idx] = src[idx];
        } else {
            have_pf = false;
            for (int idx = lane; idx < total; idx += 64) {
                const int el = idx / P, q = idx - el * P;
                const int64_t e = e0 + el;
                const int64_t row = e / n_live;
                const int i = (int)(e - row * n_live);
                sp[idx] = params[row * pstride + (int64_t)i * P + q];
            }
        }
        // wave-private slice: the wave's own LDS writes are ordered before its reads by lgkmcnt (no barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int64_t e = e0 + lane;
        const bool valid = lane < n_here;
        const int64_t row = valid ? e / n_live : 0;
        const int i = valid ? (int)(e - row * n_live) : 0;
        const int col = live_idx ? live_idx[i] : l0 + i;
        const float xv = dense16 ? x_dense : (valid ? sx_ld<BF16>(x, row * dim + col) : lo_in);
        float out, ljd;
        if (K == 16) {      // wave-uniform: straight-line register path
            bool bad;
            if (!dense16) rqs16_load<INVERSE>(pr, sp + (valid ? lane : 0) * P);
            rqs16_eval<INVERSE>(pr, xv, left, right, bottom, top, out, ljd, bad);
            if (valid && bad && err_flag) __hip_atomic_fetch_or(err_flag, SX_FLAG_RQS_NEG_DISCRIMINANT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
        const bool inside = (xv >= lo_in) && (xv <= hi_in);                    // :71 closed interval
        const float xin = inside ? xv : lo_in;
        const float *uw = sp + (valid ? lane : 0) * P, *uh = uw + K, *ud = uh + K;

        // ---- softmax normalisers (F.softmax: exp(u - max) / sum), :101,104 -------------------------------
        float mw = uw[0], mh = uh[0];
        for (int k = 1; k < K; ++k) { mw = fmaxf(mw, uw[k]); mh = fmaxf(mh, uh[k]); }
        float sw = 0.f, sh = 0.f;
        for (int k = 0; k < K; ++k) { sw += expf(uw[k] - mw); sh += expf(uh[k] - mh); }

        // ---- knots (:180-192) + bin search (search_sorted.py:4-5) in one sweep ----------------------------
        // edge_0 = lower bound <= x always; b = last j with x >= edge_j, edge_K = upper + 1e-6.
        int b = 0;
        float cw_b = left, ch_b = bottom, cw_n = right, ch_n = top;           // knots at b and b+1
        bool have_next = false;
        float csw = 0.f, csh = 0.f;
        for (int j = 1; j <= K; ++j) {
            const float wk = RQS_MIN_BIN + norm * (expf(uw[j - 1] - mw) / sw);   // :102
            const float hk = RQS_MIN_BIN + norm * (expf(uh[j - 1] - mh) / sh);   // :105
            csw += wk;                                                           // cumsum :180
            csh += hk;                                                           // cumsum :187
            const float kw = (j < K) ? (right - left) * csw + left : right;      // :182-184 (ends pinned)
            const float kh = (j < K) ? (top - bottom) * csh + bottom : top;      // :189-191
            const float edge = INVERSE ? kh : kw;
            const bool ge = xin >= ((j < K) ? edge : edge + RQS_EPS);
            if (ge && j < K) { b = j; cw_b = kw; ch_b = kh; }                    // j == K: clamp to last bin
            else if (!ge && !have_next) { cw_n = kw; ch_n = kh; have_next = true; }
        }
        const float w_b = cw_n - cw_b;                                           // :185
        const float h_b = ch_n - ch_b;                                           // :192
        const float s_b = h_b / w_b;                                             // :203-204
        const float d_b = RQS_MIN_DERIV + sx_softplus(b == 0 ? bconst : ud[b - 1]);        // :107, :206
        const float d_n = RQS_MIN_DERIV + sx_softplus(b + 1 == K ? bconst : ud[b]);        // :207

        if constexpr (INVERSE) {
            const float dy = xin - ch_b;
            const float q = d_b + d_n - 2.f * s_b;
            const float a = dy * q + h_b * (s_b - d_b);                          // :212-215
            const float bb = h_b * d_b - dy * q;                                 // :216-219
            const float c = -s_b * dy;                                           // :220
            const float disc = bb * bb - 4.f * a * c;                            // :222
            if (valid && inside && !(disc >= 0.f) && err_flag) __hip_atomic_fetch_or(err_flag, SX_FLAG_RQS_NEG_DISCRIMINANT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const float root = (2.f * c) / (-bb - sqrtf(disc));                  // :225
            out = root * w_b + cw_b;                                             // :226
            const float tomt = root * (1.f - root);                              // :228
            const float den = s_b + q * tomt;                                    // :229-230
            const float omr = 1.f - root;
            const float dnum = (s_b * s_b) * (d_n * (root * root) + 2.f * s_b * tomt + d_b * (omr * omr));
            ljd = -logf(dnum) + 2.f * logf(den);                                 // :234 (sign already flipped)
        } else {
            const float theta = (xin - cw_b) / w_b;                              // :236
            const float tomt = theta * (1.f - theta);                            // :237
            const float num = h_b * (s_b * (theta * theta) + d_b * tomt);        // :239-240
            const float den = s_b + (d_b + d_n - 2.f * s_b) * tomt;              // :241-242
            out = ch_b + num / den;                                              // :243
            const float omt = 1.f - theta;
            const float dnum = (s_b * s_b) * (d_n * (theta * theta) + 2.f * s_b * tomt + d_b * (omt * omt));
            ljd = logf(dnum) - 2.f * logf(den);                                  // :248
        }
        if (!inside) { out = xv; ljd = 0.f; }                                    // :86-87 linear tails
        }
        if (valid) {
            sx_st<BF16>(y, row * dim + col, out);
            if (ldiag) ldiag[row * dim + col] = ljd;
        }
        if (ldj_mode == 1) rl.group(valid ? ljd : 0.f, n_live, valid && (lane & (n_live - 1)) == 0, row);
        if constexpr (ALIGNED) rl.chunk(units, valid ? ljd : 0.f, i, n_live, valid, row);
      }
      if constexpr (ALIGNED) rl.finish(units, lane, grp);
    }
}

extern "C" int sx_rqs_coupling(const void *x, void *y, float *ldj, float *ldiag, const float *params,
                               int64_t params_stride, const int32_t *live_idx, int32_t live_start, int32_t n_live,
                               int32_t n_bins, float left, float right, float bottom, float top, int64_t n_rows,
                               int32_t dim, int32_t dtype, int32_t reverse, int32_t ldj_accumulate, float ldj_scale,
                               uint32_t *err_flag, void *stream) {
    SX_REQUIRE(x && y && params, "sx_rqs_coupling: null pointer");
    SX_REQUIRE(dim > 0 && n_live >= 0 && n_live <= dim && n_rows >= 0, "sx_rqs_coupling: bad sizes");
    SX_REQUIRE(n_bins >= 1, "sx_rqs_coupling: n_bins must be >= 1");
    SX_REQUIRE(dtype == SX_F32 || dtype == SX_BF16, "sx_rqs_coupling: bad dtype");
    // rational_quadratic_spline.py:96-99
    SX_REQUIRE(1e-3 * n_bins <= 1.0, "Minimal bin width too large for the number of bins");
    SX_REQUIRE(right > left && top > bottom, "sx_rqs_coupling: empty domain");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    sx_spline_plan pl;
    const int rc = sx_plan_spline("sx_rqs_coupling", x, y, ldj, ldiag, live_idx, live_start, n_live, n_bins, 3 * n_bins - 1, n_rows, dim,
                                  dtype, ldj_accumulate, st,
                                  [](auto BF, auto INV, auto AL) { return (const void *)rqs_kernel<BF(), INV(), AL()>; }, &pl);
    if (rc != SX_OK || pl.grid == 0) return rc;
    sx_dispatch(dtype == SX_BF16, reverse != 0, pl.ldj_mode == 2, [&](auto BF, auto INV, auto AL) {
        hipLaunchKernelGGL((rqs_kernel<BF(), INV(), AL()>), dim3(pl.grid), dim3(pl.sl.block), pl.sl.lds, st, x, y, ldj, ldiag, params,
                           params_stride, live_idx, live_start, n_live, n_bins, left, right, bottom, top, n_rows, dim,
                           pl.ldj_mode, ldj_accumulate, ldj_scale, err_flag);
    });
    SX_LAUNCH_CHECK();
    return SX_OK;
}

// =====================================================================================================
// Monotone cubic spline (spline_type='cubic', the reference's default), element-wise kernel.
//
// Replaces unconstrained_cubic_spline + cubic_spline (stribor/util/cubic_spline.py:21-251) and searchsorted:
// 2 softmax, 2 cumsum, pads, the Steffen-style knot derivatives (:117-132), the per-bin cubic coefficients
// (:134-137), the bin search, 6 gathers and the forward polynomial / inverse cubic solve (one-root Cardano form,
// three-root trigonometric form with the in-bin root picked, quadratic fallback for |a| < 1e-3) become one pass:
// one lane = one (row, live column) element.  Same CDNA4 mapping as rqs_kernel: the wave's 64 elements own one
// contiguous span of 64*(2K+2) parameter floats, copied coalesced into the wave's LDS slice; each lane's slice is
// padded to an odd stride (2K+3 dwords) so the 32 lanes of a ds_read_b32 group hit 32 banks, and the lane
// overwrites its un-normalised widths / heights with the normalised ones in place.
// =====================================================================================================
#include "sx_cubic_core.h"


// Forward log-derivative log f'(x) of the monotone cubic spline at normalised input `xin` from the element's
// (exp'ed) widths / heights ew[k], eh[k] with their softmax factors nw, nh and the two raw boundary-derivative parameters
// (cubic_spline.py:103-137, 229-237): the bin is searched by widths, as the forward pass does.  Used by the inverse
// kernel's reference mode when the inverted point does not land in the bin it was solved in (rare).
template <class GW, class GH>
__device__ __forceinline__ float cubic_forward_logderiv(GW ew, GH eh, float nw, float nh, float dpar0, float dpar1, int K,
                                                        float xin) {
    int b = 0;
    float cw_b = 0.f, w_b = 0.f, h_b = 0.f, w_m = 1.f, h_m = 1.f, w_p = 1.f, h_p = 1.f;
    float cw = 0.f, w_last = 1.f, h_last = 1.f;
    bool need_next = false;
    for (int k = 0; k < K; ++k) {
        const float wk = CUBIC_MIN_BIN + nw * ew(k);
        const float hk = CUBIC_MIN_BIN + nh * eh(k);
        if (xin >= cw) { b = k; cw_b = cw; w_b = wk; h_b = hk; w_m = w_last; h_m = h_last; need_next = true; }
        else if (need_next) { w_p = wk; h_p = hk; need_next = false; }
        w_last = wk; h_last = hk;
        cw += wk;
    }
    return cubic_logderiv_at(b, K, cw_b, w_b, h_b, w_m, h_m, w_p, h_p, dpar0, dpar1, xin);
}
template <bool BF16, bool INVERSE, bool ALIGNED>
__global__ __launch_bounds__(256, 4) void cubic_kernel(const void *__restrict__ x, void *__restrict__ y,
                                                    float *__restrict__ ldj, float *__restrict__ ldiag,
                                                    const float *__restrict__ params, int64_t pstride,
                                                    const int32_t *__restrict__ live_idx, int l0, int n_live, int K,
                                                    float lower, float upper, float log_span, int64_t n_rows, int dim,
                                                    int ldj_mode /*0 none, 1 direct (group), 2 row-aligned units*/, int ldj_acc,
                                                    float ldj_scale, int ref_ldj) {
    const int P = 2 * K + 2, PS = P | 1;                         // padded (odd) per-lane stride
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    float *sp = rqs_smem + (size_t)__builtin_amdgcn_readfirstlane(wave) * 64 * PS;
    const sx_units units = sx_make_units(n_rows, n_live, ALIGNED);
    const int64_t n_elem = n_rows * n_live;
    const int64_t n_groups = units.n_units;
    const float norm = 1.f - CUBIC_MIN_BIN * (float)K;          // :104, :111
    bool have_pf = false;       // dense K = 16 pipeline: this group's span and input element are already on their way
    float x_pf = 0.f;
    auto load_x = [&](int64_t e) {
        const int64_t row = e / n_live;
        const int i = (int)(e - row * n_live);
        return sx_ld<BF16>(x, row * dim + (live_idx ? live_idx[i] : l0 + i));
    };
    const float span = upper - lower;                            // right - left = top - bottom
    const float inv_span = 1.0f / span;
    const bool contig = pstride == (int64_t)n_live * P;
    const float inv_P = 1.0f / (float)P;

    for (int64_t grp = (int64_t)blockIdx.x * waves_per_block + wave; grp < n_groups;
         grp += (int64_t)gridDim.x * waves_per_block) {
      sx_row_ldj rl{ldj, ldj_acc, ldj_scale};
      for (int chunk = 0; chunk < (ALIGNED ? units.chunks : 1); ++chunk) {
        int64_t e0;
        int n_here;
        sx_unit_span(units, grp, chunk, n_rows, n_live, &e0, &n_here);      // dense units unless ALIGNED
        const int total = n_here * P;
        // ---- stage: consecutive idx -> consecutive HBM addresses (one contiguous span when rows are packed) ----
        // K even (P / 2 odd): the span is copied as it is (16 B per lane in, 16 B out) and a lane reads its element's parameters
        // as 8-byte pairs at a stride of P / 2 pairs -- odd, so the 64-bit reads are conflict-free without padding, and the
        // 270 instructions per element of index arithmetic + scalar LDS writes of the padded form reduce to 17
        // (both directions: the inverse's reference-mode re-evaluation works from the registers)
        const bool lin = K == 16 && contig && n_here == 64 && (!ALIGNED || ((e0 * P) & 3) == 0) &&
                         ((reinterpret_cast<uintptr_t>(params) & 15) == 0);
        const bool dma16 = !ALIGNED && lin;
        [[maybe_unused]] float rw[16], rh[16], x_dense = 0.f;
        float dpar0 = 0.f, dpar1 = 0.f;
        typedef float f32pair __attribute__((ext_vector_type(2)));
        auto load16 = [&](const float *q) {                      // 8-byte aligned pairs
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                const f32pair a = *reinterpret_cast<const f32pair *>(q + k), c2 = *reinterpret_cast<const f32pair *>(q + 16 + k);
                rw[k] = a.x; rw[k + 1] = a.y; rh[k] = c2.x; rh[k + 1] = c2.y;
            }
            const f32pair d2 = *reinterpret_cast<const f32pair *>(q + 32);
            dpar0 = d2.x; dpar1 = d2.y;
        };
        if (dma16) {
            // software pipeline on LDS-DMA (see rqs_kernel): the span requested one iteration ago is lifted into registers,
            // then the next group's span is requested into the same slice and lands under this group's arithmetic
            if (!have_pf) { x_pf = load_x(e0 + lane); rqs_dma_span<64 * 34 * 4>(params + e0 * P, sp, lane); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            x_dense = x_pf;
            load16(sp + lane * P);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int64_t gnext = grp + (int64_t)gridDim.x * waves_per_block;
            have_pf = gnext < n_groups && ((gnext << 6) + 64 <= n_elem);
            if (have_pf) { x_pf = load_x((gnext << 6) + lane); rqs_dma_span<64 * 34 * 4>(params + (gnext << 6) * P, sp, lane); }
        } else if (lin) {
            have_pf = false;
            const f32x4 *src = reinterpret_cast<const f32x4 *>(params + e0 * P);
            f32x4 *dst = reinterpret_cast<f32x4 *>(sp);
            for (int i4 = lane; i4 < 16 * P; i4 += 64) dst[i4] = src[i4];
        } else if (contig && n_here == 64 && (P & 1) == 0 && (!ALIGNED || ((e0 * P) & 3) == 0) && ((reinterpret_cast<uintptr_t>(params) & 15) == 0)) {
            // 64*P floats = 16*P float4, 16-byte aligned (P even): vector loads, scalar LDS writes into the padded rows
            have_pf = false;
            const f32x4 *src = reinterpret_cast<const f32x4 *>(params + e0 * P);
            for (int i4 = lane; i4 < 16 * P; i4 += 64) {
                const f32x4 v = src[i4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int idx = 4 * i4 + c;
                    const int el = (int)(((float)idx + 0.5f) * inv_P), q = idx - el * P;
                    sp[el * PS + q] = v[c];
                }
            }
        } else {
        have_pf = false;
        for (int idx = lane; idx < total; idx += 64) {
            const int el = (int)(((float)idx + 0.5f) * inv_P), q = idx - el * P;       // idx / P, exact for idx < 2^22
            float v;
            if (contig) v = params[e0 * P + idx];
            else {
                const int64_t e = e0 + el;
                const int64_t row = e / n_live;
                v = params[row * pstride + (int64_t)(e - row * n_live) * P + q];
            }
            sp[el * PS + q] = v;
        }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int64_t e = e0 + lane;
        const bool valid = lane < n_here;
        const int64_t row = valid ? e / n_live : 0;
        const int i = valid ? (int)(e - row * n_live) : 0;
        const int col = live_idx ? live_idx[i] : l0 + i;
        const float xv = dma16 ? x_dense : (valid ? sx_ld<BF16>(x, row * dim + col) : lower);
        const bool inside = (xv >= lower) && (xv <= upper);      // :40 closed interval
        const float xin = ((inside ? xv : lower) - lower) * inv_span;        // :98-101
        float *p = sp + (valid ? lane : 0) * (lin ? P : PS);     // [0,K) widths, [K,2K) heights, 2K / 2K+1 derivatives

        // ---- normalised widths / heights, running cumsums (:103-115) and the bin search (search_sorted.py:4-5) in
        //      one sweep that also keeps the widths / heights of bins b-1, b, b+1 ----------------------------------
        int b = 0;
        float cw_b = 0.f, ch_b = 0.f, w_b = 0.f, h_b = 0.f, w_m = 1.f, h_m = 1.f, w_p = 1.f, h_p = 1.f;
        float nw_k = 0.f, nh_k = 0.f;          // softmax factors, kept for the reference-mode re-evaluation
        auto sweep = [&](auto get_w, auto get_h, auto set_w, auto set_h, int KK) {
            float mw = get_w(0), mh = get_h(0);
            for (int k = 1; k < KK; ++k) { mw = fmaxf(mw, get_w(k)); mh = fmaxf(mh, get_h(k)); }
            float sw = 0.f, sh = 0.f;
            for (int k = 0; k < KK; ++k) {      // exp once per parameter (v_exp_f32 with a compensated argument)
                const float ew = fast_exp(get_w(k) - mw), eh = fast_exp(get_h(k) - mh);
                set_w(k, ew);
                set_h(k, eh);
                sw += ew;
                sh += eh;
            }
            const float nw = norm * fast_rcp(sw), nh = norm * fast_rcp(sh);         // one reciprocal per softmax
            nw_k = nw; nh_k = nh;
            float cw = 0.f, ch = 0.f, w_last = 1.f, h_last = 1.f;
            bool need_next = false;
            for (int k = 0; k < KK; ++k) {
                const float wk = CUBIC_MIN_BIN + nw * get_w(k);
                const float hk = CUBIC_MIN_BIN + nh * get_h(k);
                if (xin >= (INVERSE ? ch : cw)) {               // lower knot of bin k (knot 0 = 0): edges only grow
                    b = k; cw_b = cw; ch_b = ch; w_b = wk; h_b = hk; w_m = w_last; h_m = h_last; need_next = true;
                } else if (need_next) {
                    w_p = wk; h_p = hk; need_next = false;
                }
                w_last = wk; h_last = hk;
                cw += wk;
                ch += hk;
            }
        };
        if (K == 16) {          // wave-uniform: parameters in registers, fully unrolled, selects only
            if (dma16) {
            } else if (lin) {
                load16(p);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) { rw[k] = p[k]; rh[k] = p[16 + k]; }
                dpar0 = p[32]; dpar1 = p[33];
            }
            float mw = rw[0], mh = rh[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) { mw = fmaxf(mw, rw[k]); mh = fmaxf(mh, rh[k]); }
            float sw = 0.f, sh = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                rw[k] = fast_exp(rw[k] - mw); rh[k] = fast_exp(rh[k] - mh);
                sw += rw[k]; sh += rh[k];
            }
            const float nw = norm * fast_rcp(sw), nh = norm * fast_rcp(sh);
            nw_k = nw; nh_k = nh;
            // Two-level search (as the fused kernel's cub_search16): the group of four bins from the groups' sums, then the bin and
            // its two neighbours among the six sizes around the group -- ~110 VALU instructions instead of ~260 for the 16-step
            // sweep.  Named scalars, not array elements, feed the selects (a select between two array elements becomes a select
            // of addresses and sends the array to scratch).
#define CW_(k) const float w##k = CUBIC_MIN_BIN + nw * rw[k], h##k = CUBIC_MIN_BIN + nh * rh[k]
            CW_(0); CW_(1); CW_(2); CW_(3); CW_(4); CW_(5); CW_(6); CW_(7); CW_(8); CW_(9); CW_(10); CW_(11); CW_(12); CW_(13); CW_(14); CW_(15);
#undef CW_
            const float Sw0 = (w0 + w1) + (w2 + w3), Sw1 = (w4 + w5) + (w6 + w7), Sw2 = (w8 + w9) + (w10 + w11);
            const float Sh0 = (h0 + h1) + (h2 + h3), Sh1 = (h4 + h5) + (h6 + h7), Sh2 = (h8 + h9) + (h10 + h11);
            const float Cw1 = Sw0, Cw2 = Sw0 + Sw1, Cw3 = (Sw0 + Sw1) + Sw2, Ch1 = Sh0, Ch2 = Sh0 + Sh1, Ch3 = (Sh0 + Sh1) + Sh2;
            const bool m1 = xin >= (INVERSE ? Ch1 : Cw1), m2 = xin >= (INVERSE ? Ch2 : Cw2), m3 = xin >= (INVERSE ? Ch3 : Cw3);
            const float bw = m3 ? Cw3 : (m2 ? Cw2 : (m1 ? Cw1 : 0.f)), bh = m3 ? Ch3 : (m2 ? Ch2 : (m1 ? Ch1 : 0.f));
#define PK_(a, b_, c_, d_) (m3 ? a : (m2 ? b_ : (m1 ? c_ : d_)))
            const float zw0 = PK_(w11, w7, w3, w0), zw1 = PK_(w12, w8, w4, w0), zw2 = PK_(w13, w9, w5, w1), zw3 = PK_(w14, w10, w6, w2);
            const float zw4 = PK_(w15, w11, w7, w3), zw5 = PK_(w15, w12, w8, w4);
            const float zh0 = PK_(h11, h7, h3, h0), zh1 = PK_(h12, h8, h4, h0), zh2 = PK_(h13, h9, h5, h1), zh3 = PK_(h14, h10, h6, h2);
            const float zh4 = PK_(h15, h11, h7, h3), zh5 = PK_(h15, h12, h8, h4);
#undef PK_
            const float kw1 = bw + zw1, kw2 = kw1 + zw2, kw3 = kw2 + zw3, kh1 = bh + zh1, kh2 = kh1 + zh2, kh3 = kh2 + zh3;
            const bool g1 = xin >= (INVERSE ? kh1 : kw1), g2 = xin >= (INVERSE ? kh2 : kw2), g3 = xin >= (INVERSE ? kh3 : kw3);
#define PL_(a, b_, c_, d_) (g3 ? a : (g2 ? b_ : (g1 ? c_ : d_)))
            b = (m3 ? 12 : (m2 ? 8 : (m1 ? 4 : 0))) + PL_(3, 2, 1, 0);
            cw_b = PL_(kw3, kw2, kw1, bw); ch_b = PL_(kh3, kh2, kh1, bh);
            w_m = PL_(zw3, zw2, zw1, zw0); w_b = PL_(zw4, zw3, zw2, zw1); w_p = PL_(zw5, zw4, zw3, zw2);
            h_m = PL_(zh3, zh2, zh1, zh0); h_b = PL_(zh4, zh3, zh2, zh1); h_p = PL_(zh5, zh4, zh3, zh2);
#undef PL_
        } else {
            sweep([&](int k) { return p[k]; }, [&](int k) { return p[K + k]; }, [&](int k, float v) { p[k] = v; },
                  [&](int k, float v) { p[K + k] = v; }, K);
            dpar0 = p[2 * K]; dpar1 = p[2 * K + 1];
        }
        // ---- knot derivatives of bin b (:117-132) and its cubic (:134-137) -----------------------------------
        const float rcw = (b == K - 1) ? 1.f : cw_b + w_b;                                 // :107 (last knot pinned)
        const cubic_coef cf = cubic_bin_coef(b, K, w_b, h_b, w_m, h_m, w_p, h_p, dpar0, dpar1);
        const float a = cf.a, bb = cf.bb, c = cf.c;
        const float d = ch_b;                                                              // :137

        float out, ljd;
        if constexpr (INVERSE) {
            float so = cubic_invert(a, bb, c, d, xin, cw_b, rcw);
            float o;
            o = so + cw_b;
            ljd = -fast_log(3.f * a * (so * so) + 2.f * bb * so + c);                    // :225-227
            // (an input inside the closed domain has its pre-image inside it too: without the clamp an input ON the bound -- common
            //  with bf16 storage, whose grid contains +-3 -- can come back one ulp outside, and the reference-mode log-det below
            //  would then be the tails' 0 instead of -log f')
            out = fminf(fmaxf(o * span + lower, lower), upper);                            // :235
            ljd = (ljd - log_span) + log_span;                                             // :236 (two fp32 roundings there)
            if (ref_ldj) {
                // Reference mode (a coupling's inverse_and_log_det_jacobian): the reference does NOT use the inverse's own
                // log-derivative -- Transform.inverse_and_log_det_jacobian (flow.py:42-47) evaluates MINUS the FORWARD
                // log-det at the inverted point.  The two agree to rounding inside a bin, but differ where the inverted
                // point lands an ulp outside the domain (forward: linear tail, 0) or in a neighbouring bin, and where the
                // fp32 cubic solve breaks down.  Re-evaluate the forward log-derivative at x' = out exactly as the forward
                // kernel would: in the solved bin when x' lies inside it (no second sweep), else by a full search.
                const bool in2 = inside && (out >= lower) && (out <= upper);
                const float xin2 = ((in2 ? out : lower) - lower) * inv_span;
                const bool same_bin = (xin2 >= cw_b) && (b == K - 1 || xin2 < cw_b + w_b);
                float lf;
                {
                    const float t2 = xin2 - cw_b;
                    lf = fast_log(3.f * a * (t2 * t2) + 2.f * bb * t2 + c);
                }
                const bool slow = valid && in2 && !same_bin;
                if (__builtin_amdgcn_ballot_w64(slow)) {
                    if (slow) {
                        if (K == 16) {          // the exp'ed widths / heights are still in registers (the LDS slice may already
                                                // be receiving the next group)
                            lf = cubic_select_forward_logderiv<false>([&](int k) { return rw[k]; }, [&](int k) { return rh[k]; }, nw_k, nh_k, dpar0,
                                                                       dpar1, 16, xin2);
                        } else {                // the generic path left exp(u - max) in place of the raw widths / heights
                            lf = cubic_forward_logderiv([&](int k) { return p[k]; }, [&](int k) { return p[K + k]; }, nw_k, nh_k,
                                                        dpar0, dpar1, K, xin2);
                        }
                    }
                }
                lf = (lf + log_span) - log_span;                                           // :239 (forward's two roundings)
                ljd = in2 ? -lf : 0.f;                                                     // :46-48 tails; flow.py:47 negation
            }
        } else {
            const float t = xin - cw_b;                                                    // :229
            out = a * (t * t * t) + bb * (t * t) + c * t + d;                              // :230-233
            ljd = fast_log(3.f * a * (t * t) + 2.f * bb * t + c);                        // :235-237
            out = out * span + lower;                                                      // :238
            ljd = (ljd + log_span) - log_span;                                             // :239
        }
        if (!inside) { out = xv; ljd = 0.f; }                                              // :46-48 linear tails
        if (valid) {
            sx_st<BF16>(y, row * dim + col, out);
            if (ldiag) ldiag[row * dim + col] = ljd;
        }
        if (ldj_mode == 1) rl.group(valid ? ljd : 0.f, n_live, valid && (lane & (n_live - 1)) == 0, row);
        if constexpr (ALIGNED) rl.chunk(units, valid ? ljd : 0.f, i, n_live, valid, row);
      }
      if constexpr (ALIGNED) rl.finish(units, lane, grp);
    }
}

extern "C" int sx_cubic_coupling(const void *x, void *y, float *ldj, float *ldiag, const float *params,
                                 int64_t params_stride, const int32_t *live_idx, int32_t live_start, int32_t n_live,
                                 int32_t n_bins, float lower, float upper, int64_t n_rows, int32_t dim, int32_t dtype,
                                 int32_t reverse, int32_t ldj_accumulate, float ldj_scale, void *stream) {
    SX_REQUIRE(x && y && params, "sx_cubic_coupling: null pointer");
    SX_REQUIRE(dim > 0 && n_live >= 0 && n_live <= dim && n_rows >= 0, "sx_cubic_coupling: bad sizes");
    SX_REQUIRE(n_bins >= 1, "sx_cubic_coupling: n_bins must be >= 1");
    SX_REQUIRE(dtype == SX_F32 || dtype == SX_BF16, "sx_cubic_coupling: bad dtype");
    SX_REQUIRE(1e-2 * n_bins <= 1.0, "Minimal bin width too large for the number of bins");       // cubic_spline.py:93-96
    SX_REQUIRE(upper > lower, "sx_cubic_coupling: empty domain");
    if (n_rows == 0) return SX_OK;
    hipStream_t st = sx_stream(stream);
    const float log_span = (float)log((double)upper - (double)lower);      // math.log(top - bottom), cast as torch does
    sx_spline_plan pl;
    const int rc = sx_plan_spline("sx_cubic_coupling", x, y, ldj, ldiag, live_idx, live_start, n_live, n_bins, (2 * n_bins + 2) | 1, n_rows,
                                  dim, dtype, ldj_accumulate, st,
                                  [](auto BF, auto INV, auto AL) { return (const void *)cubic_kernel<BF(), INV(), AL()>; }, &pl);
    if (rc != SX_OK || pl.grid == 0) return rc;
    sx_dispatch(dtype == SX_BF16, reverse != 0, pl.ldj_mode == 2, [&](auto BF, auto INV, auto AL) {
        hipLaunchKernelGGL((cubic_kernel<BF(), INV(), AL()>), dim3(pl.grid), dim3(pl.sl.block), pl.sl.lds, st, x, y, ldj, ldiag, params,
                           params_stride, live_idx, live_start, n_live, n_bins, lower, upper, log_span, n_rows, dim,
                           pl.ldj_mode, ldj_accumulate, ldj_scale, (int)(reverse == 2));
    });
    SX_LAUNCH_CHECK();
    return SX_OK;
}

// =====================================================================================================
// Backward of the rational-quadratic spline in the INVERSE direction (the direction log_prob evaluates):
// given dL/d(out) and dL/d(ljd) of  (out, ljd) = rqs^{-1}(y; uw, uh, ud)  per element, produce dL/dy and the
// gradient of all 3K-1 un-normalised parameters.  Reverse mode through exactly the operations of the forward
// kernel (rational_quadratic_spline.py:101-107, 180-234): quadratic root -> (a, b, c) -> (knots of bin b, its two
// derivatives) -> cumsum -> softmax / softplus.  The bin index is piecewise constant: no gradient.  Elements in the
// linear tails pass dL/d(out) through and contribute nothing to the parameters.
// Layout / staging as rqs_kernel; the lane overwrites its parameter slice with the gradients, which then leave
// coalesced in the parameter tensor's own layout.  fp32 only (training state).
// =====================================================================================================
#include "sx_rqs_bwd.h"

template <bool INVERSE>
__global__ __launch_bounds__(256) void rqs_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gout,
                                                              const float *__restrict__ gldj,
                                                              const float *__restrict__ gldiag,
                                                              const float *__restrict__ params, int64_t pstride,
                                                              float *__restrict__ gx, float *__restrict__ gparams,
                                                              const int32_t *__restrict__ live_idx, int l0, int n_live,
                                                              int K, float left, float right, float bottom, float top,
                                                              int64_t n_rows, int dim, float ldj_scale) {
    const int P = 3 * K - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    float *sp = rqs_smem + (size_t)wave * 64 * P;
    const int64_t n_elem = n_rows * n_live;
    const int64_t n_groups = (n_elem + 63) >> 6;
    const bool contig = pstride == (int64_t)n_live * P;
    const float inv_P = 1.0f / (float)P;
    for (int64_t grp = (int64_t)blockIdx.x * waves_per_block + wave; grp < n_groups;
         grp += (int64_t)gridDim.x * waves_per_block) {
        const int64_t e0 = grp << 6;
        const int n_here = (int)((n_elem - e0) < 64 ? (n_elem - e0) : 64);
        const int total = n_here * P;
        if (contig && n_here == 64 && ((reinterpret_cast<uintptr_t>(params) & 15) == 0)) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(params + e0 * P);     // 64*P floats = 16*P float4
            f32x4 *dst = reinterpret_cast<f32x4 *>(sp);
            for (int i4 = lane; i4 < 16 * P; i4 += 64) dst[i4] = src[i4];
        } else {
            for (int idx = lane; idx < total; idx += 64) {
                const int el = (int)(((float)idx + 0.5f) * inv_P), q = idx - el * P;  // idx / P, exact for idx < 2^22
                const int64_t e = e0 + el;
                const int64_t row = e / n_live;
                sp[idx] = params[row * pstride + (int64_t)(e - row * n_live) * P + q];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int64_t e = e0 + lane;
        const bool valid = e < n_elem;
        const int64_t row = valid ? e / n_live : 0;
        const int i = valid ? (int)(e - row * n_live) : 0;
        const int col = live_idx ? live_idx[i] : l0 + i;
        const float xv = valid ? x[row * dim + col] : (INVERSE ? bottom : left);
        const float Ao = valid ? gout[row * dim + col] : 0.f;            // dL/d out
        // dL/d ljd: the row sum's adjoint (+ the element's own, when the caller differentiates log_diag_jacobian)
        const float Al = valid ? ((gldj ? gldj[row] : 0.f) + (gldiag ? gldiag[row * dim + col] : 0.f)) * ldj_scale : 0.f;
        float *uw = sp + (valid ? lane : 0) * P;
        const float gxe = rqs_bwd_element<INVERSE>(uw, K, xv, Ao, Al, left, right, bottom, top, valid);
        if (valid) gx[row * dim + col] = gxe;

        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (n_here == 64 && ((reinterpret_cast<uintptr_t>(gparams) & 15) == 0)) {
            f32x4 *dst = reinterpret_cast<f32x4 *>(gparams + e0 * P);             // [n_rows, n_live * P], packed
            const f32x4 *src = reinterpret_cast<const f32x4 *>(sp);
            for (int i4 = lane; i4 < 16 * P; i4 += 64) dst[i4] = src[i4];
        } else {
            for (int idx = lane; idx < total; idx += 64) gparams[e0 * P + idx] = sp[idx];
        }
    }
}

static int rqs_bwd_launch(bool inverse, const float *x, const float *gout, const float *gldj, const float *gldiag, const float *params,
                                  int64_t params_stride, float *gx, float *gparams, const int32_t *live_idx,
                                  int32_t live_start, int32_t n_live, int32_t n_bins, float left, float right,
                                  float bottom, float top, int64_t n_rows, int32_t dim, float ldj_scale, void *stream) {
    SX_REQUIRE(x && gout && (gldj || gldiag) && params && gx && gparams, "sx_rqs_*_bwd: null pointer");
    SX_REQUIRE(dim > 0 && n_live > 0 && n_live <= dim && n_rows >= 0 && n_bins >= 1, "sx_rqs_*_bwd: bad sizes");
    SX_REQUIRE(right > left && top > bottom, "sx_rqs_*_bwd: empty domain");
    if (n_rows == 0) return SX_OK;
    const sx_slice_plan sl = sx_plan_slices(3 * n_bins - 1);
    SX_REQUIRE(sl.lds <= 160 * 1024, "sx_rqs_*_bwd: n_bins %d needs %zu B of LDS per wave", n_bins, sl.lds);
    if (sl.lds > 48 * 1024) {
        (void)hipFuncSetAttribute((const void *)rqs_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds);
        (void)hipFuncSetAttribute((const void *)rqs_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds);
    }
    const int grid = sl.grid((n_rows * n_live + 63) / 64);
    sx_dispatch(inverse, [&](auto INV) {
        hipLaunchKernelGGL(rqs_bwd_kernel<INV()>, dim3(grid), dim3(sl.block), sl.lds, sx_stream(stream), x, gout, gldj, gldiag, params,
                           params_stride, gx, gparams, live_idx, live_start, n_live, n_bins, left, right, bottom, top, n_rows,
                           dim, ldj_scale);
    });
    SX_LAUNCH_CHECK();
    return SX_OK;
}

extern "C" int sx_rqs_inverse_bwd(const float *x, const float *gout, const float *gldj, const float *gldiag, const float *params,
                                  int64_t params_stride, float *gx, float *gparams, const int32_t *live_idx,
                                  int32_t live_start, int32_t n_live, int32_t n_bins, float left, float right,
                                  float bottom, float top, int64_t n_rows, int32_t dim, float ldj_scale, void *stream) {
    return rqs_bwd_launch(true, x, gout, gldj, gldiag, params, params_stride, gx, gparams, live_idx, live_start, n_live, n_bins, left, right,
                          bottom, top, n_rows, dim, ldj_scale, stream);
}
extern "C" int sx_rqs_forward_bwd(const float *x, const float *gout, const float *gldj, const float *gldiag, const float *params,
                                  int64_t params_stride, float *gx, float *gparams, const int32_t *live_idx,
                                  int32_t live_start, int32_t n_live, int32_t n_bins, float left, float right,
                                  float bottom, float top, int64_t n_rows, int32_t dim, float ldj_scale, void *stream) {
    return rqs_bwd_launch(false, x, gout, gldj, gldiag, params, params_stride, gx, gparams, live_idx, live_start, n_live, n_bins, left, right,
                          bottom, top, n_rows, dim, ldj_scale, stream);
}

// =====================================================================================================
// Backward of the monotone cubic spline in the INVERSE direction (training of spline_type='cubic' layers).
// The inverse pass solved f(t) = y for t in bin b, f(t) = a t^3 + b t^2 + c t + d (cubic_spline.py:134-137), and returned
// x = t + cw_b, ljd = -log f'(t).  The solve is differentiated IMPLICITLY:  dt = (dy - da t^3 - db t^2 - dc t - dd) / f'(t),
// so the Cardano / trigonometric / quadratic root formulas of the forward never appear here; the kernel is handed the
// forward's output.  (a, b, c, d) -> (w_b, s_b, the two Steffen knot derivatives, ch_b) -> widths / heights of bins
// b-1, b, b+1 and the cumsums -> softmax / sigmoid, in reverse mode.  min() / sign() pick the branch the forward took.
// Staging and layout as cubic_kernel (padded odd per-lane stride); gradients leave in the parameter tensor's layout.
// =====================================================================================================
// INVERSE = false: the FORWARD direction (x -> f(t), ljd = log f'(t), bin searched on the widths; `xout` unused): no solve, the
// adjoints of (a, b, c, d, t) are read off the polynomial, the chain below them is the same.
template <bool INVERSE>
__global__ __launch_bounds__(256) void cubic_bwd_kernel(const float *__restrict__ yin, const float *__restrict__ xout,
                                                                const float *__restrict__ gout, const float *__restrict__ gldj,
                                                                const float *__restrict__ gldiag,
                                                                const float *__restrict__ params, int64_t pstride,
                                                                float *__restrict__ gx, float *__restrict__ gparams,
                                                                const int32_t *__restrict__ live_idx, int l0, int n_live,
                                                                int K, float lower, float upper, int64_t n_rows, int dim,
                                                                float ldj_scale) {
    const int P = 2 * K + 2, PS = P | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    float *sp = rqs_smem + (size_t)wave * 64 * PS;
    const int64_t n_elem = n_rows * n_live;
    const int64_t n_groups = (n_elem + 63) >> 6;
    const float norm = 1.f - CUBIC_MIN_BIN * (float)K;
    const float span = upper - lower;
    const float inv_P = 1.0f / (float)P;
    for (int64_t grp = (int64_t)blockIdx.x * waves_per_block + wave; grp < n_groups;
         grp += (int64_t)gridDim.x * waves_per_block) {
        const int64_t e0 = grp << 6;
        const int n_here = (int)((n_elem - e0) < 64 ? (n_elem - e0) : 64);
        const int total = n_here * P;
        for (int idx = lane; idx < total; idx += 64) {
            const int el = (int)(((float)idx + 0.5f) * inv_P), q = idx - el * P;
            const int64_t e = e0 + el;
            const int64_t row = e / n_live;
            sp[el * PS + q] = params[row * pstride + (int64_t)(e - row * n_live) * P + q];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int64_t e = e0 + lane;
        const bool valid = e < n_elem;
        const int64_t row = valid ? e / n_live : 0;
        const int i = valid ? (int)(e - row * n_live) : 0;
        const int col = live_idx ? live_idx[i] : l0 + i;
        const float yv = valid ? yin[row * dim + col] : lower;
        const float xo = (INVERSE && valid) ? xout[row * dim + col] : lower;
        const float Ao = valid ? gout[row * dim + col] : 0.f;
        const float Al = valid ? ((gldj ? gldj[row] : 0.f) + (gldiag ? gldiag[row * dim + col] : 0.f)) * ldj_scale : 0.f;
        const bool inside = (yv >= lower) && (yv <= upper);
        const float yn = ((inside ? yv : lower) - lower) / span;
        float *p = sp + (valid ? lane : 0) * PS;

        // ---- forward pieces: softmax numerators in place, bin (by heights), neighbours ---------------------------
        float mw = p[0], mh = p[K];
        for (int k = 1; k < K; ++k) { mw = fmaxf(mw, p[k]); mh = fmaxf(mh, p[K + k]); }
        float sw = 0.f, sh = 0.f;
        for (int k = 0; k < K; ++k) {
            const float ew = comp_exp(p[k] - mw), eh = comp_exp(p[K + k] - mh);
            if (valid) { p[k] = ew; p[K + k] = eh; }
            sw += ew;
            sh += eh;
        }
        const float inv_sw = 1.f / sw, inv_sh = 1.f / sh;
        int b = 0;
        float cw = 0.f, ch = 0.f, cw_b = 0.f;
        for (int k = 0; k < K; ++k) {
            const float wk = CUBIC_MIN_BIN + norm * (p[k] * inv_sw), hk = CUBIC_MIN_BIN + norm * (p[K + k] * inv_sh);
            if (yn >= (INVERSE ? ch : cw)) { b = k; cw_b = cw; }
            cw += wk;
            ch += hk;
        }
        auto W = [&](int k) { return CUBIC_MIN_BIN + norm * (p[k] * inv_sw); };
        auto H = [&](int k) { return CUBIC_MIN_BIN + norm * (p[K + k] * inv_sh); };
        const float w_b = W(b), h_b = H(b), s_b = h_b / w_b;
        const bool has_m = b > 0, has_p = b < K - 1;
        const float w_m = has_m ? W(b - 1) : 1.f, h_m = has_m ? H(b - 1) : 1.f, s_m = h_m / w_m;
        const float w_p = has_p ? W(b + 1) : 1.f, h_p = has_p ? H(b + 1) : 1.f, s_p = h_p / w_p;
        const float sgl = sx_sigmoid(p[2 * K]), sgr = sx_sigmoid(p[2 * K + 1]);
        // knot derivatives and which branch produced them
        float dL, dR;
        bool L_m1 = false, L_first = false, R_m1 = false, R_first = false;
        if (!has_m) dL = sgl * 3.f * s_b;
        else {
            const float m1 = fminf(s_m, s_b), m2 = 0.5f * (w_b * s_m + w_m * s_b) / (w_m + w_b);
            L_m1 = m1 < m2; L_first = s_m < s_b;
            dL = fminf(m1, m2) * 2.f;
        }
        if (!has_p) dR = sgr * 3.f * s_b;
        else {
            const float m1 = fminf(s_b, s_p), m2 = 0.5f * (w_p * s_b + w_b * s_p) / (w_b + w_p);
            R_m1 = m1 < m2; R_first = s_b < s_p;
            dR = fminf(m1, m2) * 2.f;
        }
        const float a = (dL + dR - 2.f * s_b) / (w_b * w_b);
        const float bb = (3.f * s_b - 2.f * dL - dR) / w_b;
        const float c = dL;
        const float t = INVERSE ? (xo - lower) / span - cw_b : yn - cw_b;
        const float fp = 3.f * a * (t * t) + 2.f * bb * t + c, fpp = 6.f * a * t + 2.f * bb;

        // ---- reverse ----------------------------------------------------------------------------------------------
        const float Aon = Ao * span;                                   // out = out_n * span + lower
        const float ifp = 1.f / fp;
        float Ay, Aa, Ab, Ac, Achb, Acwb;
        if constexpr (INVERSE) {
            const float At = Aon - Al * fpp / fp;                      // out_n = t + cw_b,  ljd = -log f'(t) + const
            // the root as an implicit function of the bin's polynomial, dt/dtheta = -(df/dtheta) / f'(t) -- except where
            // |a| < 1e-3: there the reference solves the QUADRATIC bb t^2 + c t + (d - y) = 0 (cubic_spline.py:216-222), whose
            // root does not depend on a and whose other derivatives carry 1 / q'(t), q' = 2 bb t + c.  (da/dtheta carries
            // 1 / w^2, so the a-path is as large as the others; a near-identity spline has a ~ 0 in every bin.)
            const bool quad = fabsf(a) < CUBIC_QUAD_THRESHOLD;
            const float iq = quad ? 1.f / (2.f * bb * t + c) : ifp;
            Ay = At * iq / span;                                       // y_n = (y - lower) / span
            Aa = (quad ? 0.f : -At * (t * t * t) * iq) - Al * 3.f * (t * t) * ifp;
            Ab = -At * (t * t) * iq - Al * 2.f * t * ifp;
            Ac = -At * t * iq - Al * ifp;
            Achb = -At * iq;                                           // d = ch_b
            Acwb = Aon;
        } else {
            const float At = Aon * fp + Al * fpp * ifp;                // out_n = f(t),  ljd = log f'(t),  t = x_n - cw_b
            Ay = At / span;
            Aa = Aon * (t * t * t) + Al * 3.f * (t * t) * ifp;
            Ab = Aon * (t * t) + Al * 2.f * t * ifp;
            Ac = Aon * t + Al * ifp;
            Achb = Aon;                                                // d = ch_b
            Acwb = -At;
        }
        float AdL = Aa / (w_b * w_b) - 2.f * Ab / w_b + Ac;
        float AdR = Aa / (w_b * w_b) - Ab / w_b;
        float As = -2.f * Aa / (w_b * w_b) + 3.f * Ab / w_b;
        float Aw = -2.f * a * Aa / w_b - bb * Ab / w_b;
        float Ah = 0.f, Awm = 0.f, Ahm = 0.f, Awp = 0.f, Ahp = 0.f, Asm = 0.f, Asp = 0.f, Audl = 0.f, Audr = 0.f;
        if (!has_m) { Audl = AdL * 3.f * s_b * sgl * (1.f - sgl); As += AdL * 3.f * sgl; }
        else if (L_m1) { if (L_first) Asm += 2.f * AdL; else As += 2.f * AdL; }
        else {
            const float Wd = w_m + w_b, N = w_b * s_m + w_m * s_b, g = AdL;          // dL = N / Wd
            Aw += g * (s_m / Wd - N / (Wd * Wd));
            Awm += g * (s_b / Wd - N / (Wd * Wd));
            Asm += g * w_b / Wd;
            As += g * w_m / Wd;
        }
        if (!has_p) { Audr = AdR * 3.f * s_b * sgr * (1.f - sgr); As += AdR * 3.f * sgr; }
        else if (R_m1) { if (R_first) As += 2.f * AdR; else Asp += 2.f * AdR; }
        else {
            const float Wd = w_b + w_p, N = w_p * s_b + w_b * s_p, g = AdR;          // dR = N / Wd
            Awp += g * (s_b / Wd - N / (Wd * Wd));
            Aw += g * (s_p / Wd - N / (Wd * Wd));
            As += g * w_p / Wd;
            Asp += g * w_b / Wd;
        }
        Ah += As / w_b;  Aw += -As * s_b / w_b;
        Ahm += Asm / w_m; Awm += -Asm * s_m / w_m;
        Ahp += Asp / w_p; Awp += -Asp * s_p / w_p;
        // widths / heights: direct terms at b-1, b, b+1 + the cumsums' (cw_b, ch_b) on every bin below b
        auto Gw = [&](int k) { return (k < b ? Acwb : 0.f) + (k == b ? Aw : 0.f) + ((has_m && k == b - 1) ? Awm : 0.f) + ((has_p && k == b + 1) ? Awp : 0.f); };
        auto Gh = [&](int k) { return (k < b ? Achb : 0.f) + (k == b ? Ah : 0.f) + ((has_m && k == b - 1) ? Ahm : 0.f) + ((has_p && k == b + 1) ? Ahp : 0.f); };
        float dotw = 0.f, doth = 0.f;
        for (int k = 0; k < K; ++k) { dotw += p[k] * inv_sw * Gw(k); doth += p[K + k] * inv_sh * Gh(k); }
        const float gate = inside ? 1.f : 0.f;
        if (valid) {
            for (int k = 0; k < K; ++k) {
                const float pw = p[k] * inv_sw, ph = p[K + k] * inv_sh;
                p[k] = gate * norm * pw * (Gw(k) - dotw);
                p[K + k] = gate * norm * ph * (Gh(k) - doth);
            }
            p[2 * K] = gate * Audl;
            p[2 * K + 1] = gate * Audr;
            gx[row * dim + col] = inside ? Ay : Ao;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int idx = lane; idx < total; idx += 64) {
            const int el = (int)(((float)idx + 0.5f) * inv_P), q = idx - el * P;
            gparams[e0 * P + idx] = sp[el * PS + q];
        }
    }
}

static int cubic_bwd_launch(bool inverse, const float *yin, const float *xout, const float *gout, const float *gldj, const float *gldiag,
                                    const float *params, int64_t params_stride, float *gx, float *gparams,
                                    const int32_t *live_idx, int32_t live_start, int32_t n_live, int32_t n_bins, float lower,
                                    float upper, int64_t n_rows, int32_t dim, float ldj_scale, void *stream) {
    SX_REQUIRE(yin && (xout || !inverse) && gout && (gldj || gldiag) && params && gx && gparams, "sx_cubic_*_bwd: null pointer");
    SX_REQUIRE(dim > 0 && n_live > 0 && n_live <= dim && n_rows >= 0 && n_bins >= 1, "sx_cubic_inverse_bwd: bad sizes");
    SX_REQUIRE(upper > lower, "sx_cubic_inverse_bwd: empty domain");
    if (n_rows == 0) return SX_OK;
    const sx_slice_plan sl = sx_plan_slices((2 * n_bins + 2) | 1);
    SX_REQUIRE(sl.lds <= 160 * 1024, "sx_cubic_inverse_bwd: n_bins %d needs %zu B of LDS per wave", n_bins, sl.lds);
    if (sl.lds > 48 * 1024) {
        (void)hipFuncSetAttribute((const void *)cubic_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds);
        (void)hipFuncSetAttribute((const void *)cubic_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds);
    }
    const int grid = sl.grid((n_rows * n_live + 63) / 64);
    sx_dispatch(inverse, [&](auto INV) {
        hipLaunchKernelGGL(cubic_bwd_kernel<INV()>, dim3(grid), dim3(sl.block), sl.lds, sx_stream(stream), yin, xout, gout, gldj, gldiag,
                           params, params_stride, gx, gparams, live_idx, live_start, n_live, n_bins, lower, upper, n_rows, dim,
                           ldj_scale);
    });
    SX_LAUNCH_CHECK();
    return SX_OK;
}
extern "C" int sx_cubic_inverse_bwd(const float *yin, const float *xout, const float *gout, const float *gldj, const float *gldiag,
                                    const float *params, int64_t params_stride, float *gx, float *gparams,
                                    const int32_t *live_idx, int32_t live_start, int32_t n_live, int32_t n_bins, float lower,
                                    float upper, int64_t n_rows, int32_t dim, float ldj_scale, void *stream) {
    return cubic_bwd_launch(true, yin, xout, gout, gldj, gldiag, params, params_stride, gx, gparams, live_idx, live_start, n_live, n_bins,
                            lower, upper, n_rows, dim, ldj_scale, stream);
}
extern "C" int sx_cubic_forward_bwd(const float *x, const float *gout, const float *gldj, const float *gldiag, const float *params,
                                    int64_t params_stride, float *gx, float *gparams, const int32_t *live_idx,
                                    int32_t live_start, int32_t n_live, int32_t n_bins, float lower, float upper,
                                    int64_t n_rows, int32_t dim, float ldj_scale, void *stream) {
    return cubic_bwd_launch(false, x, nullptr, gout, gldj, gldiag, params, params_stride, gx, gparams, live_idx, live_start, n_live, n_bins,
                            lower, upper, n_rows, dim, ldj_scale, stream);
}
