// Monotone cubic spline (stribor/util/cubic_spline.py:21-251): the per-element arithmetic shared by the element-wise kernel
// (sx_rqs.hip: cubic_kernel), the slab tiers (sx_rqs_slab.hip, sx_rqs_bwd.h) and the fused flow kernel's cubic phases (sx_flow_kernel.h).
#pragma once
#include "sx_common.h"
#define CUBIC_MIN_BIN 1e-2f          // cubic_spline.py:13-14
#define CUBIC_EPS 1e-5f              // :15
#define CUBIC_QUAD_THRESHOLD 1e-3f   // :16

// ---- cubic_kernel's arithmetic: the hardware's 1-ulp exp2 / log2 / rcp / sqrt instead of libm calls and IEEE division
// sequences (the kernel is VALU-bound: 1,489 -> ~900 VALU instructions per element in the inverse direction, 791 -> ~500
// forward, tools/pmc_spline_kernels.sh).  Their errors (~1e-7 relative) are the size of the reference's own fp32 rounding;
// the inverse ends in Newton steps on the bin's cubic, so its result does not depend on how exactly the closed form ran.
__device__ __forceinline__ float cubic_fcbrt(float v) {        // :18-20  sign(x) * exp(log|x| / 3)
    const float m = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(fabsf(v)) * (1.0f / 3.0f));
    return (v == 0.f) ? 0.f : copysignf(m, v);
}
// Knot derivatives of bin b (:117-132) and its cubic a t^3 + bb t^2 + c t + d (:134-137) from the sizes of bins b-1, b, b+1.
// Bin sizes are >= 1e-2, so every slope is positive: sign(s_m) + sign(s_b) = 2 and the |.| of :118-119 are no-ops.
struct cubic_coef { float a, bb, c; };
__device__ __forceinline__ cubic_coef cubic_bin_coef(int b, int K, float w_b, float h_b, float w_m, float h_m, float w_p, float h_p,
                                                     float dpar0, float dpar1) {
    const float rwb = fast_rcp(w_b);
    const float s_b = h_b * rwb;                                                           // :117
    const float s_m = h_m * fast_rcp(w_m), s_p = h_p * fast_rcp(w_p);
    const float mL = 0.5f * (w_b * s_m + w_m * s_b) * fast_rcp(w_m + w_b);              // :120-123
    const float mR = 0.5f * (w_p * s_b + w_b * s_p) * fast_rcp(w_b + w_p);
    const float dL = (b == 0) ? fast_sigmoid(dpar0) * 3.f * s_b : 2.f * fminf(fminf(s_m, s_b), mL);       // :126, :118-129
    const float dR = (b == K - 1) ? fast_sigmoid(dpar1) * 3.f * s_b : 2.f * fminf(fminf(s_b, s_p), mR);   // :127
    cubic_coef q;
    q.a = (dL + dR - 2.f * s_b) * (rwb * rwb);                                             // :134
    q.bb = (3.f * s_b - 2.f * dL - dR) * rwb;                                              // :135
    q.c = dL;                                                                              // :136
    return q;
}
// log f'(x) in bin b from the sizes of bins b-1, b, b+1 (:117-137, :235-237)
__device__ __forceinline__ float cubic_logderiv_at(int b, int K, float cw_b, float w_b, float h_b, float w_m, float h_m, float w_p,
                                                   float h_p, float dpar0, float dpar1, float xin) {
    const cubic_coef q = cubic_bin_coef(b, K, w_b, h_b, w_m, h_m, w_p, h_p, dpar0, dpar1);
    const float t = xin - cw_b;
    return fast_log(3.f * q.a * (t * t) + 2.f * q.bb * t + q.c);
}
// The forward log-derivative at normalised input `xin` from an element's exp'ed widths / heights in registers (ew(k), eh(k): how
// entry k is read) and their softmax factors nw, nh: one unrolled sweep over sixteen entries, selects only; the bin is searched by
// widths, as the forward pass does.  BOUNDED: K <= 16 entries count (k < K is tested); otherwise all sixteen do.  (The inverse
// kernels' reference mode, where the inverted point does not land in the bin it was solved in.)
template <bool BOUNDED, class GW, class GH>
__device__ __forceinline__ float cubic_select_forward_logderiv(GW ew, GH eh, float nw, float nh, float dpar0, float dpar1, int K, float xin) {
    int b = 0;
    float cw_b = 0.f, w_b = 0.f, h_b = 0.f, w_m = 1.f, h_m = 1.f, w_p = 1.f, h_p = 1.f;
    float cw = 0.f, w_last = 1.f, h_last = 1.f;
    bool need_next = false;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool used = BOUNDED ? k < K : true;
        const float wk = CUBIC_MIN_BIN + nw * ew(k);
        const float hk = CUBIC_MIN_BIN + nh * eh(k);
        const bool ge = used && xin >= cw;
        const bool nx = used && !ge && need_next;
        b = ge ? k : b; cw_b = ge ? cw : cw_b; w_b = ge ? wk : w_b; h_b = ge ? hk : h_b;
        w_m = ge ? w_last : w_m; h_m = ge ? h_last : h_m;
        w_p = nx ? wk : w_p; h_p = nx ? hk : h_p;
        need_next = used ? ge : need_next;
        w_last = wk; h_last = hk;
        cw += wk;
    }
    return cubic_logderiv_at(b, K, cw_b, w_b, h_b, w_m, h_m, w_p, h_p, dpar0, dpar1, xin);
}
// The inverse of the bin's cubic f(t) = a t^3 + bb t^2 + c t + d at y = xin (:154-222): the reference's closed forms (one-root
// Cardano form, three-root trigonometric form with the in-bin root picked in its order, quadratic formula where |a| < 1e-3),
// then Newton steps inside the bin.  Returns t = root - cw_b in [0, rcw - cw_b].
__device__ __forceinline__ float cubic_invert(float a, float bb, float c, float d, float xin, float cw_b, float rcw) {
            float o;
            const float ra = fast_rcp(a);
            const float b_ = (bb * ra) * (1.0f / 3.0f);                                    // :154-156
            const float c_ = (c * ra) * (1.0f / 3.0f);
            const float d_ = (d - xin) * ra;
            const float delta_1 = -(b_ * b_) + c_;                                         // :158-160
            const float delta_2 = -c_ * b_ + d_;
            const float delta_3 = b_ * d_ - c_ * c_;
            const float disc = 4.f * delta_1 * delta_3 - delta_2 * delta_2;                // :162
            const float dep1 = -2.f * b_ * delta_1 + delta_2;                              // :164
            const bool three = disc > 0.f;                                                 // :167
            const float sqd = __builtin_amdgcn_sqrtf(fabsf(disc));
            // one root (:174-179)
            const float sq = three ? 0.f : sqd;
            const float one_root = (cubic_fcbrt((-dep1 + sq) * 0.5f) + cubic_fcbrt((-dep1 - sq) * 0.5f)) - b_ + cw_b;
            // three roots (:183-212): the first (order 1, 2, 3) that lies in the bin, root 1 if none does.
            // theta = atan2(sqrt(disc), -dep1) / 3 in [0, pi/3]: odd polynomial for atan on [0, 1] (1.3e-7), Taylor sums for
            // cos / sin on [0, pi/3] (< 4e-9) -- no range reduction is needed anywhere.
            const float ty = three ? sqd : 0.f, tx = -dep1;
            const float ax = fabsf(tx), hi_ = fmaxf(ax, ty), lo_ = fminf(ax, ty);
            const float qa = (hi_ > 0.f) ? lo_ * fast_rcp(hi_) : 0.f, q2 = qa * qa;
            float at = -0.00405455706641078f;
            at = fmaf(at, q2, 0.021862920373678207f); at = fmaf(at, q2, -0.05591226741671562f); at = fmaf(at, q2, 0.09642192721366882f);
            at = fmaf(at, q2, -0.1390862762928009f); at = fmaf(at, q2, 0.19946564733982086f); at = fmaf(at, q2, -0.33329859375953674f);
            at = fmaf(at, q2, 0.9999993443489075f);
            at = at * qa;
            at = (ty > ax) ? 1.5707963267948966f - at : at;
            at = (tx < 0.f) ? 3.141592653589793f - at : at;
            const float theta = at * (1.0f / 3.0f), th2 = theta * theta;
            float cr1 = -2.755731922398589e-07f;                                           // cos: 1 - t^2/2! + ... - t^10/10!
            cr1 = fmaf(cr1, th2, 2.48015873015873e-05f); cr1 = fmaf(cr1, th2, -1.388888888888889e-03f); cr1 = fmaf(cr1, th2, 4.166666666666666e-02f);
            cr1 = fmaf(cr1, th2, -0.5f); cr1 = fmaf(cr1, th2, 1.f);
            float cr2 = -2.505210838544172e-08f;                                           // sin: t (1 - t^2/3! + ... - t^10/11!)
            cr2 = fmaf(cr2, th2, 2.755731922398589e-06f); cr2 = fmaf(cr2, th2, -1.984126984126984e-04f); cr2 = fmaf(cr2, th2, 8.333333333333333e-03f);
            cr2 = fmaf(cr2, th2, -1.666666666666667e-01f); cr2 = fmaf(cr2, th2, 1.f);
            cr2 = cr2 * theta;
            const float scale = 2.f * __builtin_amdgcn_sqrtf(three ? -delta_1 : 0.f), shift = -b_ + cw_b;
            const float r1 = cr1 * scale + shift;
            const float r2 = (-0.5f * cr1 - 0.5f * 1.7320508075688772f * cr2) * scale + shift;
            const float r3 = (-0.5f * cr1 + 0.5f * 1.7320508075688772f * cr2) * scale + shift;
            const float lo3 = cw_b - CUBIC_EPS, hi3 = rcw + CUBIC_EPS;
            const bool k1 = (lo3 < r1) && (r1 < hi3), k2 = (lo3 < r2) && (r2 < hi3), k3 = (lo3 < r3) && (r3 < hi3);
            const float pick = k1 ? r1 : (k2 ? r2 : (k3 ? r3 : r1));
            o = three ? pick : one_root;
            // a -> 0 (:216-222)
            if (fabsf(a) < CUBIC_QUAD_THRESHOLD) {
                // (-c + sqrt(c^2 - 4 bb qc)) / (2 bb) in its cancellation-free form -2 qc / (c + sqrt(.)), c = dL > 0: the same
                // root, but the reference's form loses everything as bb -> 0 (a near-identity spline has bb ~ 1e-5: 5 % of t,
                // 1e-2 of x in fp32 -- the reference's own fp32 path does that; its fp64 values are what this returns)
                const float qc = d - xin;
                o = (-2.f * qc) * fast_rcp(c + __builtin_amdgcn_sqrtf(c * c - 4.f * bb * qc)) + cw_b;
            }
            // Newton steps on f(t) = a t^3 + bb t^2 + c t + d - y inside the bin (f is monotone there): the closed forms above lose
            // up to 5e-3 of the bin in fp32 where the cubic degenerates (the reference's fp32 path does too); two steps from
            // their result bring the residual to rounding level.  A non-finite start falls back to the bin's lower knot.
            float so = o - cw_b;                                                           // :224
            const float t_hi = rcw - cw_b, f0 = d - xin;
            so = fminf(fmaxf(so, 0.f), t_hi);                                              // (fmaxf(NaN, 0) = 0)
            const bool quad = fabsf(a) < CUBIC_QUAD_THRESHOLD;     // the reference's quadratic root stays as it is (it is not the cubic's)
            const float so_q = o - cw_b;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const float fv = fmaf(fmaf(fmaf(a, so, bb), so, c), so, f0);
                const float fd = fmaf(fmaf(3.f * a, so, 2.f * bb), so, c);
                const float st = fv * fast_rcp(fd);
                so = (fd > 0.f) ? fminf(fmaxf(so - st, 0.f), t_hi) : so;
            }
            so = quad ? so_q : so;
            return so;
}
