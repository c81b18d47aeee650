// Rational-quadratic spline (stribor/util/rational_quadratic_spline.py:11-251): the constants and the per-element arithmetic shared by
// the element-wise kernels (sx_rqs.hip), their backward (sx_rqs_bwd.h), the slab tiers (sx_rqs_slab.hip) and the fused flow kernel's
// spline phases (sx_flow_spline.h) -- the counterpart of sx_cubic_core.h.  Which evaluation flavour uses what, and which copies stay
// because folding them moved device code: DESIGN 4.18.
#pragma once
#include "sx_common.h"

#define RQS_MIN_BIN 1e-3f                        // rational_quadratic_spline.py:7-8 (bin widths and heights)
#define RQS_MIN_DERIV 1e-3f                      // :9
#define RQS_EPS 1e-6f                            // search_sorted.py:4: the last knot carries + eps
#define RQS_BOUNDARY_DERIV 0.5397424172369522f   // log(exp(1 - RQS_MIN_DERIV) - 1), :81: the raw parameter whose knot derivative is 1

// a knot's derivative from its raw parameter (:107), softplus on v_exp_f32 / v_log_f32
__device__ __forceinline__ float rqs_knot_deriv(float r) { return RQS_MIN_DERIV + fast_softplus(r); }

// ---- the closing form: from the bin's geometry (its slope s_b = h_b / w_b included) and its two knot derivatives to the output and
// the numerator / denominator of its derivative, forward (:236-248) or inverse (:212-234), in the fast flavour: v_rcp_f32 /
// v_sqrt_f32, the discriminant clamped at 0 and the root to [0, 1].  The caller forms d_b, d_n and s_b, each at the point of its
// own instruction stream where it needs them, and takes the logs (rqs_log_deriv, or the slab's own tail).  (disc >= 0 in exact arithmetic -- the spline is monotone --; rounding can leave
// it a few ulps below zero where the root sits on a knot and the reference's own fp32 evaluation stays at or above it: clamp instead
// of returning NaN, :223.  The root is a position inside the bin: rounding can also leave it an ulp outside [0, 1], where a steep bin
// next to a flat one -- slope ~1e3, knot derivative ~1e-3 -- turns the derivative's numerator negative and its log into NaN.)
// `hk.at<Y>(values...)` is called at the named points below with the values produced since the previous one; a kernel that runs the
// evaluation beside MFMAs ties them down and issues its matrix work from there.  A hook answers the points it wants and ignores the rest.
enum rqs_yield {
    RQS_Y_Q, RQS_Y_DISC, RQS_Y_ROOT,    // inverse: d_b + d_n - 2 s, the discriminant, the clamped root
    RQS_Y_THETA, RQS_Y_NUM,             // forward: the position inside the bin, the numerator
    RQS_Y_DEN, RQS_Y_OUT, RQS_Y_DNUM    // denominator, output (forward: with the denominator again), the derivative's numerator
};
struct rqs_no_hook {
    template <int Y, class... T> __device__ __forceinline__ void at(T &...) {}
};
struct rqs_closed { float out, den, dnum; };
template <bool REV, class Hook>
__device__ __forceinline__ rqs_closed rqs_close(float d_b, float d_n, float s_b, float cw_b, float w_b, float ch_b, float h_b, float xin, Hook &hk) {
    if constexpr (REV) {
        const float dy = xin - ch_b;
        float q = d_b + d_n - 2.f * s_b;
        hk.template at<RQS_Y_Q>(q);
        const float a = dy * q + h_b * (s_b - d_b);
        const float bb = h_b * d_b - dy * q;
        const float c = -s_b * dy;
        float disc = bb * bb - 4.f * a * c;
        hk.template at<RQS_Y_DISC>(disc);
        float root = __builtin_amdgcn_fmed3f((2.f * c) * fast_rcp(-bb - __builtin_amdgcn_sqrtf(__builtin_fmaxf(disc, 0.f))), 0.f, 1.f);
        hk.template at<RQS_Y_ROOT>(root);
        float out = root * w_b + cw_b;
        hk.template at<RQS_Y_OUT>(out);
        const float tomt = root * (1.f - root), omr = 1.f - root;
        float den = s_b + q * tomt;
        hk.template at<RQS_Y_DEN>(den);
        float dnum = (s_b * s_b) * (d_n * (root * root) + 2.f * s_b * tomt + d_b * (omr * omr));
        hk.template at<RQS_Y_DNUM>(dnum);
        return {out, den, dnum};
    } else {
        float theta = (xin - cw_b) * fast_rcp(w_b);
        hk.template at<RQS_Y_THETA>(theta);
        const float tomt = theta * (1.f - theta), omt = 1.f - theta;
        float num = h_b * (s_b * (theta * theta) + d_b * tomt);
        hk.template at<RQS_Y_NUM>(num);
        float den = s_b + (d_b + d_n - 2.f * s_b) * tomt;
        hk.template at<RQS_Y_DEN>(den);
        float out = ch_b + num * fast_rcp(den);
        hk.template at<RQS_Y_OUT>(out, den);
        float dnum = (s_b * s_b) * (d_n * (theta * theta) + 2.f * s_b * tomt + d_b * (omt * omt));
        hk.template at<RQS_Y_DNUM>(dnum);
        return {out, den, dnum};
    }
}
// log|d out / d in| from the two: two logs, each scaled by ln 2 (REV: already negated like the reference's, :234)
template <bool REV>
__device__ __forceinline__ float rqs_log_deriv(float dnum, float den) {
    return REV ? -fast_log(dnum) + 2.f * fast_log(den) : fast_log(dnum) - 2.f * fast_log(den);
}
