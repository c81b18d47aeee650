// Per-element arithmetic of the time-dependent point-wise flows (ContinuousTanh / ContinuousActivation, stribor/flows/activations.py:125-196),
// shared by the stand-alone sx_pointwise_time kernels and the SX_STEP_POINTWISE_TIME step of the fused flow kernel.
//
// The tanh-flow y = asinh(e^tau sinh x) is stated in the log domain: the literal sequence overflows in fp32 once |x| + tau passes ~89 and
// its log-derivative once it passes ~44.  With a = |x|, q = exp(-2a) and s = tau + a + log(1 - q) = log(2u) for u = e^tau sinh a:
//   s >= 0:  asinh(u) = s + log1p((sqrt(1 + 4 e^-2s) - 1) / 2),        log dy/dx = log1p(q) - log(1 - q) - 1/2 log1p(4 e^-2s)
//   s <  0:  asinh(u) = log1p(u + u^2 / (1 + sqrt(1 + u^2))), u = e^s / 2,  log dy/dx = tau + a + log1p(q) - log 2 - 1/2 log1p(u^2)
// 1 - q comes from expm1 (no cancellation near x = 0).  Both branches also give tanh|y| = u / sqrt(1 + u^2) and 1 - tanh^2 y, which
// the backward needs (dy/dtau = tanh y, d(log dy/dx)/dtau = 1 - tanh^2 y, d(log dy/dx)/dx = tanh x - tanh y dy/dx).
#pragma once
#include "sx_common.h"

#define PWT_LOG2 0.69314718055994531f

__device__ __forceinline__ bool pwt_is_flow(int kind) { return kind == SX_PWT_TANH_FLOW || kind == SX_PWT_TANH_FLOW_INV; }

// what a row's time becomes before the elements see it: tau (signed by the direction; log1p(t) with log_time) for the tanh-flow kinds,
// w = tanh(temperature t) for the mix kinds
__device__ __forceinline__ float pwt_row(int kind, float param, float t) {
    if (pwt_is_flow(kind)) {
        const float tau = param != 0.f ? log1pf(t) : t;
        return kind == SX_PWT_TANH_FLOW_INV ? -tau : tau;
    }
    return tanhf(param * t);
}

struct pwt_flow_out {
    float y, ld;            // value, log dy/dx
    float tanh_x, tanh_y;   // signed
    float sech2_y;          // 1 - tanh^2 y
};
__device__ __forceinline__ pwt_flow_out pwt_tanh_flow(float tau, float x) {
    pwt_flow_out o;
    const float a = fabsf(x);
    const float em = expm1f(-2.f * a);          // -(1 - q)
    const float q = 1.f + em;
    const float l1 = logf(-em);                 // log(1 - q); -inf at x = 0
    const float lq = log1pf(q);
    const float s = (tau + a) + l1;
    float ya, ty;
    if (s >= 0.f) {
        const float w = 4.f * expf(-2.f * s);   // 1 / u^2
        const float r = sqrtf(1.f + w);
        ya = s + log1pf(w / (2.f * (r + 1.f)));
        o.ld = (lq - l1) - 0.5f * log1pf(w);
        ty = 1.f / r;
        o.sech2_y = w / (1.f + w);
    } else {
        const float u = 0.5f * expf(s);
        const float u2 = u * u;
        const float r = sqrtf(1.f + u2);
        ya = log1pf(u + u2 / (1.f + r));
        o.ld = ((tau + a) + (lq - PWT_LOG2)) - 0.5f * log1pf(u2);
        ty = u / r;
        o.sech2_y = 1.f / (1.f + u2);
    }
    o.y = copysignf(ya, x);
    if (tau == 0.f) { o.y = x; o.ld = 0.f; }    // the flow's defining property, exactly: the identity at t = 0 (asinh(sinh x) rounds)
    o.tanh_y = copysignf(ty, x);
    o.tanh_x = copysignf(-em / (1.f + q), x);
    return o;
}

// act(x) of a mix kind (activations.py:149-150: x (1 - w) + act(x) w) and its derivative
__device__ __forceinline__ float pwt_act(int kind, float x, float &dact) {
    if (kind == SX_PWT_MIX_TANH) {
        const float th = tanhf(x);
        dact = 1.f - th * th;
        return th;
    }
    if (kind == SX_PWT_MIX_SIGMOID) {
        const float sg = sx_sigmoid(x);
        dact = sg * (1.f - sg);
        return sg;
    }
    dact = x > 0.f ? 1.f : 0.f;
    return x < 0.f ? 0.f : x;                   // relu; NaN stays NaN
}
__device__ __forceinline__ float pwt_mix(int kind, float w, float x) {
    float d;
    const float av = pwt_act(kind, x, d);
    return x * (1.f - w) + av * w;
}
