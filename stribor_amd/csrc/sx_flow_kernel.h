// Fused flow kernel: a whole NormalizingFlow (or one Coupling, or one conditioner MLP) in ONE launch.
//
// Replaces the Python loop of stribor/flow.py:99-130 and, per coupling layer, the torch-op chain
//   mask -> x*mask -> Linear -> Tanh -> Linear -> chunk -> (x-shift)*exp(-log_scale) -> blend -> sum
// of stribor/flows/coupling.py:48-95 + flows/affine.py:59-123 + net/mlp.py:65.
//
// Mapping to CDNA4 (MI355X_MICROARCH.md, cdna_hip_programming.md §3; measurements in DESIGN.md §4.1/§6):
//   * one wave = 32 samples.  Samples sit on the MFMA column (lane&31), features on the C rows, so the flow
//     state x[D] of a sample is 16*D/32 VGPRs per lane in MFMA C-fragment order (lane half h = lane>>5 owns
//     features kmap(r,h), r = 0..15, of every 32-wide tile);
//   * a C tile is directly the B operand of the next GEMM (k-step <-> feature kmap; the weights are
//     pre-permuted by sx_pack_linear), so x -> hidden -> (log_scale, shift) -> x' never leaves registers:
//     no LDS transposes, no HBM round trips between layers;
//   * GEMM arithmetic is a build-time choice.  Default (-DSX_F16X3): both operands split hi + lo in fp16, three
//     products per 16-deep step on v_mfma_f32_32x32x16_f16 with fp32 accumulation (~2^-22 per product,
//     fp32-grade) -- on the matrix pipe, BESIDE the VALU.  EXACT_F32=1: v_mfma_f32_32x32x2_f32, an exact fp32
//     fma chain, which on gfx950 executes at the VALU rate ON the VALU (tools/mfma_probe.hip), so the tanh /
//     exp work serialises behind it;
//   * the kernel is VALU-issue bound, so VALU work is shaved: tanh's and exp's constants live in the packed
//     weights (hidden r = 1/(exp2(z') + 1): v_exp, v_add, v_rcp), activations of one tile are issued between the
//     MFMAs of the next, every LDS access is pointer + immediate, one runtime dispatch per step selects a
//     straight-line specialisation;
//   * weights of one step (<= ~33 KB) stream L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds), double-buffered:
//     step s+1 lands while step s computes; the NEXT step's descriptor is fetched one step early as well;
//   * 256-thread workgroups (4 waves = 128 samples per pass), persistent grid-stride over sample chunks,
//     2 workgroups per CU for D <= 64, 1 for D = 128;
//   * per-sample log-det / log-prob: in-lane sums + ONE cross-half shuffle; optional batch sum as fp64
//     block partials + one atomic per workgroup (flow.py:129 + the multi-GPU all-reduce operand).
#pragma once
#include "sx_common.h"
#include "sx_flow_types.h"
#include "sx_cubic_core.h"
#include "sx_rqs_core.h"
#include "sx_pointwise_core.h"
#include "sx_pointwise_time_core.h"
#include <stdlib.h>
#include <type_traits>

#define SX_HALF_LOG_2PI 0.91893853320467274178f

// Both GEMM arithmetics live in one library: this header is compiled twice per (tiles, hidden-tiles) pair, with and
// without -DSX_F16X3, into its own namespace; sx_flow_run picks the variant per call (`precision`).
#ifdef SX_F16X3
#define SX_PREC_NS sx_f16x3
#else
#define SX_PREC_NS sx_f32x
#endif
namespace SX_PREC_NS {

extern __shared__ __attribute__((aligned(16))) float smem[];

typedef __attribute__((address_space(3))) void lds_void;

template <int NS>
struct tile {            // one 32-feature tile of NS x 32 samples, C-fragment order
    f32x16 v[NS];
};

// fp16 x 3 operand range.  hi + lo holds a value only while |v| <= 65504 (fp16's largest finite number); beyond it the
// split saturates.  Every UNBOUNDED B operand a lane forms (flow state, gradients, activations other than the
// tanh / sigmoid family) passes through the tracked make_btile below, which keeps the running max |v| in one register
// (one v_max3_f32 per register pair); the chunk epilogue turns an overflow into NaN outputs for that sample and raises
// SX_FLAG_F16_RANGE in the caller's flag word, so an out-of-range input can never come back as a plausible number.
// (NaN inputs are not counted -- they propagate through the MFMAs by themselves.)  The exact-fp32 variant has no range
// limit and carries no tracker.
#define SX_F16_MAX 65504.0f
// With a redo list (sx_flow_run2) a sample is NAMED -- and evaluated by the exact-fp32 kernel -- as soon as one of its tracked operands
// exceeds SX_REDO_ABOVE, well inside fp16's range.  A weight below 0.125 is held as hi + lo only to an ABSOLUTE 2^-25 (fp16's subnormal
// quantum bounds its low half): an error of 3e-8 |x| sqrt(K) in the pre-activation, about 0.5 / |w| (~ 7 for nn.Linear's default
// initialisation) times the fp32 sequence's own rounding whatever |x| is -- invisible against O(1) pre-activations at |x| ~ 1, but it
// grows with |x| while the sensitive range of tanh does not: a row of |x| = 6.4e4, inside fp16's range, came out at 1.4e-4 relative, 27 x
// the fp32 sequence's error (tools/fuzz_dense.py 120 914 --big, case 85).  The term is linear in |x|: 4.5e-6 at 2048, below the 1e-5 of
// BASELINE's north_star with a factor of two to spare.  (256 was tried first: the states of the randomly initialised cfg-4 flow pass it
// on ~ 7 % of the rows -- +0.23 ms of exact pass per 2^20 rows; at 2048 the BASELINE flows name nothing.)
// Ordinary (normalised) data never reaches it; data that does is evaluated exactly, at the exact kernel's speed.
// Without a list (graph-building calls, plain sx_flow_run) the limit stays fp16's own: beyond it NaN + SX_FLAG_F16_RANGE.
#define SX_REDO_ABOVE 2048.0f
struct rng_t {
    uint64_t bad;          // lanes that formed an out-of-range operand: wave-uniform, lives in SGPRs (the pure coupling kernel
                           // sits exactly on its 128-VGPR budget: a per-lane running max spilled)
    float thr = SX_F16_MAX;    // wave-uniform (an SGPR): SX_REDO_ABOVE in launches that carry a redo list
};
__device__ __forceinline__ float rng_max(float m, float a, float b) {
    // ONE v_max3_f32 m, |a|, |b|.  Written as fmaxf(m, fmaxf(fabsf(a), fabsf(b))) the compiler canonicalises each operand first
    // (v_max_f32 |a|, |a| ...): four vector instructions per register pair, a seventh of cfg 4's vector work (round-5 ISA reading).
    float r;
    asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void rng_note(rng_t &rg, float m) {
#ifdef SX_F16X3
    rg.bad |= __builtin_amdgcn_ballot_w64(m > rg.thr);              // v_cmp + s_or_b64
#endif
}
// the redo pass closes an overwriting call (flow_kargs::sum_slot): the total leaves the slot for the caller's word, 0 stays behind
__device__ __forceinline__ void redo_close_sum(double *slot, double *sum_out) {
    *sum_out = __longlong_as_double((long long)atomicExch(reinterpret_cast<unsigned long long *>(slot), 0ull));
}

// one (32-row group, bad-sample mask) pair per sample tile of the wave onto the redo list (flow_kargs::redo)
template <int NS>
__device__ __forceinline__ void redo_push(uint32_t *redo, const rng_t &rg, int lane, uint32_t group0) {
    if (lane == 0) {
        const uint32_t msk = (uint32_t)(rg.bad | (rg.bad >> 32));
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const uint32_t i = atomicAdd(redo, 1u);
            redo[2 + 2 * i] = group0 + (uint32_t)n;
            redo[3 + 2 * i] = msk;
        }
    }
}
// Round 6 (VERDICT r5 missing #1 / next #4a): what happens to a sample whose operand left fp16's range.
// Round 5 rescaled it by a power of two inside the kernel (rng_pow2_of): finite, but not fp32-grade -- a weight is hi + lo in fp16
// and fp16's subnormal quantum bounds the low half: |w| >= 0.125 carries 22 bits, a conditioner weight of 0.01 .. 0.1 only 18 .. 21 (an
// ABSOLUTE 3e-8), which against state entries of 1e5 is 20 .. 170 x the fp32 sequence's error on rows whose huge terms cancel inside
// a hidden unit.  Those bits were dropped at pack time; no rescaling of the operands brings them back.  Now the sample is
// NAMED (its lanes' bits in rg.bad) and the chunk epilogue puts its 32-row group and the per-sample mask on the launch's redo list
// (flow_kargs::redo, sx_flow_run2): a second launch of the same program on the exact-fp32 kernel evaluates exactly those samples.
// Without a list the sample comes back as NaN + SX_FLAG_F16_RANGE (never a plausible number), as before round 5.
// (Built first as an in-kernel rescue on an fp32 twin of the weights -- global loads + v_mfma_f32_32x32x2_f32 in the rare branch:
//  parity-green, but the branch's registers cost cfg 2 +3 .. 5 % and cfg 4 +3 %: inlined, spills inside <1,4,2,7>'s MFMA loops; out
//  of line, the call's ABI took ten spline kernels from two waves per SIMD to one.  The hot kernels carry no rescue code at all now:
//  the rescale paths are gone too.)
__device__ __forceinline__ bool rng_bad_sample(const rng_t &rg, int lane) {
    // the two lane halves hold one sample
    return ((rg.bad >> (lane & 31)) | (rg.bad >> ((lane & 31) + 32))) & 1ull;
}

// ---- weights: L2 -> LDS by LDS-DMA, 1 KiB per wave-instruction, lane-linear -----------------------------
template <int WAVES>
__device__ __forceinline__ void stage_blob(const float *__restrict__ g, int lds_float_off, uint32_t n_floats) {
    // wave-uniform loop: scalar piece offsets (the LDS address goes through m0), one VGPR of lane offsets
    // The MUBUF form (buffer_load_dwordx4 ... lds), not global_load_lds: the compiler's wait-count pass books a FLAT-encoded
    // LDS-DMA as "may touch both memories" and, while one is in flight, turns EVERY later wait into a full one -- each
    // s_waitcnt lgkmcnt(N) in front of an MFMA became lgkmcnt(0), so a wave could never keep the next tile's ds_reads in flight
    // across the current tile's MFMAs (found on cfg 4: 64 exposed LDS round trips per dense layer).
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t n_bytes = n_floats * 4u;    // multiple of 1024 (host pads blobs to 256 floats)
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g), 0, n_bytes, 0x00020000);
    char *ldst = reinterpret_cast<char *>(smem + lds_float_off);
    for (uint32_t off = wave * 1024u; off < n_bytes; off += WAVES * 1024u) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void *)(ldst + off), 16, lane * 16, off, 0, 0);
    }
}

// ---- one 32x32 output tile (x NS sample tiles) += A(32 x 32) . B, A from LDS --------------------------
// f(i), i = 0..15, is one unit of independent VALU work slotted between the MFMAs.
#ifndef SX_F16X3
// exact fp32: 16 k-steps of v_mfma_f32_32x32x2_f32; the B operand is the fp32 C tile itself
template <int NS>
using btile = tile<NS>;
template <int NS>
__device__ __forceinline__ const btile<NS> &make_btile(const tile<NS> &c) { return c; }
template <int NS>
__device__ __forceinline__ const btile<NS> &make_btile(const tile<NS> &c, rng_t &) { return c; }
template <int NS>
__device__ __forceinline__ const btile<NS> &make_btile_mx(const tile<NS> &c, float &) { return c; }      // (no operand range in this arithmetic)
__device__ __forceinline__ bool rng_over(float) { return false; }

template <int NS, class F>
__device__ __forceinline__ void gemm_tile_f(const char *wb, int a_off, const btile<NS> &b, tile<NS> &acc, F &&f) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(wb + (a_off + g * 256) * 4);   // ds_read_b128, imm offset
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.v[n][4 * g + 0], acc.v[n], 0, 0, 0);
        f(4 * g + 0);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.v[n][4 * g + 1], acc.v[n], 0, 0, 0);
        f(4 * g + 1);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.v[n][4 * g + 2], acc.v[n], 0, 0, 0);
        f(4 * g + 2);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.v[n][4 * g + 3], acc.v[n], 0, 0, 0);
        f(4 * g + 3);
    }
}
#else
// fp16 x 3 split: a = a_hi + a_lo, b = b_hi + b_lo in fp16 (22 mantissa bits each), a.b ~= a_hi b_hi + a_hi b_lo +
// a_lo b_hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation: 6 MFMAs x 32 cycles per 32-deep tile instead of
// 16 x 64 cycles, and -- unlike the fp32 form, which executes on the VALU -- on the matrix pipe, beside the VALU.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <int NS>
struct btile {            // one 32-deep B operand: 2 k16-steps x (hi, lo) fragments, per sample tile
    h8 hi[NS][2], lo[NS][2];
};
// Two fp32 -> one register of two fp16, round to NEAREST even: gfx950's v_cvt_pk_f16_f32.  (Rounds 1-4 used v_cvt_pkrtz_f16_f32, the
// only packed conversion of gfx942: truncation leaves |v - hi - lo| up to 2^-20 |v|, always towards zero -- a BIAS that adds up
// over a sum; nearest leaves 2^-22 |v| without a sign preference.  Same instruction count, same time on cfg 2 / 3 / 4
// (tools/experiments/cfg4_ab.sh, three interleaved rounds); against the fp64 oracle on 8,192 rows
// (tools/experiments/split_accuracy.py): cfg 2 log_prob rms 1.9e-7 -> 1.2e-7, mean signed error +1.1e-7 -> +1.7e-8 (the reference's own
// fp32 sequence: 8.6e-8, +6.8e-9); cfg 4 rms 1.8e-6 -> 8.3e-7, mean +1.6e-6 -> +6e-8 (fp32 sequence: 1.2e-6).)
__device__ __forceinline__ uint32_t pk_f16(float a, float b) {
    typedef float f32x2v __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2v){a, b}, f16x2v));
}
// lo halfs of a pair: f16(v - hi) straight from the packed hi register: v_fma_mix_f32 reads the fp16 source in
// place (no v_cvt_f32_f16) and subtracts in fp32 (exact): 4 full-rate VALU instructions per pair for the whole
// split instead of 6.  (v_fma_mixlo/mixhi_f16 would make it 3, but they issue at the transcendental rate:
// tools/valu_cost_probe.hip.)
__device__ __forceinline__ uint32_t pk_residual(uint32_t ph, float v0, float v1) {
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(ph), "v"(v0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(ph), "v"(v1));
    return pk_f16(l0, l1);
}
// C tile (fp32, 16 registers) -> B fragments: k16-step s takes registers 8s..8s+7 (cdna_hip_programming.md §3
// 'An accumulator tile as the next MFMA's operand'); hi = f16(v), lo = f16(v - hi) (v - hi is exact in fp32), both to nearest.
template <int NS, bool TRACK>
__device__ __forceinline__ btile<NS> make_btile_impl(const tile<NS> &c, rng_t *rg) {
    btile<NS> b;
    [[maybe_unused]] float mx = 0.f;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 hi, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v0 = c.v[n][8 * s + 2 * q], v1 = c.v[n][8 * s + 2 * q + 1];
                if constexpr (TRACK) mx = rng_max(mx, v0, v1);
                const uint32_t ph = pk_f16(v0, v1);
                hi[q] = ph;
                lo[q] = pk_residual(ph, v0, v1);
            }
            b.hi[n][s] = __builtin_bit_cast(h8, hi);
            b.lo[n][s] = __builtin_bit_cast(h8, lo);
        }
    if constexpr (TRACK) rng_note(*rg, mx);
    return b;
}
// ---- operands beyond fp16's range: a per-sample power of two (round 5) ------------------------------------------------------------
// The reference takes any finite fp32 (net/mlp.py:65, flows/affine.py:104-109, 156-163).  The conditioner inputs and the dense layers'
// inputs -- the flow STATE, the one unbounded operand of the forward kernels -- are therefore rescaled when a sample leaves the range:
// the tracked split hands its running max |v| back, one ballot says whether ANY lane of the wave is beyond 65504 (wave-uniform, not
// taken in practice), and only then the layer is evaluated once more for the whole wave with every sample's operands multiplied by
// 2^-e (e from the sample's own maximum: both lane halves), the products accumulated from zero and the result restored as
// bias + 2^e . acc -- exact scalings, the same three fp16 products.  The fast path pays one v_cmp + s_cbranch per layer.
// split of a tile that also returns the lane's running max |v| (no flag: the caller decides)
template <int NS>
__device__ __forceinline__ btile<NS> make_btile_mx(const tile<NS> &c, float &mx) {
    btile<NS> b;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 hi, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v0 = c.v[n][8 * s + 2 * q], v1 = c.v[n][8 * s + 2 * q + 1];
                mx = rng_max(mx, v0, v1);
                const uint32_t ph = pk_f16(v0, v1);
                hi[q] = ph;
                lo[q] = pk_residual(ph, v0, v1);
            }
            b.hi[n][s] = __builtin_bit_cast(h8, hi);
            b.lo[n][s] = __builtin_bit_cast(h8, lo);
        }
    return b;
}
__device__ __forceinline__ bool rng_over(float mx) {
    return __builtin_amdgcn_ballot_w64(mx > SX_F16_MAX) != 0ull;
}
struct rng_pow2 { float sc, inv; };
// 2^-e / 2^e with |v| 2^-e < 2^15 for every operand of the sample (its max over BOTH lane halves); e = 0 inside the range
__device__ __forceinline__ rng_pow2 rng_pow2_of(float mx) {
    const float m = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
    int e = (int)((__float_as_uint(m) >> 23) & 0xffu) - (127 + 14);
    e = e < 0 ? 0 : (e > 110 ? 110 : e);          // (inf / NaN: the products become inf / NaN like the reference's)
    return rng_pow2{__uint_as_float((uint32_t)(127 - e) << 23), __uint_as_float((uint32_t)(127 + e) << 23)};
}
template <int NS>
__device__ __forceinline__ btile<NS> make_btile_scaled(const tile<NS> &c, float sc) {
    tile<NS> t;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) t.v[n][r] = c.v[n][r] * sc;
    return make_btile_impl<NS, false>(t, nullptr);
}
// bounded operands (tanh / sigmoid-family activations)
template <int NS>
__device__ __forceinline__ btile<NS> make_btile(const tile<NS> &c) { return make_btile_impl<NS, false>(c, nullptr); }
// unbounded operands: tracked
template <int NS>
__device__ __forceinline__ btile<NS> make_btile(const tile<NS> &c, rng_t &rg) { return make_btile_impl<NS, true>(c, &rg); }
template <int NS, class F>
__device__ __forceinline__ void gemm_tile_f(const char *wb, int a_off, const btile<NS> &b, tile<NS> &acc, F &&f) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const u32x4 ahu = *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s) * 256) * 4);       // ds_read_b128, imm offset
        const u32x4 alu = *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s + 1) * 256) * 4);
        const h8 ah = __builtin_bit_cast(h8, ahu), al = __builtin_bit_cast(h8, alu);
        // smallest terms first
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b.hi[n][s], acc.v[n], 0, 0, 0);
        f(8 * s + 0); f(8 * s + 1); f(8 * s + 2);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.lo[n][s], acc.v[n], 0, 0, 0);
        f(8 * s + 3); f(8 * s + 4); f(8 * s + 5);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.hi[n][s], acc.v[n], 0, 0, 0);
        f(8 * s + 6); f(8 * s + 7);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep later tiles' ds_reads from piling up ahead (register pressure)
}
#endif
template <int NS>
__device__ __forceinline__ void gemm_tile(const char *wb, int a_off, const btile<NS> &b, tile<NS> &acc) {
    gemm_tile_f<NS>(wb, a_off, b, acc, [](int) {});
}
// the same without the scheduling fence behind it: the caller interleaves the MFMAs with independent VALU work of its own
template <int NS>
__device__ __forceinline__ void gemm_tile_open(const char *wb, int a_off, const btile<NS> &b, tile<NS> &acc) {
#ifdef SX_F16X3
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const u32x4 ahu = *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s) * 256) * 4);       // ds_read_b128, imm offset
        const u32x4 alu = *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s + 1) * 256) * 4);
        const h8 ah = __builtin_bit_cast(h8, ahu), al = __builtin_bit_cast(h8, alu);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b.hi[n][s], acc.v[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.lo[n][s], acc.v[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.hi[n][s], acc.v[n], 0, 0, 0);
    }
#else
    gemm_tile_f<NS>(wb, a_off, b, acc, [](int) {});
#endif
}

// bias / per-feature constants in C-fragment order: [h][16] floats at off, replicated over the sample tiles
__device__ __forceinline__ f32x16 load_cfrag1(const char *cb, int off) {
    f32x16 v;
    const f32x4 *p = reinterpret_cast<const f32x4 *>(cb + off * 4);
    const f32x4 a = p[0], b = p[1], c = p[2], d = p[3];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    v[12] = d.x; v[13] = d.y; v[14] = d.z; v[15] = d.w;
    return v;
}
template <int NS>
__device__ __forceinline__ tile<NS> load_cfrag(const char *cb, int off) {
    tile<NS> t;
    t.v[0] = load_cfrag1(cb, off);
#pragma unroll
    for (int n = 1; n < NS; ++n) t.v[n] = t.v[0];
    return t;
}

// r = 1/(exp2(z) + 1): the folded form of tanh (the weights carry its constants, see sx_pack_linear)
__device__ __forceinline__ float fast_sig2(float v) { return __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v) + 1.0f); }
// the same on registers i, i+1 of a C tile (i even; odd i is a no-op so callers can pass gemm_tile_f's unit index)
__device__ __forceinline__ void fast_sig2_pair(f32x16 &t, int i) {
    if (i & 1) return;
    t[i] = fast_sig2(t[i]);
    t[i + 1] = fast_sig2(t[i + 1]);
}
// fp32 arithmetic on register pairs, written as scalar operations: beside MFMAs a v_pk_*_f32 costs more than the two scalar
// instructions it replaces (MI355X_MICROARCH.md 'price of one filler beside MFMAs'; measured here 0.423 vs 0.443 ms on cfg 2)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) { return f32x2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) { return f32x2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ f32x2 pk_mul(f32x2 a, f32x2 b) { return f32x2{a.x * b.x, a.y * b.y}; }

__device__ __forceinline__ float act_one(float v, int act) {
    switch (act) {
        case SX_ACT_TANH: return fast_tanh(v);
        case SX_ACT_RELU: return fmaxf(v, 0.f);
        case SX_ACT_SIGMOID: return fast_rcp(1.f + fast_exp(-v));
        case SX_ACT_ELU: return v > 0.f ? v : expm1f(v);
        case SX_ACT_SOFTPLUS: return v > 20.f ? v : log1pf(expf(v));
        case SX_ACT_LEAKYRELU: return v > 0.f ? v : 0.01f * v;
        case SX_ACT_SILU: return v * fast_rcp(1.f + fast_exp(-v));
        case SX_ACT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
        default: return v;
    }
}
// Generic activations are rare: one out-of-line copy keeps the code (and hipcc's compile time) small.
__device__ __attribute__((noinline)) void activate_generic(f32x16 *v, int act) {
    f32x16 t = *v;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = act_one(t[r], act);
    *v = t;
}
template <int NS>
__device__ __forceinline__ void activate(tile<NS> &t, int act) {
    if (act == SX_ACT_TANH) {
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) t.v[n][r] = fast_tanh(t.v[n][r]);
    } else if (act != SX_ACT_IDENTITY) {
#pragma unroll
        for (int n = 0; n < NS; ++n) activate_generic(&t.v[n], act);
    }
}

// per-step LDS pointers: every weight / bias access below is `pointer + compile-time offset`, so the offsets
// fold into the ds_read immediates and no scalar address arithmetic is issued per access
struct wptr {
    const char *wb;   // blob base + lane*16  (A-operand fragments, one ds_read_b128 per lane)
    const char *cb;   // blob base + h*64     (C-fragment constants: bias, per-feature scale / shift)
};
__device__ __forceinline__ wptr make_wptr(int base_floats, int lane) {
    const char *p = reinterpret_cast<const char *>(smem) + base_floats * 4;
    return wptr{p + lane * 16, p + (lane >> 5) * 64};
}

// hidden[m] = act(W . src[C0..C0+CT) + b),  blob = pack_linear(W, HT m-tiles, CT k-tiles) at float offset OFF.
// FOLDED: weights carry tanh's constants, the activation is r = 1/(exp2(z') + 1) (SX_ACT_TANH_FOLDED) and the
// activation of tile m-1 is issued between the MFMAs of tile m; the LAST tile is returned un-activated so the
// caller can hide it under its own MFMAs.  Otherwise: runtime activation `act`, applied in place.
// (body: the B operands `bsrc` are given -- hidden_layer forms them from state tiles, the deep-conditioner steps of the
//  spline kernel keep the previous layer's activations in this form)
template <int NS, int HT, int CT, bool FOLDED>
__device__ __forceinline__ void hidden_body(const btile<NS> (&bsrc)[CT], tile<NS> (&hid)[HT], const wptr w, int off,
                                            int act) {
    const int bias = off + HT * CT * 1024;
    if constexpr (FOLDED) {
        tile<NS> acc = load_cfrag<NS>(w.cb, bias);
#pragma unroll
        for (int c = 0; c < CT; ++c) gemm_tile<NS>(w.wb, off + c * 1024, bsrc[c], acc);
#pragma unroll
        for (int m = 1; m < HT; ++m) {
            tile<NS> nxt = load_cfrag<NS>(w.cb, bias + m * 32);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c == 0)
                    gemm_tile_f<NS>(w.wb, off + (m * CT + c) * 1024, bsrc[c], nxt, [&](int i) {
#pragma unroll
                        for (int n = 0; n < NS; ++n) fast_sig2_pair(acc.v[n], i);
                    });
                else
                    gemm_tile<NS>(w.wb, off + (m * CT + c) * 1024, bsrc[c], nxt);
            }
            hid[m - 1] = acc;
            acc = nxt;
            __builtin_amdgcn_sched_barrier(0);
        }
        hid[HT - 1] = acc;
    } else {
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            tile<NS> acc = load_cfrag<NS>(w.cb, bias + m * 32);
#pragma unroll
            for (int c = 0; c < CT; ++c) gemm_tile<NS>(w.wb, off + (m * CT + c) * 1024, bsrc[c], acc);
            activate<NS>(acc, act);
            hid[m] = acc;
        }
    }
}

template <int NS, int NSRC, int HT, int C0, int CT, bool FOLDED>
__device__ __forceinline__ void hidden_layer(const tile<NS> (&src)[NSRC], tile<NS> (&hid)[HT], const wptr w, int off,
                                             int act, rng_t &rg) {
    btile<NS> bsrc[CT];          // B operands are formed once and reused by every output tile
    [[maybe_unused]] float mx = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) bsrc[c] = make_btile_mx<NS>(src[C0 + c], mx);
    __builtin_amdgcn_sched_barrier(0);
    hidden_body<NS, HT, CT, FOLDED>(bsrc, hid, w, off, act);
#ifdef SX_F16X3
    rng_note(rg, mx);          // a sample's input beyond fp16's range: named for the exact pass (see rng_note)
#endif
}

// hidden_layer that hands the B fragments of its source tiles back (the training backward contracts them again)
template <int NS, int NSRC, int HT, int C0, int CT, bool FOLDED>
__device__ __forceinline__ void hidden_layer_keep(const tile<NS> (&src)[NSRC], tile<NS> (&hid)[HT], btile<NS> (&bsrc)[CT],
                                                  const wptr w, int off, int act, rng_t &rg) {
#pragma unroll
    for (int c = 0; c < CT; ++c) bsrc[c] = make_btile<NS>(src[C0 + c], rg);
    __builtin_amdgcn_sched_barrier(0);
    hidden_body<NS, HT, CT, FOLDED>(bsrc, hid, w, off, act);
}

// Affine coupling step (affine.py:104-109 through coupling.py:69-95), conditioner evaluated once (quirk Q2).
// FOLDED (the Tanh hot path): no runtime conditionals inside; REV selects (x - sh)*scale vs x*scale + sh.
template <int NS, int TX, int HT, int C0, int CT, int T0, int TT, bool FOLDED, bool REV>
__device__ __forceinline__ void coupling_affine(tile<NS> (&xs)[TX], const wptr w, const dstep &st, float (&ldj)[NS],
                                                rng_t &rg) {
    tile<NS> hid[HT];
    hidden_layer<NS, TX, HT, C0, CT, FOLDED>(xs, hid, w, 0, st.act, rg);
    constexpr int a2 = HT * CT * 1024 + HT * 32;   // pack_linear(W2: 2*TT m-tiles, HT k-tiles)
    constexpr int b2 = a2 + 2 * TT * HT * 1024;
    f32x2 s[NS];         // log-det partial sums, two lanes of v_pk_add_f32
#pragma unroll
    for (int n = 0; n < NS; ++n) s[n] = f32x2{0.f, 0.f};
    if constexpr (FOLDED && HT == 1) {
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; r += 2) fast_sig2_pair(hid[0].v[n], r);
    }
    btile<NS> bh[HT];
    // folded tanh: r in (0, 1), bounded; run-time activations (ReLU, ELU, ...) are not
#pragma unroll
    for (int m = 0; m + 1 < HT; ++m) {
        if constexpr (FOLDED) bh[m] = make_btile<NS>(hid[m]);
        else bh[m] = make_btile<NS>(hid[m], rg);
    }
    if constexpr (!FOLDED) bh[HT - 1] = make_btile<NS>(hid[HT - 1], rg);
    else if constexpr (HT == 1) bh[HT - 1] = make_btile<NS>(hid[HT - 1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        tile<NS> ls = load_cfrag<NS>(w.cb, b2 + (2 * t) * 32);
        tile<NS> sh = load_cfrag<NS>(w.cb, b2 + (2 * t + 1) * 32);
#pragma unroll
        for (int m = 0; m + 1 < HT; ++m) {
            if (FOLDED && t == 0 && m == 0)        // the last hidden tile's activation rides under this k-chunk
                gemm_tile_f<NS>(w.wb, a2 + ((2 * t) * HT + m) * 1024, bh[m], ls, [&](int i) {
#pragma unroll
                    for (int n = 0; n < NS; ++n) fast_sig2_pair(hid[HT - 1].v[n], i);
                });
            else
                gemm_tile<NS>(w.wb, a2 + ((2 * t) * HT + m) * 1024, bh[m], ls);
            gemm_tile<NS>(w.wb, a2 + ((2 * t + 1) * HT + m) * 1024, bh[m], sh);
        }
        if (FOLDED && t == 0 && HT > 1) {
            bh[HT - 1] = make_btile<NS>(hid[HT - 1]);   // its activation just finished
            __builtin_amdgcn_sched_barrier(0);
        }
        gemm_tile<NS>(w.wb, a2 + ((2 * t) * HT + (HT - 1)) * 1024, bh[HT - 1], ls);
        // the scale exp(+-log_scale) rides under the shift tile's last k-chunk; ls is overwritten by it
        const float sgn = FOLDED ? 1.0f : (REV ? -1.44269504088896341f : 1.44269504088896341f);
        gemm_tile_f<NS>(w.wb, a2 + ((2 * t + 1) * HT + (HT - 1)) * 1024, bh[HT - 1], sh, [&](int i) {
            if (i & 1) return;
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                s[n] = pk_add(s[n], f32x2{ls.v[n][i], ls.v[n][i + 1]});
                ls.v[n][i] = __builtin_amdgcn_exp2f(FOLDED ? ls.v[n][i] : ls.v[n][i] * sgn);
                ls.v[n][i + 1] = __builtin_amdgcn_exp2f(FOLDED ? ls.v[n][i + 1] : ls.v[n][i + 1] * sgn);
            }
        });
        tile<NS> &x = xs[T0 + t];
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {      // v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 on register pairs
                const f32x2 xv = {x.v[n][r], x.v[n][r + 1]}, sv = {sh.v[n][r], sh.v[n][r + 1]};
                const f32x2 ev = {ls.v[n][r], ls.v[n][r + 1]};
                const f32x2 yv = REV ? pk_mul(pk_sub(xv, sv), ev) : pk_add(pk_mul(xv, ev), sv);
                x.v[n][r] = yv.x;
                x.v[n][r + 1] = yv.y;
            }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) ldj[n] += st.ldj_scale * (s[n].x + s[n].y);
}
#ifdef SX_F16X3
// ---- the same step with the A fragments one tile ahead ------------------------------------------------------------------------
// Two waves per SIMD (the 128-column kernels, MODE 7 / 8) cannot cover a wave's LDS round trips with other waves' work: here the
// four ds_read_b128 of tile i + 1 go out BEFORE the six MFMAs of tile i (two register sets), through the hidden layer, the output
// layer and across the VALU sections between them, so a wave waits for LDS once per step.  (Counted lgkmcnt waits are what makes
// this work: see stage_blob.)
struct afr { u32x4 q[4]; };
__device__ __forceinline__ afr afr_load(const char *wb, int a_off) {
    afr a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a.q[i] = *reinterpret_cast<const u32x4 *>(wb + (a_off + i * 256) * 4);
    return a;
}
// one tile: request tile `next_off` (< 0: none), then the MFMAs on `cur` with the riders f(0..15) between them, then cur = next
// (an MFMA is a pure instruction too: without a use at its place in the chain of volatile statements, instruction selection sinks the
//  MFMAs of a tile whose result nothing needs yet below all its riders -- the accumulator passes through an empty volatile asm)
#define SX_PIN_ACC(a) asm volatile("" : "+v"(a))
// (PIN = false: kernels that own the whole 512-entry file keep accumulators in AGPRs, where a "+v" pin costs a v_accvgpr read and write
//  per register and MFMA -- the 128-column backward ran 21 ms instead of 13 with them)
template <int NS, bool PIN = true, class F>
__device__ __forceinline__ void gemm_tile_pf(const char *wb, afr &cur, int next_off, const btile<NS> &b, tile<NS> &acc, F &&f) {
    afr nxt = cur;
    if (next_off >= 0) nxt = afr_load(wb, next_off);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const h8 ah = __builtin_bit_cast(h8, cur.q[2 * s]), al = __builtin_bit_cast(h8, cur.q[2 * s + 1]);
#pragma unroll
        for (int n = 0; n < NS; ++n) { acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b.hi[n][s], acc.v[n], 0, 0, 0); if constexpr (PIN) SX_PIN_ACC(acc.v[n]); }
        f(8 * s + 0); f(8 * s + 1); f(8 * s + 2);
        __builtin_amdgcn_sched_barrier(0);       // the riders stay in THIS MFMA's shadow (unfenced, the scheduler gathers them in front of the tile)
#pragma unroll
        for (int n = 0; n < NS; ++n) { acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.lo[n][s], acc.v[n], 0, 0, 0); if constexpr (PIN) SX_PIN_ACC(acc.v[n]); }
        f(8 * s + 3); f(8 * s + 4); f(8 * s + 5);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < NS; ++n) { acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.hi[n][s], acc.v[n], 0, 0, 0); if constexpr (PIN) SX_PIN_ACC(acc.v[n]); }
        f(8 * s + 6); f(8 * s + 7);
        __builtin_amdgcn_sched_barrier(0);
    }
    cur = nxt;
}
// ---- vector work spread BETWEEN the MFMAs (round 5) ------------------------------------------------------------------------------
// tools/coexec_probe.hip, two waves per SIMD, each step = 32 split pairs + 48 MFMAs (a dense half-layer), cycles per step and SIMD
// (matrix-pipe floor 3,072): phases [split][MFMAs] in lockstep behind the barrier 4,223 -- the round-4 structure; the same with
// waves 4..7 running the complementary phase (a "stagger": built here first, with a three-deep weight ring, and measured on cfg 4
// at 1.383 vs 1.384 ms: tools/experiments/cfg4_stagger_three_deep_ring.patch) 4,633; s_setprio around the MFMAs 4,229; the vector
// instructions of the SAME wave placed between its MFMAs 3,385.  A SIMD overlaps a wave's vector instructions with the matrix pipe
// when they sit in the shadow of that wave's own MFMAs, and hardly at all across waves in coarse phases.  So: the fp16 split of source
// tile c + 1 rides between the MFMAs of k-tile c (dense layers: k-major over four live accumulators), a hidden tile's sigmoid and
// split ride under the next tile's MFMAs, the scale's exp2 and the affine map of tile t under the MFMAs of tile t + 1.
// one pair (registers 2p, 2p + 1) of a C tile -> element p of the B operand's hi / lo fragments
// A rider's inputs pass through an empty VOLATILE asm at the point where the rider stands: instruction selection orders pure vector
// instructions by register pressure, not by source position -- unpinned, the sixteen exp2 / rcp of a tile's sigmoid gather in front of
// the tile's first MFMA and the scheduling fences (which only bind the later machine scheduler) find nothing left to hold in place.
__device__ __forceinline__ float pinned(float v) { asm volatile("" : "+v"(v)); return v; }
template <int NS, bool TRACK>
__device__ __forceinline__ void split_pair(const tile<NS> &c, u32x4 (&hi)[NS][2], u32x4 (&lo)[NS][2], int p, float &mx) {
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        const float v0 = c.v[n][2 * p], v1 = c.v[n][2 * p + 1];
        if constexpr (TRACK) mx = rng_max(mx, v0, v1);
        const uint32_t ph = pk_f16(v0, v1);
        hi[n][p >> 2][p & 3] = ph;
        lo[n][p >> 2][p & 3] = pk_residual(ph, v0, v1);
    }
}
template <int NS>
__device__ __forceinline__ btile<NS> btile_of(const u32x4 (&hi)[NS][2], const u32x4 (&lo)[NS][2]) {
    btile<NS> b;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int s = 0; s < 2; ++s) { b.hi[n][s] = __builtin_bit_cast(h8, hi[n][s]); b.lo[n][s] = __builtin_bit_cast(h8, lo[n][s]); }
    return b;
}
// Split coupling on 2 + 2 tiles, folded tanh.  Order of the twelve (HT = 2) gemm tiles and what rides between their MFMAs:
//   [split src 0]  h0.k0 {split src 1}  h0.k1  h1.k0 {sigmoid h0}  h1.k1 {split h0}
//   ls0.k0 {sigmoid h1}  sh0.k0 {split h1, pairs 0..3}  ls1.k0 {split h1, pairs 4..7}  sh1.k0
//   ls0.k1  sh0.k1 {exp2 ls0, log-det}  ls1.k1 {affine map of tile 0}  sh1.k1 {exp2 ls1, log-det}   [affine map of tile 1]
// ([..] = not covered by MFMAs of this wave.)  The output layer runs k-major over four live accumulators.
template <int NS, int TX, int HT, int C0, int CT, int T0, int TT, bool REV>
__device__ __forceinline__ void coupling_affine_pf(tile<NS> (&xs)[TX], const wptr w, const dstep &st, float (&ldj)[NS],
                                                   rng_t &rg) {
    static_assert(CT == 2 && HT <= 2, "coupling_affine_pf: two conditioner tiles, hidden <= 64");
    constexpr int a2 = HT * CT * 1024 + HT * 32;   // pack_linear(W2: 2*TT m-tiles, HT k-tiles)
    constexpr int b2 = a2 + 2 * TT * HT * 1024;
    constexpr int bias1 = HT * CT * 1024;
    constexpr int NH = HT * CT, NO = 2 * TT * HT;
    // offset of the q-th gemm tile in execution order: hidden m-major, output k-major
    auto off_of = [](int q) { return q < NH ? q * 1024 : (q < NH + NO ? a2 + (((q - NH) % (2 * TT)) * HT + (q - NH) / (2 * TT)) * 1024 : -1); };
    auto none = [](int) {};
    afr cur = afr_load(w.wb, 0);                   // the first tile's fragments fly under the split of the first source tile
    float mx = 0.f;
    u32x4 shi[NS][2], slo[NS][2];
    btile<NS> bsrc0 = make_btile_mx<NS>(xs[C0], mx);
    tile<NS> hid[HT];
    int q = 0;
    {
        tile<NS> acc = load_cfrag<NS>(w.cb, bias1);
        gemm_tile_pf<NS>(w.wb, cur, off_of(q + 1), bsrc0, acc, [&](int i) { if (!(i & 1)) split_pair<NS, true>(xs[C0 + 1], shi, slo, i >> 1, mx); });
        ++q;
        const btile<NS> bsrc1 = btile_of<NS>(shi, slo);
        gemm_tile_pf<NS>(w.wb, cur, off_of(q + 1), bsrc1, acc, none);
        ++q;
        hid[0] = acc;
        if constexpr (HT == 2) {
            tile<NS> acc1 = load_cfrag<NS>(w.cb, bias1 + 32);
            gemm_tile_pf<NS>(w.wb, cur, off_of(q + 1), bsrc0, acc1, [&](int i) {
                if (i & 1) return;
#pragma unroll
                for (int n = 0; n < NS; ++n) { hid[0].v[n][i] = pinned(fast_sig2(hid[0].v[n][i])); hid[0].v[n][i + 1] = pinned(fast_sig2(hid[0].v[n][i + 1])); }
            });
            ++q;
            gemm_tile_pf<NS>(w.wb, cur, off_of(q + 1), bsrc1, acc1, [&](int i) { if (!(i & 1)) split_pair<NS, false>(hid[0], shi, slo, i >> 1, mx); });
            ++q;
            hid[1] = acc1;
        }
        rng_note(rg, mx);      // a sample's conditioner input beyond fp16's range: named for the exact pass (rng_note)
    }
    btile<NS> bh[HT];
    if constexpr (HT == 1) {
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; r += 2) fast_sig2_pair(hid[0].v[n], r);
        bh[0] = make_btile<NS>(hid[0]);
    } else {
        bh[0] = btile_of<NS>(shi, slo);
    }
    f32x2 s[NS];         // log-det partial sums
#pragma unroll
    for (int n = 0; n < NS; ++n) s[n] = f32x2{0.f, 0.f};
    tile<NS> out[2 * TT];
#pragma unroll
    for (int r = 0; r < 2 * TT; ++r) out[r] = load_cfrag<NS>(w.cb, b2 + r * 32);
    auto exp_rider = [&](tile<NS> &ls, int i) {
        if (i & 1) return;
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            // (results pinned too: a pure instruction may also SINK -- the last tile's exp2 and the whole log-det chain otherwise end up
            //  behind the step's last MFMA)
            const float l0 = ls.v[n][i], l1 = ls.v[n][i + 1];
            s[n].x = pinned(s[n].x + l0);
            s[n].y = pinned(s[n].y + l1);
            ls.v[n][i] = pinned(__builtin_amdgcn_exp2f(l0));
            ls.v[n][i + 1] = pinned(__builtin_amdgcn_exp2f(l1));
        }
    };
    auto affine_rider = [&](tile<NS> &x, const tile<NS> &e, const tile<NS> &sh, int i) {
        if (i & 1) return;
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const f32x2 xv = {x.v[n][i], x.v[n][i + 1]}, sv = {sh.v[n][i], sh.v[n][i + 1]}, ev = {e.v[n][i], e.v[n][i + 1]};
            const f32x2 yv = REV ? pk_mul(pk_sub(xv, sv), ev) : pk_add(pk_mul(xv, ev), sv);
            x.v[n][i] = pinned(yv.x);
            x.v[n][i + 1] = pinned(yv.y);
        }
    };
#pragma unroll
    for (int k = 0; k < HT; ++k) {
#pragma unroll
        for (int r = 0; r < 2 * TT; ++r) {
            const bool last_k = k == HT - 1;
            gemm_tile_pf<NS>(w.wb, cur, off_of(q + 1), bh[k], out[r], [&](int i) {
                if (HT == 2 && k == 0) {
                    // the last hidden tile: its sigmoid under the first tile of this k-chunk, its split under the next two
                    if (r == 0) {
                        if (!(i & 1)) {
#pragma unroll
                            for (int n = 0; n < NS; ++n) {
                                hid[HT - 1].v[n][i] = pinned(fast_sig2(hid[HT - 1].v[n][i]));
                                hid[HT - 1].v[n][i + 1] = pinned(fast_sig2(hid[HT - 1].v[n][i + 1]));
                            }
                        }
                    } else if (r <= 2) {
                        if ((i & 3) == 0) split_pair<NS, false>(hid[HT - 1], shi, slo, 4 * (r - 1) + (i >> 2), mx);
                    }
                }
                if (last_k) {
                    if (r & 1) exp_rider(out[r - 1], i);                                          // sh_t's MFMAs: exp2 of ls_t
                    else if (r >= 2) affine_rider(xs[T0 + r / 2 - 1], out[r - 2], out[r - 1], i);  // ls_t's MFMAs: the map of tile t - 1
                }
            });
            ++q;
            if (HT == 2 && k == 0 && r == 2) bh[1] = btile_of<NS>(shi, slo);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i += 2) affine_rider(xs[T0 + TT - 1], out[2 * TT - 2], out[2 * TT - 1], i);
#pragma unroll
    for (int n = 0; n < NS; ++n) ldj[n] += st.ldj_scale * (s[n].x + s[n].y);
}
// ---- the split step on 1 + 1 tiles, hidden 33..64 (MODE 5 / 6, cfg 2), scheduled at k16-step grain -----------------------------
// The same instructions as coupling_affine<.., 2, 2, ..>, every accumulator fed in the same order (k-tile 0 then 1, step 0 then 1,
// smallest term first), so each row's result is the same bits; what changes is where the vector work stands.  The unit is a GROUP:
// the three MFMAs (al.bhi, ah.blo, ah.bhi) of one k16-step of one output tile, with a GAP behind each MFMA that takes riders of at
// most 24 issue cycles (a transcendental 8, anything else 4: tools/gap_census.py counts them in the assembly).  Nothing new is live:
// a group's two A fragments are requested behind the previous group's last MFMA, one set.
//   [X 0-3]  H0.s0 H1.s0 {X 4-7}  H0.s1 {nop}  H1.s1 {S h0 ..}  [S h0 pairs ..3, P h0 0-3]
//   LS.k0s0 SH.k0s0 {S h0 4-7}  [P h0 4-7]  LS.k0s1 SH.k0s1 {S h1 0-3}  [P h1 0-3]  LS.k1s0 SH.k1s0 {S h1 4-7}  [P h1 4-7]
//   LS.k1s1 {nop}  SH.k1s1 {E ..}  [E, F]
// X = tracked split of a source pair, S = exp2, add, rcp of a hidden pair, P = its split, E = log-det add + exp2 of a log-scale
// pair, F = the affine map; {..} rides in the gaps, [..] is not covered by MFMAs of this wave.  Every rider's result passes
// through `pinned` (see coupling_affine_pf) and a scheduling fence closes every gap.
struct ks_frag { h8 ah, al; };
__device__ __forceinline__ ks_frag ks_load(const char *wb, int a_off, int s) {
    const u32x4 ahu = *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s) * 256) * 4);       // ds_read_b128, imm offset
    const u32x4 alu = *reinterpret_cast<const u32x4 *>(wb + (a_off + (2 * s + 1) * 256) * 4);
    return ks_frag{__builtin_bit_cast(h8, ahu), __builtin_bit_cast(h8, alu)};
}
__device__ __forceinline__ uint32_t pinned_u(uint32_t v) { asm volatile("" : "+v"(v)); return v; }
template <int LO, int HI, class F>
__device__ __forceinline__ void ks_ops(F &&f) {
#pragma unroll
    for (int j = LO; j < HI; ++j) f(j);
}
template <int NS, class R1, class R2, class R3>
__device__ __forceinline__ void ks_group(tile<NS> &acc, const ks_frag &a, const u32x4 (&hi)[NS][2], const u32x4 (&lo)[NS][2], int s,
                                         R1 &&r1, R2 &&r2, R3 &&r3) {
#pragma unroll
    for (int n = 0; n < NS; ++n) { acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.al, __builtin_bit_cast(h8, hi[n][s]), acc.v[n], 0, 0, 0); SX_PIN_ACC(acc.v[n]); }
    __builtin_amdgcn_sched_barrier(0);          // (a rider is a pure instruction too: unfenced it rises above the MFMA it rides under)
    r1();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NS; ++n) { acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.ah, __builtin_bit_cast(h8, lo[n][s]), acc.v[n], 0, 0, 0); SX_PIN_ACC(acc.v[n]); }
    __builtin_amdgcn_sched_barrier(0);
    r2();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NS; ++n) { acc.v[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.ah, __builtin_bit_cast(h8, hi[n][s]), acc.v[n], 0, 0, 0); SX_PIN_ACC(acc.v[n]); }
    __builtin_amdgcn_sched_barrier(0);
    r3();
    __builtin_amdgcn_sched_barrier(0);
}
template <int NS, int C0, int T0, bool REV>
__device__ __forceinline__ void coupling_affine_ks(tile<NS> (&xs)[2], const wptr w, const dstep &st, float (&ldj)[NS], rng_t &rg) {
    constexpr int bias1 = 2 * 1024;                // pack_linear(W1: 2 m-tiles, 1 k-tile)
    constexpr int a2 = bias1 + 2 * 32;             // pack_linear(W2: (ls, sh) m-tiles, 2 k-tiles): tile (r, k) at a2 + (2 r + k) * 1024
    constexpr int b2 = a2 + 4 * 1024;
    static_assert(NS == 1, "coupling_affine_ks: one sample tile per wave");
    const tile<NS> &src = xs[C0];
    tile<NS> &x = xs[T0];
    float mx;
    float t0[NS][4], t1[NS][4];                    // the residuals of the four pairs a split stream stands at
    u32x4 xhi[NS][2], xlo[NS][2], phi[NS][2], plo[NS][2];
    f32x2 sum[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) sum[n] = f32x2{0.f, 0.f};
    // the two groups that have no rider: the wave stands aside for six cycles behind each of their MFMAs, so its SIMD partners' vector
    // work gets the issue port (measured: profiles/ab_head_kstep_cfg2.txt -- the schedule alone ties the old step, with this -1.3 %)
    auto aside = [] { asm volatile("s_nop 5"); };
    // Every stream runs four chains abreast (a transcendental's or an asm statement's result costs wait states when the next
    // instruction reads it: chain by chain the riders came with 93 s_nop per arm)
    // X: (max3, cvt) x 4, residual x 8, cvt x 4 on the four source pairs 4 (j / 20) ..
    auto x_op = [&](int j) {
        const int q = 4 * (j / 20), k = j % 20;
        const int p = q + (k < 8 ? k / 2 : (k < 16 ? (k - 8) / 2 : k - 16));
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const float v0 = src.v[n][2 * p], v1 = src.v[n][2 * p + 1];
            const uint32_t ph = xhi[n][p >> 2][p & 3];
            if (k < 8 && !(k & 1)) {
                if (j == 0) asm("v_max3_f32 %0, 0, |%1|, |%2|" : "=v"(mx) : "v"(v0), "v"(v1));      // (no register for the chain's zero)
                else mx = rng_max(mx, v0, v1);
                mx = pinned(mx);
            } else if (k < 8) xhi[n][p >> 2][p & 3] = pinned_u(pk_f16(v0, v1));
            else if (k < 16 && !(k & 1)) { asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(t0[n][p & 3]) : "v"(ph), "v"(v0)); t0[n][p & 3] = pinned(t0[n][p & 3]); }
            else if (k < 16) { asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1[n][p & 3]) : "v"(ph), "v"(v1)); t1[n][p & 3] = pinned(t1[n][p & 3]); }
            else xlo[n][p >> 2][p & 3] = pinned_u(pk_f16(t0[n][p & 3], t1[n][p & 3]));
        }
    };
    // S: exp2 x 4, add x 4, rcp x 4 on the hidden registers 4 (j / 12) .., in place
    auto s_op = [&](float (&h)[NS][16], int j) {
        const int k = j % 12, r = 4 * (j / 12) + (k & 3);
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const float v = h[n][r];
            h[n][r] = pinned(k < 4 ? __builtin_amdgcn_exp2f(v) : (k < 8 ? v + 1.0f : __builtin_amdgcn_rcpf(v)));
        }
    };
    // P: cvt x 4, residual x 8, cvt x 4 on the four activated pairs 4 (j / 16) .. (bounded: not tracked)
    auto p_op = [&](const float (&h)[NS][16], int j) {
        const int q = 4 * (j / 16), k = j % 16;
        const int p = q + (k < 4 ? k : (k < 12 ? (k - 4) / 2 : k - 12));
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const float v0 = h[n][2 * p], v1 = h[n][2 * p + 1];
            const uint32_t ph = phi[n][p >> 2][p & 3];
            if (k < 4) phi[n][p >> 2][p & 3] = pinned_u(pk_f16(v0, v1));
            else if (k < 12 && !(k & 1)) { asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(t0[n][p & 3]) : "v"(ph), "v"(v0)); t0[n][p & 3] = pinned(t0[n][p & 3]); }
            else if (k < 12) { asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1[n][p & 3]) : "v"(ph), "v"(v1)); t1[n][p & 3] = pinned(t1[n][p & 3]); }
            else plo[n][p >> 2][p & 3] = pinned_u(pk_f16(t0[n][p & 3], t1[n][p & 3]));
        }
    };
    tile<NS> ls, sh;
    // E: the log-det adds of log-scale pair p = j / 4, then its exp2 in place
    auto e_op = [&](int j) {
        const int p = j / 4, k = j % 4;
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            if (k == 0) sum[n].x = pinned(sum[n].x + ls.v[n][2 * p]);
            else if (k == 1) sum[n].y = pinned(sum[n].y + ls.v[n][2 * p + 1]);
            else ls.v[n][2 * p + k - 2] = pinned(__builtin_amdgcn_exp2f(ls.v[n][2 * p + k - 2]));
        }
    };
    // F: the affine map of pair p
    auto f_op = [&](int p) {
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const f32x2 xv = {x.v[n][2 * p], x.v[n][2 * p + 1]}, sv = {sh.v[n][2 * p], sh.v[n][2 * p + 1]};
            const f32x2 ev = {ls.v[n][2 * p], ls.v[n][2 * p + 1]};
            const f32x2 yv = REV ? pk_mul(pk_sub(xv, sv), ev) : pk_add(pk_mul(xv, ev), sv);
            x.v[n][2 * p] = yv.x;
            x.v[n][2 * p + 1] = yv.y;
        }
    };
    tile<NS> c0, c1;
    float h0[NS][16], h1[NS][16];                  // the hidden tiles as single registers once their GEMM is done: halves die separately
    ks_frag f, g;
    ks_ops<0, 5>(x_op);
    __builtin_amdgcn_sched_barrier(0);
    c0 = load_cfrag<NS>(w.cb, bias1);
    f = ks_load(w.wb, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    ks_ops<5, 20>(x_op);
    __builtin_amdgcn_sched_barrier(0);
    ks_group<NS>(c0, f, xhi, xlo, 0, [&] { ks_ops<20, 24>(x_op); }, [&] { ks_ops<24, 28>(x_op); },
                 [&] { c1 = load_cfrag<NS>(w.cb, bias1 + 32); g = ks_load(w.wb, 1024, 0); ks_ops<28, 31>(x_op); });
    ks_group<NS>(c1, g, xhi, xlo, 0, [&] { ks_ops<31, 34>(x_op); }, [&] { ks_ops<34, 37>(x_op); },
                 [&] { f = ks_load(w.wb, 0, 1); ks_ops<37, 40>(x_op); rng_note(rg, mx); });
    ks_group<NS>(c0, f, xhi, xlo, 1, aside, aside, [&] { aside(); g = ks_load(w.wb, 1024, 1); });
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) h0[n][r] = c0.v[n][r];
    ks_group<NS>(c1, g, xhi, xlo, 1, [&] { ks_ops<0, 3>([&](int j) { s_op(h0, j); }); }, [&] { ks_ops<3, 8>([&](int j) { s_op(h0, j); }); },
                 [&] { f = ks_load(w.wb, a2, 0); ks_ops<8, 11>([&](int j) { s_op(h0, j); }); });
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[n][r] = c1.v[n][r];
    ks_ops<11, 24>([&](int j) { s_op(h0, j); });
    ks_ops<0, 8>([&](int j) { p_op(h0, j); });
    __builtin_amdgcn_sched_barrier(0);
    ls = load_cfrag<NS>(w.cb, b2);                 // (the output biases as late as their first MFMA allows: 32 registers)
    __builtin_amdgcn_sched_barrier(0);
    ks_ops<8, 16>([&](int j) { p_op(h0, j); });
    __builtin_amdgcn_sched_barrier(0);
    // the output layer: k-tile 0 under the rest of h0's and the first half of h1's activation, k-tile 1 under the second half
    ks_group<NS>(ls, f, phi, plo, 0, [&] { ks_ops<24, 27>([&](int j) { s_op(h0, j); }); }, [&] { ks_ops<27, 32>([&](int j) { s_op(h0, j); }); },
                 [&] { sh = load_cfrag<NS>(w.cb, b2 + 32); g = ks_load(w.wb, a2 + 2 * 1024, 0); ks_ops<32, 35>([&](int j) { s_op(h0, j); }); });
    ks_group<NS>(sh, g, phi, plo, 0, [&] { ks_ops<35, 38>([&](int j) { s_op(h0, j); }); }, [&] { ks_ops<38, 42>([&](int j) { s_op(h0, j); }); },
                 [&] { f = ks_load(w.wb, a2, 1); ks_ops<42, 46>([&](int j) { s_op(h0, j); }); });
    ks_ops<46, 48>([&](int j) { s_op(h0, j); });
    ks_ops<16, 32>([&](int j) { p_op(h0, j); });
    __builtin_amdgcn_sched_barrier(0);
    ks_group<NS>(ls, f, phi, plo, 1, [&] { ks_ops<0, 3>([&](int j) { s_op(h1, j); }); }, [&] { ks_ops<3, 8>([&](int j) { s_op(h1, j); }); },
                 [&] { g = ks_load(w.wb, a2 + 2 * 1024, 1); ks_ops<8, 11>([&](int j) { s_op(h1, j); }); });
    ks_group<NS>(sh, g, phi, plo, 1, [&] { ks_ops<11, 14>([&](int j) { s_op(h1, j); }); }, [&] { ks_ops<14, 18>([&](int j) { s_op(h1, j); }); },
                 [&] { f = ks_load(w.wb, a2 + 1024, 0); ks_ops<18, 22>([&](int j) { s_op(h1, j); }); });
    ks_ops<22, 24>([&](int j) { s_op(h1, j); });
    ks_ops<0, 16>([&](int j) { p_op(h1, j); });
    __builtin_amdgcn_sched_barrier(0);
    ks_group<NS>(ls, f, phi, plo, 0, [&] { ks_ops<24, 27>([&](int j) { s_op(h1, j); }); }, [&] { ks_ops<27, 32>([&](int j) { s_op(h1, j); }); },
                 [&] { g = ks_load(w.wb, a2 + 3 * 1024, 0); ks_ops<32, 35>([&](int j) { s_op(h1, j); }); });
    ks_group<NS>(sh, g, phi, plo, 0, [&] { ks_ops<35, 38>([&](int j) { s_op(h1, j); }); }, [&] { ks_ops<38, 42>([&](int j) { s_op(h1, j); }); },
                 [&] { f = ks_load(w.wb, a2 + 1024, 1); ks_ops<42, 46>([&](int j) { s_op(h1, j); }); });
    ks_ops<46, 48>([&](int j) { s_op(h1, j); });
    ks_ops<16, 32>([&](int j) { p_op(h1, j); });
    __builtin_amdgcn_sched_barrier(0);
    ks_group<NS>(ls, f, phi, plo, 1, aside, aside, [&] { aside(); g = ks_load(w.wb, a2 + 3 * 1024, 1); });
    ks_group<NS>(sh, g, phi, plo, 1, [&] { ks_ops<0, 4>(e_op); }, [&] { ks_ops<4, 8>(e_op); }, [&] { ks_ops<8, 12>(e_op); });
    ks_ops<12, 32>(e_op);
    ks_ops<0, 8>(f_op);
#pragma unroll
    for (int n = 0; n < NS; ++n) ldj[n] += st.ldj_scale * (sum[n].x + sum[n].y);
}
#endif
// Deep conditioners (>= 2 hidden layers, kernel MODE 9): the earlier hidden layers ran as their own steps and left their
// activations in `hsrc`; this step evaluates the last hidden layer from them, then the output layer and the affine map.
template <int NS, int TX, int HT, int T0, int TT, bool REV>
__device__ __forceinline__ void coupling_affine_deep(tile<NS> (&xs)[TX], const tile<NS> (&hsrc)[HT], const wptr w,
                                                     const dstep &st, float (&ldj)[NS], rng_t &rg) {
    tile<NS> hid[HT];
    hidden_layer<NS, HT, HT, 0, HT, false>(hsrc, hid, w, 0, st.act, rg);
    constexpr int a2 = HT * HT * 1024 + HT * 32;       // pack_linear(W_out: 2*TT m-tiles, HT k-tiles)
    constexpr int b2 = a2 + 2 * TT * HT * 1024;
    btile<NS> bh[HT];
#pragma unroll
    for (int m = 0; m < HT; ++m) bh[m] = make_btile<NS>(hid[m], rg);
    __builtin_amdgcn_sched_barrier(0);
    float s[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) s[n] = 0.f;
    const float sgn = REV ? -1.44269504088896341f : 1.44269504088896341f;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        tile<NS> ls = load_cfrag<NS>(w.cb, b2 + (2 * t) * 32);
        tile<NS> sh = load_cfrag<NS>(w.cb, b2 + (2 * t + 1) * 32);
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            gemm_tile<NS>(w.wb, a2 + ((2 * t) * HT + m) * 1024, bh[m], ls);
            gemm_tile<NS>(w.wb, a2 + ((2 * t + 1) * HT + m) * 1024, bh[m], sh);
        }
        tile<NS> &x = xs[T0 + t];
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[n] += ls.v[n][r];
                const float e = __builtin_amdgcn_exp2f(ls.v[n][r] * sgn);
                x.v[n][r] = REV ? (x.v[n][r] - sh.v[n][r]) * e : x.v[n][r] * e + sh.v[n][r];
            }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) ldj[n] += st.ldj_scale * s[n];
}

// Hidden layers wider than the program's hidden tiles (round 4: hidden 128 -> 160 used to cost 6x, the layer left the fused tier):
// W2 tanh(W1 z + b1) + b2 is a SUM over hidden-unit chunks, so a coupling is a run of CHUNK steps -- each evaluates its 32 HT
// hidden units (folded tanh) and adds its share of (kk log_scale, shift) to accumulator tiles that live in registers across the
// steps (`pacc`: 2 TT tiles, kernel MODE 9); the first chunk's bias carries b2, every chunk's its own share of the folded
// constant W2 1; the last chunk applies the affine map.  step.pad: bit 0 first, bit 1 last chunk.
template <int NS, int TX, int HT, int C0, int CT, int T0, int TT, bool REV, int PN>
__device__ __forceinline__ void coupling_affine_chunk(tile<NS> (&xs)[TX], tile<NS> (&pacc)[PN], const wptr w, const dstep &st,
                                                      float (&ldj)[NS], rng_t &rg) {
    tile<NS> hid[HT];
    hidden_layer<NS, TX, HT, C0, CT, true>(xs, hid, w, 0, SX_ACT_TANH_FOLDED, rg);
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int r = 0; r < 16; r += 2) fast_sig2_pair(hid[HT - 1].v[n], r);        // (the layer returns its last tile un-activated)
    btile<NS> bh[HT];
#pragma unroll
    for (int m = 0; m < HT; ++m) bh[m] = make_btile<NS>(hid[m]);
    __builtin_amdgcn_sched_barrier(0);
    constexpr int a2 = HT * CT * 1024 + HT * 32;       // pack_linear(W2 chunk: 2 TT m-tiles, HT k-tiles)
    constexpr int b2 = a2 + 2 * TT * HT * 1024;
    const bool first = st.pad & 1, last = st.pad & 2;
#pragma unroll
    for (int t = 0; t < 2 * TT; ++t) {
        tile<NS> acc = load_cfrag<NS>(w.cb, b2 + t * 32);
        if (!first) {
#pragma unroll
            for (int n = 0; n < NS; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc.v[n][r] += pacc[t].v[n][r];
        }
#pragma unroll
        for (int m = 0; m < HT; ++m) gemm_tile<NS>(w.wb, a2 + (t * HT + m) * 1024, bh[m], acc);
        pacc[t] = acc;
    }
    if (last) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            tile<NS> &x = xs[T0 + t];
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float l = pacc[2 * t].v[n][r], sh = pacc[2 * t + 1].v[n][r];       // l = kk log_scale (the pack folds kk in)
                    s += l;
                    const float e = __builtin_amdgcn_exp2f(l);
                    x.v[n][r] = REV ? (x.v[n][r] - sh) * e : x.v[n][r] * e + sh;
                }
                ldj[n] += st.ldj_scale * s;
            }
        }
    }
}
template <int NS, int TX, int HT, int C0, int CT, int T0, int TT, int PN>
__device__ __forceinline__ void coupling_affine_chunk_dispatch(tile<NS> (&xs)[TX], tile<NS> (&pacc)[PN], const wptr w, const dstep &st,
                                                               float (&ldj)[NS], rng_t &rg) {
    if (st.reverse) coupling_affine_chunk<NS, TX, HT, C0, CT, T0, TT, true>(xs, pacc, w, st, ldj, rg);
    else coupling_affine_chunk<NS, TX, HT, C0, CT, T0, TT, false>(xs, pacc, w, st, ldj, rg);
}

// 129 .. 256 columns (round 4: D 128 -> 160 used to cost 12x, the flow left the fused tier): eight state tiles at one wave per SIMD
// (kernel MODE 20, TX = 8).  A coupling whose mask splits the tiles is 1 + 4 steps -- the weights of a whole coupling (48 HT KB) do not
// fit the LDS ring, those of its pieces do:
//   WIDE_HIDDEN       r = folded tanh(W1' . the four conditioning tiles + b1'), kept as B fragments (`bhp`) across the steps (16 HT KB);
//   WIDE_AFFINE_TILE  one transformed tile: (kk log_scale, shift) = W2'[the tile's rows] . r + b2', the affine map, the log-det (8 HT KB).
template <int TX, int HT, int C0>
__device__ __forceinline__ void wide_hidden(tile<1> (&xs)[TX], btile<1> (&bhp)[HT], const wptr w, rng_t &rg) {
    tile<1> hid[HT];
#ifdef SX_F16X3
    // One wave per SIMD (eight state tiles): nothing covers a gemm tile's LDS round trips but the wave itself -- the in-kernel stamps put
    // 70 % of the wave's lifetime in these arms at ~17 % matrix-pipe use (round 5).  The A fragments of gemm tile q + 1 are requested
    // before the MFMAs of tile q (gemm_tile_pf, unpinned: the accumulators of a 512-register kernel live in AGPRs), hidden tile m - 1's
    // sigmoid rides under tile m; operands beyond fp16's range take hidden_layer's rescale afterwards.
    constexpr int CT = TX / 2;
    float mx = 0.f;
    btile<1> bsrc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) bsrc[c] = make_btile_mx<1>(xs[C0 + c], mx);
    __builtin_amdgcn_sched_barrier(0);
    afr cura = afr_load(w.wb, 0);
    constexpr int bias = HT * CT * 1024;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        tile<1> acc = load_cfrag<1>(w.cb, bias + m * 32);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int qn = m * CT + c + 1;
            const int next_off = qn < HT * CT ? qn * 1024 : -1;
            if (m > 0 && c == 0)
                gemm_tile_pf<1, false>(w.wb, cura, next_off, bsrc[c], acc, [&](int i) { fast_sig2_pair(hid[m > 0 ? m - 1 : 0].v[0], i); });
            else
                gemm_tile_pf<1, false>(w.wb, cura, next_off, bsrc[c], acc, [](int) {});
        }
        hid[m] = acc;
    }
    rng_note(rg, mx);
#else
    hidden_layer<1, TX, HT, C0, TX / 2, true>(xs, hid, w, 0, SX_ACT_TANH_FOLDED, rg);
#endif
#pragma unroll
    for (int r = 0; r < 16; r += 2) fast_sig2_pair(hid[HT - 1].v[0], r);
#pragma unroll
    for (int m = 0; m < HT; ++m) bhp[m] = make_btile<1>(hid[m]);
}
template <int TX, int HT>
__device__ __forceinline__ void wide_affine_tile(tile<1> (&xs)[TX], const btile<1> (&bhp)[HT], const wptr w, const dstep &st, float &ldj) {
    tile<1> ls = load_cfrag<1>(w.cb, 2 * HT * 1024), sh = load_cfrag<1>(w.cb, 2 * HT * 1024 + 32);
#ifdef SX_F16X3
    afr cura = afr_load(w.wb, 0);
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        gemm_tile_pf<1, false>(w.wb, cura, (HT + m) * 1024, bhp[m], ls, [](int) {});
        gemm_tile_pf<1, false>(w.wb, cura, m + 1 < HT ? (m + 1) * 1024 : -1, bhp[m], sh, [](int) {});
    }
#else
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        gemm_tile<1>(w.wb, m * 1024, bhp[m], ls);
        gemm_tile<1>(w.wb, (HT + m) * 1024, bhp[m], sh);
    }
#endif
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        s += ls.v[0][r];
        ls.v[0][r] = __builtin_amdgcn_exp2f(ls.v[0][r]);          // exp(+-log_scale): the pack folds kk = +-log2 e in
    }
    const bool rev = st.reverse != 0;
#define WIDE_APPLY(T) { asm volatile("" ::: "memory"); _Pragma("unroll") for (int r = 0; r < 16; ++r) \
        xs[T].v[0][r] = rev ? (xs[T].v[0][r] - sh.v[0][r]) * ls.v[0][r] : xs[T].v[0][r] * ls.v[0][r] + sh.v[0][r]; }
    switch (st.t0) {            // (scalar branches: the tile's registers are static in every arm)
        default: WIDE_APPLY(0) break;
        case 1: if constexpr (TX > 1) WIDE_APPLY(1) break;
        case 2: if constexpr (TX > 2) WIDE_APPLY(2) break;
        case 3: if constexpr (TX > 3) WIDE_APPLY(3) break;
        case 4: if constexpr (TX > 4) WIDE_APPLY(4) break;
        case 5: if constexpr (TX > 5) WIDE_APPLY(5) break;
        case 6: if constexpr (TX > 6) WIDE_APPLY(6) break;
        case 7: if constexpr (TX > 7) WIDE_APPLY(7) break;
    }
#undef WIDE_APPLY
    ldj += st.ldj_scale * s;
}

// ------------------------------------------------------------------------------------------------
// Time-conditioned affine coupling (ContinuousAffineCoupling, stribor/flows/coupling.py:184-213; kernel MODE 15):
//   (log_scale, shift) = net(cat[x * mask, latent, t]);  (e_ls, e_sh) = time_net(t).chunk(2)      (net/time_net.py:6-91)
//   y = x exp(log_scale e_ls) + shift e_sh   |   x = (y - shift e_sh) exp(-log_scale e_ls);   log-det = sum log_scale e_ls (1 - mask)
// One step = conditioner GEMM-1 over ALL tiles (data, latent and the time slots: t and t0 sit in the two slots behind the latent
// columns and are filled from row_t / row_t2), GEMM-2 onto the TT data tiles, the time embedding per element and the affine map.
// blob = pack(W1, HT x TX) ++ pack(W2, 2 TT x HT) ++ time constants in C-fragment order per data tile:
//   kinds 1 - 3 (TimeLinear / TimeTanh / TimeLog): [c_ls (32) | c_sh (32)]  (the per-column scale; exp(scale) for TimeLog)
//   kind 4 (TimeFourier(Bounded), K features): K x [w_ls | s_ls | w_sh | s_sh]   (e = sum_k w_k sin(s_k t))
// step.pad_ = time kind | (time select: 0 = row_t, 1 = row_t2) << 8 | K << 16.
// ------------------------------------------------------------------------------------------------
#define SX_TIME_IDENTITY 0
#define SX_TIME_LINEAR 1
#define SX_TIME_TANH 2
#define SX_TIME_LOG 3
#define SX_TIME_FOURIER 4
// sin(x) on v_sin_f32 (argument in revolutions): x / 2 pi carried to double-float accuracy, reduced to [-1/2, 1/2) first
// (libm's sinf keeps a Payne-Hanek table in scratch memory: 448 B per lane in this kernel)
__device__ __forceinline__ float time_sin(float x) {
    const float hi = x * 0.15915494309189535f;
    const float lo = __builtin_fmaf(x, 0.15915494309189535f, -hi) + x * 6.4206383e-9f;      // 1 / (2 pi) = fp32(0.15915494) + 6.42e-9
    const float fr = (hi - __builtin_rintf(hi)) + lo;
    return __builtin_amdgcn_sinf(fr);
}
template <int NS, int TT>
__device__ __forceinline__ void time_embed(const char *cb, int toff, uint32_t code, const float (&tv)[NS], int t,
                                           f32x16 (&els)[NS], f32x16 (&esh)[NS]) {
    const int kind = code & 0xff, K = (code >> 16) & 0xff;
    if (kind == SX_TIME_IDENTITY) {
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) { els[n][r] = tv[n]; esh[n][r] = tv[n]; }
    } else if (kind == SX_TIME_FOURIER) {
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) { els[n][r] = 0.f; esh[n][r] = 0.f; }
        for (int kf = 0; kf < K; ++kf) {
            const int o = toff + (t * K + kf) * 128;
            const f32x16 wl = load_cfrag1(cb, o), sl = load_cfrag1(cb, o + 32), ws = load_cfrag1(cb, o + 64), ss = load_cfrag1(cb, o + 96);
#pragma unroll
            for (int n = 0; n < NS; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    els[n][r] += wl[r] * time_sin(sl[r] * tv[n]);
                    esh[n][r] += ws[r] * time_sin(ss[r] * tv[n]);
                }
        }
    } else {
        const f32x16 cl = load_cfrag1(cb, toff + t * 64), cs = load_cfrag1(cb, toff + t * 64 + 32);
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = cl[r] * tv[n], b = cs[r] * tv[n];
                if (kind == SX_TIME_LINEAR) { els[n][r] = a; esh[n][r] = b; }
                else if (kind == SX_TIME_TANH) { els[n][r] = fast_tanh(a); esh[n][r] = fast_tanh(b); }
                else { els[n][r] = logf(a + 1.f); esh[n][r] = logf(b + 1.f); }       // TimeLog: c = exp(scale)
            }
    }
}
template <int NS, int TX, int HT, int TT, bool FOLDED, bool REV>
__device__ __forceinline__ void coupling_time_affine(tile<NS> (&xs)[TX], const wptr w, const dstep &st, float (&ldj)[NS],
                                                     rng_t &rg, const float (&tv)[NS]) {
    tile<NS> hid[HT];
    hidden_layer<NS, TX, HT, 0, TX, FOLDED>(xs, hid, w, 0, st.act, rg);
    if constexpr (FOLDED) {
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; r += 2) fast_sig2_pair(hid[HT - 1].v[n], r);
    }
    btile<NS> bh[HT];
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        if constexpr (FOLDED) bh[m] = make_btile<NS>(hid[m]);
        else bh[m] = make_btile<NS>(hid[m], rg);
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int a2 = HT * TX * 1024 + HT * 32;       // pack_linear(W2: 2 TT m-tiles, HT k-tiles)
    constexpr int b2 = a2 + 2 * TT * HT * 1024;
    constexpr int toff = b2 + 2 * TT * 32;
    float s[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) s[n] = 0.f;
    const float sgn = FOLDED ? 1.0f : (REV ? -1.44269504088896341f : 1.44269504088896341f);
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        tile<NS> ls = load_cfrag<NS>(w.cb, b2 + (2 * t) * 32);
        tile<NS> sh = load_cfrag<NS>(w.cb, b2 + (2 * t + 1) * 32);
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            gemm_tile<NS>(w.wb, a2 + ((2 * t) * HT + m) * 1024, bh[m], ls);
            gemm_tile<NS>(w.wb, a2 + ((2 * t + 1) * HT + m) * 1024, bh[m], sh);
        }
        f32x16 els[NS], esh[NS];
        time_embed<NS, TT>(w.cb, toff, st.mask, tv, t, els, esh);
        tile<NS> &x = xs[t];
#pragma unroll
        for (int n = 0; n < NS; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float l = ls.v[n][r] * els[n][r];            // FOLDED: kk log_scale e_ls, kk = +-log2 e (the pack folds it in)
                s[n] += l;
                const float e = __builtin_amdgcn_exp2f(FOLDED ? l : l * sgn);
                const float shv = sh.v[n][r] * esh[n][r];
                x.v[n][r] = REV ? (x.v[n][r] - shv) * e : x.v[n][r] * e + shv;
            }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) ldj[n] += st.ldj_scale * s[n];
}
template <int NS, int TX, int HT, int TT>
__device__ __forceinline__ void coupling_time_dispatch(tile<NS> (&xs)[TX], const wptr w, const dstep &st, float (&ldj)[NS],
                                                       rng_t &rg, const float (&tv)[NS]) {
    if (st.act == SX_ACT_TANH_FOLDED) {
        if (st.reverse) coupling_time_affine<NS, TX, HT, TT, true, true>(xs, w, st, ldj, rg, tv);
        else coupling_time_affine<NS, TX, HT, TT, true, false>(xs, w, st, ldj, rg, tv);
    } else {
        if (st.reverse) coupling_time_affine<NS, TX, HT, TT, false, true>(xs, w, st, ldj, rg, tv);
        else coupling_time_affine<NS, TX, HT, TT, false, false>(xs, w, st, ldj, rg, tv);
    }
}

// one runtime dispatch per step on (activation kind, direction) -> straight-line specialisations
template <int NS, int TX, int HT, int C0, int CT, int T0, int TT>
__device__ __forceinline__ void coupling_affine_dispatch(tile<NS> (&xs)[TX], const wptr w, const dstep &st,
                                                         float (&ldj)[NS], rng_t &rg) {
    if (st.act == SX_ACT_TANH_FOLDED) {
        if (st.reverse) coupling_affine<NS, TX, HT, C0, CT, T0, TT, true, true>(xs, w, st, ldj, rg);
        else coupling_affine<NS, TX, HT, C0, CT, T0, TT, true, false>(xs, w, st, ldj, rg);
    } else {
        if (st.reverse) coupling_affine<NS, TX, HT, C0, CT, T0, TT, false, true>(xs, w, st, ldj, rg);
        else coupling_affine<NS, TX, HT, C0, CT, T0, TT, false, false>(xs, w, st, ldj, rg);
    }
}

// Elementwise affine with per-feature constants (st.Affine without latent_net, affine.py:63-64,104-109)
template <int NS, int TX>
__device__ __forceinline__ void affine_const(tile<NS> (&xs)[TX], const wptr w, const dstep &st, int x_tiles,
                                             float (&ldj)[NS]) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TX; ++t) {
        if (t < x_tiles) {
            const f32x16 ls = load_cfrag1(w.cb, t * 32);
            const f32x16 sh = load_cfrag1(w.cb, (TX + t) * 32);
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                if (st.reverse) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) xs[t].v[n][r] = (xs[t].v[n][r] - sh[r]) * fast_exp(-ls[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) xs[t].v[n][r] = xs[t].v[n][r] * fast_exp(ls[r]) + sh[r];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s += ls[r];     // padding slots carry log_scale = 0
        }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) ldj[n] += st.ldj_scale * s;
}


// Point-wise flows inside a fused program (Sigmoid / Logit sigmoid.py:9-56, ELU / LeakyReLU activations.py:11-101): the
// arithmetic of the stand-alone kernel (sx_pointwise_core.h) on the state tiles.  blob = live-slot mask in C-fragment order
// (1 = the slot holds a column, 0 = padding: stays 0 and adds nothing) ++ {log-slope of the LeakyReLU kinds}.  The *_INV kinds
// and LOGIT return MINUS the forward log-derivative at the value produced, like the stand-alone kernel (flow.py:42-47); the
// step's ldj_scale carries the sign that turns it into the program's convention.
template <int NS, int TX, int KIND>
__device__ __forceinline__ void pointwise_tiles(tile<NS> (&xs)[TX], const wptr w, const dstep &st, int x_tiles, int mask_tiles,
                                                float (&ldj)[NS]) {
    const float param = st.ldj_const;
    const float log_slope = *reinterpret_cast<const float *>(w.cb - ((threadIdx.x & 63) >> 5) * 64 + 32 * mask_tiles * 4);
#pragma unroll
    for (int t = 0; t < TX; ++t) {
        if (t < x_tiles) {
            const f32x16 live = load_cfrag1(w.cb, t * 32);
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float out, ld;
                    pw_eval(KIND, param, log_slope, xs[t].v[n][r], out, ld);
                    const bool on = live[r] != 0.f;
                    xs[t].v[n][r] = on ? out : xs[t].v[n][r];
                    s += on ? ld : 0.f;
                }
                ldj[n] += st.ldj_scale * s;
            }
        }
    }
}
template <int NS, int TX>
__device__ __forceinline__ void pointwise_step(tile<NS> (&xs)[TX], const wptr w, const dstep &st, int x_tiles, int mask_tiles,
                                               float (&ldj)[NS]) {
    switch (st.act) {
        case SX_PW_SIGMOID: pointwise_tiles<NS, TX, SX_PW_SIGMOID>(xs, w, st, x_tiles, mask_tiles, ldj); break;
        case SX_PW_LOGIT: pointwise_tiles<NS, TX, SX_PW_LOGIT>(xs, w, st, x_tiles, mask_tiles, ldj); break;
        case SX_PW_ELU: pointwise_tiles<NS, TX, SX_PW_ELU>(xs, w, st, x_tiles, mask_tiles, ldj); break;
        case SX_PW_ELU_INV: pointwise_tiles<NS, TX, SX_PW_ELU_INV>(xs, w, st, x_tiles, mask_tiles, ldj); break;
        case SX_PW_LEAKY_RELU: pointwise_tiles<NS, TX, SX_PW_LEAKY_RELU>(xs, w, st, x_tiles, mask_tiles, ldj); break;
        default: pointwise_tiles<NS, TX, SX_PW_LEAKY_RELU_INV>(xs, w, st, x_tiles, mask_tiles, ldj); break;
    }
}

// Time-dependent point-wise flows inside a program of time couplings (ContinuousTanh / ContinuousActivation, activations.py:125-196;
// kernel MODE 21): the arithmetic of the stand-alone kernel (sx_pointwise_time_core.h) on the data tiles; tv = the row's time.  blob =
// live-slot mask as pointwise_tiles.  Values only (NeuralFlow returns no log-det).
template <int NS, int TX, int KIND>
__device__ __forceinline__ void pointwise_time_tiles(tile<NS> (&xs)[TX], const wptr w, const dstep &st, int x_tiles, const float (&tv)[NS]) {
    float rp[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) rp[n] = pwt_row(KIND, st.ldj_const, tv[n]);
#pragma unroll
    for (int t = 0; t < TX; ++t) {
        if (t < x_tiles) {
            const f32x16 live = load_cfrag1(w.cb, t * 32);
#pragma unroll
            for (int n = 0; n < NS; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float xv = xs[t].v[n][r];
                    float out;
                    if constexpr (KIND == SX_PWT_TANH_FLOW || KIND == SX_PWT_TANH_FLOW_INV) out = pwt_tanh_flow(rp[n], xv).y;
                    else out = pwt_mix(KIND, rp[n], xv);
                    xs[t].v[n][r] = live[r] != 0.f ? out : xv;
                }
        }
    }
}
template <int NS, int TX>
__device__ __forceinline__ void pointwise_time_step(tile<NS> (&xs)[TX], const wptr w, const dstep &st, int x_tiles, const float (&tv)[NS]) {
    switch (st.act) {
        case SX_PWT_TANH_FLOW: pointwise_time_tiles<NS, TX, SX_PWT_TANH_FLOW>(xs, w, st, x_tiles, tv); break;
        case SX_PWT_TANH_FLOW_INV: pointwise_time_tiles<NS, TX, SX_PWT_TANH_FLOW_INV>(xs, w, st, x_tiles, tv); break;
        case SX_PWT_MIX_TANH: pointwise_time_tiles<NS, TX, SX_PWT_MIX_TANH>(xs, w, st, x_tiles, tv); break;
        case SX_PWT_MIX_SIGMOID: pointwise_time_tiles<NS, TX, SX_PWT_MIX_SIGMOID>(xs, w, st, x_tiles, tv); break;
        default: pointwise_time_tiles<NS, TX, SX_PWT_MIX_RELU>(xs, w, st, x_tiles, tv); break;
    }
}

#include "sx_flow_spline.h"      // spline-coupling phases (rqs_* / cub_*)
#include "sx_flow_bwd.h"         // training backward steps

__device__ __forceinline__ void st_elem(void *p, int64_t off, float v, int bf16) {
    if (bf16) reinterpret_cast<uint16_t *>(p)[off] = f32_to_bf16(v);
    else reinterpret_cast<float *>(p)[off] = v;
}

// The x tiles of one sample slot, all pieces issued back to back (flow_fused_kernel's one-flight path); p = the row's first element.
// A bf16 piece stays raw (two dwords, registers of its own) until x_flight_widen; fp32 pieces land in the state registers.
template <int TX>
__device__ __forceinline__ void x_flight_issue(u32x2 (&raw)[TX][4], const uint16_t *p, int h) {
    // (plain loads: the eight pieces of a lane share one 128-B line; the streaming policy re-fetched it between them)
#pragma unroll
    for (int t = 0; t < TX; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) raw[t][q] = *reinterpret_cast<const u32x2 *>(p + 32 * t + 8 * q + 4 * h);
}
template <int TX, int NS>
__device__ __forceinline__ void x_flight_widen(tile<NS> (&xs)[TX], int n, const u32x2 (&raw)[TX][4]) {
#pragma unroll
    for (int t = 0; t < TX; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t a = raw[t][q].x, b = raw[t][q].y;
            xs[t].v[n][4 * q + 0] = __uint_as_float(a << 16); xs[t].v[n][4 * q + 1] = __uint_as_float(a & 0xffff0000u);
            xs[t].v[n][4 * q + 2] = __uint_as_float(b << 16); xs[t].v[n][4 * q + 3] = __uint_as_float(b & 0xffff0000u);
        }
}
template <int TX, int MODE, int NS>
__device__ __forceinline__ void x_flight_issue(tile<NS> (&xs)[TX], int n, const float *p, int h) {
    // spline programs re-read 3.2 MB of blobs from L2 per chunk: x is kept out of their way by the streaming policy
    constexpr bool NT_X = MODE == 3 || MODE == 10 || MODE == 12 || MODE == 13 || MODE == 18 || MODE == 19;
#pragma unroll
    for (int t = 0; t < TX; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
            if constexpr (NT_X) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p + 32 * t + 8 * q + 4 * h));
            else v = *reinterpret_cast<const f32x4 *>(p + 32 * t + 8 * q + 4 * h);
            xs[t].v[n][4 * q + 0] = v.x; xs[t].v[n][4 * q + 1] = v.y;
            xs[t].v[n][4 * q + 2] = v.z; xs[t].v[n][4 * q + 3] = v.w;
        }
}

// A step descriptor out of the kernarg segment, as DWORDS: the eight byte-sized fields of dstep otherwise come through vector
// byte loads (no scalar sub-dword load on gfx9) -- and a vector load's s_waitcnt vmcnt(0) right behind the next step's
// LDS-DMA issue waits for that DMA and for every store still in flight (vector-memory operations retire in order).
__device__ __forceinline__ dstep load_step(const dprog &prog, int idx) {
    static_assert(sizeof(dstep) == 28, "dstep layout");
    const uint32_t *p = reinterpret_cast<const uint32_t *>(&prog.steps[idx]);
    const uint32_t w0 = p[0], w1 = p[1];
    dstep s;
    s.kind = (uint8_t)(w0 & 0xffu); s.c0 = (uint8_t)((w0 >> 8) & 0xffu); s.ct = (uint8_t)((w0 >> 16) & 0xffu); s.t0 = (uint8_t)(w0 >> 24);
    s.tt = (uint8_t)(w1 & 0xffu); s.reverse = (uint8_t)((w1 >> 8) & 0xffu); s.act = (uint8_t)((w1 >> 16) & 0xffu); s.pad = (uint8_t)(w1 >> 24);
    s.blob_off = p[2]; s.blob_floats = p[3];
    s.ldj_scale = __builtin_bit_cast(float, p[4]); s.ldj_const = __builtin_bit_cast(float, p[5]);
    s.mask = p[6];
    return s;
}

struct flow_kargs {     // everything but the program, by value in the kernarg segment
    const float *blobs; const void *x; const float *latent; const int32_t *in_col; const int32_t *out_col;
    void *y; float *ldj_out; float *logp_out; double *sum_out; float *mlp_out; const float *row_t; float *side;
    int64_t mlp_out_stride; int64_t n_rows; int mlp_out_dim; int buf_floats; int bf16; int side_width;
    uint32_t *work;     // {next-chunk ticket, finished workgroups}: dynamic chunk hand-out (NULL = static stride)
    uint32_t *flags;    // caller's error-flag word (SX_FLAG_*; device or host-mapped memory), or NULL
    // MODE 11 (training backward, weight gradients contracted in-kernel; see coupling_affine_bwd_acc)
    const float *frag_in;   // state (x | dL/dx) of the previous launch in fragment order, or NULL: start from z (= x) and row_t
    float *frag_out;        // state for the next launch, or NULL: y receives dL/d(input)
    float *acc_out;         // [n_steps]{[gridDim.x][E2], [gridDim.x][E1]} per-workgroup weight-gradient partials (wgrad_reduce layout)
    // The REDO list (round 6; sx_flow_run2): {count, workgroups done, then (32-row group, bad-sample mask) pairs}.  The fp16 x 3
    // kernel APPENDS the groups that hold a sample whose operand left fp16's range (instead of flagging them); a second launch of
    // the SAME program on the exact-fp32 kernel (redo_pass = 1, the exact blobs) takes its row groups from the list, stores and
    // sums only the samples the mask names, and the last workgroup out empties the list.  NULL: rows are flagged as before.
    uint32_t *redo;
    int redo_pass;
    // The SUM SLOT of the redo pass (sx_flow_run3): one fp64 accumulator, zero between calls.  The main launch has added its batch
    // sum THERE (its sum_out points at the slot: that kernel is the same code whether it adds to the caller's word or to the slot);
    // the redo pass adds the named samples' rows there too, and whoever closes the pass -- workgroup 0 when the list is empty, else
    // the last workgroup out -- moves the total to sum_out and leaves 0 behind.  So the call leaves sum_out EQUAL to the batch sum
    // whatever it held, with no zero-fill launched in front of it.  NULL: the pass adds into sum_out.
    double *sum_slot;
};

// MODE 0: flow programs (coupling / affine-const steps); MODE 1: + persistent hidden state (MLP programs);
// MODE 2: flow programs with dense linear layers (AffineLU / MatrixExponential): + a second state tile set;
// MODE 3: flow programs with rational-quadratic spline couplings: + hidden B operands and the group state;
// MODE 4: training backward of affine-coupling log_prob flows: tiles [0,2) = x, [2,4) = dL/dx
// MODE 11: the same for a pair of layers per launch with the weight gradients contracted in-kernel (fp16 x 3 build)
template <int NS, int TX, int HT, int MODE>
__global__ __launch_bounds__(64 * SX_BLOCK_WAVES(TX, MODE), SX_WAVES_FOR(TX, MODE)) void flow_fused_kernel(const dprog prog, const flow_kargs k) {
    constexpr int WB = SX_BLOCK_WAVES(TX, MODE);      // waves per workgroup
    constexpr int ROWS_PER_BLOCK = 32 * WB * NS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    [[maybe_unused]] const int j = lane & 31, h = lane >> 5;
    const int dim = prog.dim, x_tiles = prog.x_tiles, n_steps = prog.n_steps;
    const int64_t n_rows = k.n_rows;
    // redo pass: the "chunks" are WB * NS listed groups each; an empty list ends the workgroup before it touches LDS
    // (the pass runs on the exact-fp32 kernels only: the fp16 x 3 build carries none of it)
#ifndef SX_F16X3
    const bool redo_pass = k.redo != nullptr && k.redo_pass != 0;
#else
    constexpr bool redo_pass = false;
#endif
    const uint32_t redo_count = redo_pass ? k.redo[0] : 0u;
    if (redo_pass && (uint32_t)blockIdx.x * (uint32_t)(WB * NS) >= redo_count) {
        // (every workgroup reports, the last one out empties the list for the next call -- unless the list IS empty, the ordinary
        //  case: word 1 is zero and stays zero, nobody counts, and workgroup 0 alone hands the main launch's sum over.  Word 0 is
        //  written by the last workgroup out only, after every workgroup has read it: the whole grid takes the same branch.)
        if (threadIdx.x == 0) {
            if (redo_count == 0u) {
                if (blockIdx.x == 0 && k.sum_slot != nullptr) redo_close_sum(k.sum_slot, k.sum_out);
            } else {
                __threadfence();
                if (atomicAdd(k.redo + 1, 1u) == gridDim.x - 1) {
                    __threadfence();
                    if (k.sum_slot != nullptr) redo_close_sum(k.sum_slot, k.sum_out);
                    k.redo[0] = 0u; k.redo[1] = 0u;
                }
            }
        }
        return;
    }
    const int64_t n_chunks = redo_pass ? (int64_t)((redo_count + WB * NS - 1) / (WB * NS)) : (n_rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    const int bf16 = k.bf16, buf_floats = k.buf_floats;
    double block_sum = 0.0;
    // MODE 5 / 6 (the pure split-coupling kernels sit exactly on their 128-register budget): the lane's running fp64 sum lives in LDS
    // (one slot per lane behind the weight ring and the ticket slots: sx_flow_run adds the bytes), not in a register pair carried
    // across the step loop -- round 6's range tracking made the allocator spill that pair to scratch (2 x 4096 chunks x 512 lanes x
    // 12 B = +9 MB of HBM writes per cfg-2 launch: pmc_cfg2.json 145.6 -> 159.2 MB); two LDS instructions per chunk instead
    constexpr bool LDS_SUM = MODE == 5 || MODE == 6;
    [[maybe_unused]] double *lds_sum = reinterpret_cast<double *>(smem + 2 * k.buf_floats + 4) + threadIdx.x;
    if constexpr (LDS_SUM) *lds_sum = 0.0;

    // word 0 of the blob buffer's header: SX_FLAG_* bits raised while the weights were packed (a weight beyond the
    // fp16 x 3 range packs as inf); every launch that uses such weights reports it
    if (blockIdx.x == 0 && threadIdx.x == 0 && k.flags != nullptr && k.blobs != nullptr) {
        const uint32_t wf = reinterpret_cast<const uint32_t *>(k.blobs)[0];
        if (wf) __hip_atomic_fetch_or(k.flags, wf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // prologue: first step's weights into buffer 0, first step's descriptor into registers
    int cur = 0;
    dstep st_next = load_step(prog, 0);
    if ((int64_t)blockIdx.x < n_chunks && n_steps > 0 && st_next.blob_floats)
        stage_blob<WB>(k.blobs + st_next.blob_off, 0, st_next.blob_floats);
    // the DMA fields of the step after next are fetched a step early, so the refill below never waits on a scalar load
    uint32_t dma_off = prog.steps[n_steps > 1 ? 1 : 0].blob_off, dma_floats = prog.steps[n_steps > 1 ? 1 : 0].blob_floats;

    // Chunks (128 rows) are handed out dynamically: workgroups sharing a SIMD do not progress at the same rate (the
    // issue arbiter favours the oldest wave), so a static stride leaves the last third of the kernel with CUs
    // running one workgroup.  Thread 0 takes a ticket for the NEXT chunk in the prologue; it travels to the other
    // waves through LDS across the first step's barrier (two slots, alternating, behind the weight ring).
#ifdef SX_F16X3
    [[maybe_unused]] wacc<HT> WA;
    [[maybe_unused]] sel_t sel;
    if constexpr (MODE == 11) {
        wacc_zero<HT>(WA);
        sel = make_sel(lane);
    }
#endif
    const bool dyn = k.work != nullptr && !redo_pass;      // (the redo pass walks its list with a static stride)
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    // MODE 11 with a single step (the default build): the step's weights stay resident in buffer 0 for the whole launch,
    // and the second buffer's place is taken by a per-wave 16 KB landing zone into which the NEXT chunk's state is
    // prefetched by LDS-DMA while this chunk computes (one wave per SIMD: nothing else would hide that latency)
    const bool resident = MODE == 11 && n_steps == 1;
    const int pf_base = buf_floats;                           // floats; WB * 4096 floats behind buffer 0
    lds_u32 *slot = (lds_u32 *)(smem + (resident ? buf_floats + WB * 4096 : 2 * buf_floats));      // ds_write_b32 / ds_read_b32, ordered by the barrier
    [[maybe_unused]] bool have_pf = false;
    [[maybe_unused]] float gg_next = 0.f;                     // MODE 11: dL/dlog_prob of the prefetched chunk's row
    // whole x tiles in identity column order and no other state tile: the chunk's rows are loaded in one flight (x_flight_issue);
    // ragged widths, gathered columns, latent tiles and the backward kernels' adjoint tiles and fragment paths keep the loads below
    const bool x_flight = MODE != 4 && MODE != 11 && prog.identity_cols && x_tiles == TX && dim == 32 * TX;
    // MODE 5 / 6 on bf16 rows: the NEXT chunk's rows and ticket are requested behind this chunk's last step, in front of its stores,
    // row reduction and LDS sum (below).  The raw pieces are defined there on every path and read only at the top of the next chunk:
    // never live across the step loop, where these kernels have no register to spare (LDS_SUM).  (fp32 rows keep the flight at the
    // top: their 32 raw registers, held across the epilogue as four-register tuples, made <1,2,2,5> spill seven VGPRs to scratch.)
    constexpr bool X_AHEAD = MODE == 5 || MODE == 6;
    [[maybe_unused]] u32x2 xpre[NS][TX][4];
    [[maybe_unused]] uint32_t ticket_pre = 0;
    [[maybe_unused]] bool have_xpre = false;
    int iter = 0;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; ++iter) {
        // lane-derived indices are re-derived per chunk from the thread id (opaque to the optimizer) instead of
        // living in -- or being spilled from -- registers across the step loop
        uint32_t tid_ = threadIdx.x;
        asm volatile("" : "+v"(tid_));
        [[maybe_unused]] const int lane = tid_ & 63, wave = tid_ >> 6, j = lane & 31, h = lane >> 5;
        int64_t next_chunk = chunk + gridDim.x;
        int64_t row[NS], lrow[NS];
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            row[n] = chunk * ROWS_PER_BLOCK + wave * (32 * NS) + n * 32 + j;
            lrow[n] = row[n] < n_rows ? row[n] : n_rows - 1;      // clamp loads, mask stores
        }
        if (redo_pass) {
            // this wave's 32-row groups come from the list; a sample the fp16 x 3 pass did NOT name keeps that pass's results (its
            // row index is pushed beyond n_rows: loads clamp, stores and the sum skip it -- the ragged-tail machinery)
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                const uint32_t e = (uint32_t)chunk * (uint32_t)(WB * NS) + (uint32_t)(wave * NS + n);
                const bool have = e < redo_count;
                const uint32_t grp = have ? k.redo[2 + 2 * e] : 0u, msk = have ? k.redo[3 + 2 * e] : 0u;
                const int64_t r = (int64_t)grp * 32 + j;
                lrow[n] = r < n_rows ? r : n_rows - 1;
                row[n] = ((msk >> j) & 1u) && r < n_rows ? r : n_rows;
            }
        }

        // MODE 4 on 4 + 4 tiles: the row's dL/dlog_prob once per chunk (a load inside the step loop is waited for with vmcnt(0):
        // behind the weight DMA just issued and every factor store in flight), and whether this wave stores factors at all
        [[maybe_unused]] float gg_chunk = 0.f;
        [[maybe_unused]] bool stores_young = false;
        // the counted wait at the loop head is only sound when the SECOND half of the previous iteration issued >= 64 factor
        // stores behind its weight DMA: a dense layer's adjoint half stores 4 tiles (64), a coupling's step B 2 HT tiles (32 HT)
        [[maybe_unused]] bool head_counted = false;
        if constexpr (MODE == 4 && TX == 8 && NS == 1) {
            gg_chunk = k.row_t[lrow[0]];
            stores_young = k.side != nullptr && __builtin_amdgcn_readfirstlane((int)(row[0] - j < n_rows)) != 0;
        }
        // ---- load the state tiles in C-fragment order ---------------------------------------------------
        tile<NS> xs[TX];
        bool from_frag = false;
        [[maybe_unused]] float gg11 = 0.f;
        if constexpr (MODE == 11) {
            from_frag = k.frag_in != nullptr;
            // (a row's dL/dlog_prob travels with its prefetched state: an ordinary load inside the step would be waited for with
            //  vmcnt(0) -- behind the LDS-DMA just issued for the next chunk)
            gg11 = have_pf ? gg_next : k.row_t[lrow[0]];
            if (have_pf) {
                // this chunk's state was prefetched into the wave's landing zone during the previous chunk, and waited for at
                // the END of that chunk, before its stores: a wait here would sit behind those stores (in-order retirement).
                // First launch (z, row-major): the x tiles only; the adjoint tiles start at -g z as below.
                const f32x4 *fl = reinterpret_cast<const f32x4 *>(smem + pf_base + wave * 4096) + lane;
#pragma unroll
                for (int t = 0; t < TX; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (t < TX / 2 || from_frag) {
                            const f32x4 v = fl[(t * 4 + q) * 64];
                            xs[t].v[0][4 * q + 0] = v.x; xs[t].v[0][4 * q + 1] = v.y;
                            xs[t].v[0][4 * q + 2] = v.z; xs[t].v[0][4 * q + 3] = v.w;
                        } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c) xs[t].v[0][4 * q + c] = -gg11 * xs[t - TX / 2].v[0][4 * q + c];
                        }
                    }
                from_frag = true;            // (= the state is loaded: skip the row-major loads below)
            } else if (from_frag) {
                // fragment-order state of the previous launch: [32-row group][tile][q][lane] float4 (1 KB per instruction)
                const int64_t n_grp = (n_rows + 31) >> 5;
                int64_t grp = chunk * WB + wave;
                grp = grp < n_grp ? grp : n_grp - 1;
                const f32x4 *fi = reinterpret_cast<const f32x4 *>(k.frag_in) + grp * (TX * 4 * 64) + lane;
#pragma unroll
                for (int t = 0; t < TX; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = fi[(t * 4 + q) * 64];
                        xs[t].v[0][4 * q + 0] = v.x; xs[t].v[0][4 * q + 1] = v.y;
                        xs[t].v[0][4 * q + 2] = v.z; xs[t].v[0][4 * q + 3] = v.w;
                    }
            }
            have_pf = false;
        }
        // the ticket is requested behind the x loads and, like them, first waited for at step 0's vmcnt(0)
        // (built with the atomic optimizer off: its readfirstlane epilogue would wait right here)
        uint32_t ticket = 0;
        const auto take_ticket = [&]() { if (dyn && threadIdx.x == 0) ticket = atomicAdd(k.work, 1u); };
        if (x_flight) {
            // ONE FLIGHT: every piece of the chunk's rows goes out back to back -- no branch and no wait between them -- and is first
            // waited for behind the ticket request (bf16 pieces are widened there): one memory round trip per chunk where a load and
            // its conversion under `c + 3 < dim` made one per piece (eight dependent ones on the headline).  The row address is
            // formed once, for the storage type in use.  Bounds: lrow[] is clamped to [0, n_rows) and dim == 32 * TX, so the pieces
            // are exactly the bytes of one row of x -- the very bytes the loop below reads.
            if (X_AHEAD && have_xpre) {
                // (requested a chunk ago, and long since landed: the previous chunk's closing wait covers them)
#pragma unroll
                for (int n = 0; n < NS; ++n) x_flight_widen<TX>(xs, n, xpre[n]);
                ticket = ticket_pre;
            } else if (bf16) {
                u32x2 raw[NS][TX][4];
#pragma unroll
                for (int n = 0; n < NS; ++n) x_flight_issue<TX>(raw[n], reinterpret_cast<const uint16_t *>(k.x) + lrow[n] * dim, h);
                take_ticket();
#pragma unroll
                for (int n = 0; n < NS; ++n) x_flight_widen<TX>(xs, n, raw[n]);
            } else {
#pragma unroll
                for (int n = 0; n < NS; ++n) x_flight_issue<TX, MODE>(xs, n, reinterpret_cast<const float *>(k.x) + lrow[n] * dim, h);
                take_ticket();
            }
        } else {
        if (!from_frag)
#pragma unroll
        for (int n = 0; n < NS; ++n) {
#pragma unroll
            for (int t = 0; t < TX; ++t) {
                if (t < x_tiles) {
                    if (prog.identity_cols) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = 32 * t + 8 * q + 4 * h;
                            f32x4 v = {0.f, 0.f, 0.f, 0.f};
                            if (c + 3 < dim) {
                                if (bf16) {
                                    // (plain loads: a lane takes 8 B of a 128-B row per instruction, eight instructions share a line -- with
                                    //  the streaming policy the line was re-fetched between them: FETCH_SIZE 69 -> 164 MKiB per launch)
                                    const u16x4 u = *reinterpret_cast<const u16x4 *>(
                                        reinterpret_cast<const uint16_t *>(k.x) + lrow[n] * dim + c);
                                    v = f32x4{bf16_to_f32(u.x), bf16_to_f32(u.y), bf16_to_f32(u.z), bf16_to_f32(u.w)};
                                } else {
                                    // spline programs (96 steps, 3.2 MB of blobs that every chunk re-reads from L2): x is read once and
                                    // kept out of their way by the streaming policy (cfg 3: FETCH_SIZE 318 -> 154 MKiB per launch, same
                                    // time); elsewhere plain loads (cfg 4 measured 2 % slower with it)
                                    constexpr bool NT_X = MODE == 3 || MODE == 10 || MODE == 12 || MODE == 13 || MODE == 18 || MODE == 19;
                                    if constexpr (NT_X) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(k.x) + lrow[n] * dim + c));
                                    else v = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(k.x) + lrow[n] * dim + c);
                                }
                            }
                            xs[t].v[n][4 * q + 0] = v.x; xs[t].v[n][4 * q + 1] = v.y;
                            xs[t].v[n][4 * q + 2] = v.z; xs[t].v[n][4 * q + 3] = v.w;
                        }
                    } else {
                        // gathered columns (Flip / Permute relabelling, ragged widths): all 16 indices, then all 16 elements -- a
                        // load under `c >= 0` is a branch with its own s_waitcnt vmcnt(0), i.e. 32 dependent round trips per tile
                        int cidx[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) cidx[r] = k.in_col[32 * t + sx_kmap(r, h)];
                        const int64_t rb = lrow[n] * (prog.pad ? prog.pad : dim);      // prog.pad: row stride of x when the program reads a column subset of wider rows
                        if (bf16) {
                            uint16_t u[16];
#pragma unroll
                            for (int r = 0; r < 16; ++r) u[r] = reinterpret_cast<const uint16_t *>(k.x)[rb + (cidx[r] >= 0 ? cidx[r] : 0)];
#pragma unroll
                            for (int r = 0; r < 16; ++r) xs[t].v[n][r] = cidx[r] >= 0 ? bf16_to_f32(u[r]) : 0.f;
                        } else {
                            float u[16];
#pragma unroll
                            for (int r = 0; r < 16; ++r) u[r] = reinterpret_cast<const float *>(k.x)[rb + (cidx[r] >= 0 ? cidx[r] : 0)];
#pragma unroll
                            for (int r = 0; r < 16; ++r) xs[t].v[n][r] = cidx[r] >= 0 ? u[r] : 0.f;
                        }
                    }
                } else if constexpr (MODE == 4 || MODE == 11) {
                    // adjoint tiles: dL/dz of log p = -z^2/2 + ... is -g z (g = dL/dlog_prob of the row)
                    if constexpr (TX == 2 || TX == 4 || TX == 8) {
                        const float gg = k.row_t[lrow[n]];
#pragma unroll
                        for (int r = 0; r < 16; ++r) xs[t].v[n][r] = -gg * xs[t - TX / 2].v[n][r];
                    }
                } else {   // latent tiles (fp32), conditioner-only inputs (coupling.py:64-65)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = 32 * (t - x_tiles) + sx_kmap(r, h);
                        float v = (k.latent != nullptr && c < prog.latent_dim) ? k.latent[lrow[n] * prog.latent_dim + c] : 0.f;
                        if constexpr (MODE == 15 || MODE == 21) {      // the two slots behind the latent columns: t and t0 (coupling.py:155-156)
                            if (c == prog.latent_dim && k.row_t != nullptr) v = k.row_t[lrow[n]];
                            if (c == prog.latent_dim + 1 && k.side != nullptr) v = k.side[lrow[n]];
                        }
                        xs[t].v[n][r] = v;
                    }
                }
            }
        }

        take_ticket();
        }
        float ldj[NS];
#pragma unroll
        for (int n = 0; n < NS; ++n) ldj[n] = 0.f;
        float ldj_c = 0.f;
        rng_t rg;                                                    // fp16 x 3 operand range of this chunk's samples
        rg.bad = 0ull;
        rg.thr = k.redo != nullptr ? SX_REDO_ABOVE : SX_F16_MAX;
        tile<NS> hid[MODE == 1 ? HT : 1];
        constexpr bool LIN = MODE == 2 || MODE == 7 || MODE == 8;    // programs with dense linear layers
        tile<NS> hidp[(MODE == 9 || MODE == 14 || MODE == 16 || MODE == 17) ? HT : 1];   // MODE 9 / 14 / 16 / 17: hidden state kept between deep-conditioner steps
        // MODE 20: programs with hidden-chunk couplings (split masks: TX / 2 transformed tiles): their (log_scale, shift) accumulators.
        // (An own kernel instance: as part of MODE 9 the loop-carried tiles took its deep-conditioner programs from 54 to 205 spilled
        //  registers at 64 columns.)
        [[maybe_unused]] tile<NS> pacc[(MODE == 20 && TX >= 2 && TX <= 4) ? TX : 1];
        [[maybe_unused]] btile<1> bhp[(MODE == 20 && TX == 8) ? HT : 1];        // eight-tile programs: the coupling's hidden activations (B fragments)
        // MODE 18 / 19 = MODE 3 / 12 with the training forward's side outputs (tanh h per layer, the state each layer received):
        // their own instances, so that the inference kernels carry none of that code (it cost cfg 3 0.7 % when it shared MODE 3)
        constexpr bool SIDE_OUT = MODE == 18 || MODE == 19;
        constexpr bool CUB = MODE == 12 || MODE == 13 || MODE == 19;    // cubic-spline couplings (13: + deep conditioners)
        constexpr bool RQ = MODE == 3 || MODE == 10 || MODE == 18 || CUB;      // spline couplings (10: + deep conditioners)
        constexpr bool RQDEEP = MODE == 10 || MODE == 13;
        // MODE 14: MIXED programs -- affine couplings, spline couplings of either type, point-wise steps and element-wise affines
        // in one launch (the reference's flagship stack, test_normalizing_flow.py:13-35: affine coupling -> Flip -> Sigmoid ->
        // cubic-spline coupling -> Logit).  One wave per SIMD: both splines' group states and the coupling arms share the file.
        // MODE 16: the same with cubic splines as the only spline type (the reference's default, and its flagship stack): one group
        // state instead of two, two waves per SIMD up to 64 columns
        // MODE 17: the same with rational-quadratic splines only
        constexpr bool MIX = MODE == 14 || MODE == 16 || MODE == 17;
        constexpr bool MIXC = MODE == 16, MIXQ = MODE == 17;
        btile<1> rq_bh[(RQ || MIX) ? HT : 1];             // hidden B operands + group state
        std::conditional_t<(CUB || MIXC), cubic_elems, rqs_elems> rq_e;
        [[maybe_unused]] std::conditional_t<(MODE == 14), cubic_elems, int> rq_ec;     // MODE 14 keeps both kinds of group state
        [[maybe_unused]] bool rq_lean = true;             // mixed programs: the current rational-quadratic group runs the bounded-logit code

        for (int s = 0; s < n_steps; ++s) {
            // (1) this step's weights were issued one step ago (or in the prologue): wait for MY pieces, then
            //     the barrier makes every wave's pieces visible AND guarantees all waves left step s-1,
            //     i.e. nobody still reads buffer cur^1;
            // MODE 11 with resident weights and static chunks: after the first chunk a wave needs nothing from the others (weights
            // are read-only, landing zones private): no wait, no barrier -- the waves of a workgroup drift freely
            const bool free_run = MODE == 11 && resident && !dyn && iter > 0;
            if (!free_run) {
                if constexpr (MODE == 4 && TX == 8) {
                    // the weights (LDS-DMA issued one half-step ago) are OLDER than the >= 64 factor stores of that half-step:
                    // a counted wait leaves the stores in flight (vector-memory operations retire in order).  vmcnt cannot count
                    // beyond 63, so with fewer than 64 stores behind the DMA (hidden <= 32: step B stores 32) the wait is a full one
                    if (s > 0 && stores_young && head_counted) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                if (dyn && s == 0 && threadIdx.x == 0) slot[iter & 1] = ticket;
                __syncthreads();
                if (dyn && s == 0) next_chunk = (int64_t)gridDim.x + __builtin_amdgcn_readfirstlane(slot[iter & 1]);
            }
            const bool has_next_chunk = next_chunk < n_chunks;
            // (2) refill buffer cur^1 with the next step's weights (the DMA flies under this step's MFMAs)
            //     and fetch the next step's descriptor one step early.
            const dstep st = st_next;
            // this step's LDS read offsets are formed BEFORE the DMA goes out (the empty asm pins them there): in the variants that
            // keep lane-derived values in scratch, a reload behind the DMA is a vector-memory load whose s_waitcnt vmcnt(0)
            // waits for the DMA itself -- the refill then no longer flies under the step's arithmetic
            int wb_off = cur * buf_floats * 4 + lane * 16, cb_off = cur * buf_floats * 4 + (lane >> 5) * 64;
            asm volatile("" : "+v"(wb_off), "+v"(cb_off));
            // MODE 7 / 8 on four tiles (8-wave workgroups): the refill is the OLDER half's job, at the END of its step (below) -- the
            // older half wins the SIMD's issue arbitration, finishes a step at ~65 % of its duration and waits at the next barrier: the
            // refill then costs the younger half (the critical path) nothing
            constexpr bool DMA_LATE = (MODE == 7 || MODE == 8) && WB == 8;
            [[maybe_unused]] const uint32_t dma_off_now = dma_off, dma_floats_now = (s + 1 < n_steps || has_next_chunk) ? dma_floats : 0u;
            if constexpr (!DMA_LATE)
                if ((s + 1 < n_steps || has_next_chunk) && dma_floats && !resident)
                    stage_blob<WB>(k.blobs + dma_off, (cur ^ 1) * buf_floats, dma_floats);
            if constexpr (MODE == 11) {
                if (resident && s == 0 && k.frag_in != nullptr && has_next_chunk) {
                    const int64_t ngrp = next_chunk * WB + wave;
                    if (ngrp < ((n_rows + 31) >> 5)) {       // wave-uniform
                        // (MUBUF LDS-DMA: see stage_blob -- this prefetch is in flight for the whole chunk)
                        const int64_t ngrp_s = __builtin_amdgcn_readfirstlane((int)ngrp);
                        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(k.frag_in + ngrp_s * (TX * 4 * 64 * 4)), 0, TX * 4 * 1024, 0x00020000);
                        char *ldst = reinterpret_cast<char *>(smem + pf_base + __builtin_amdgcn_readfirstlane(wave) * 4096);
#pragma unroll
                        for (int i = 0; i < TX * 4; ++i)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void *)(ldst + i * 1024), 16, lane * 16, i * 1024, 0, 0);
                        const int64_t nrow = ngrp * 32 + (lane & 31);
                        gg_next = k.row_t[nrow < n_rows ? nrow : n_rows - 1];
                        have_pf = true;
                    }
                } else if (resident && s == 0 && k.frag_in == nullptr && has_next_chunk && dim == 32 * (TX / 2)) {
                    // first launch: the next chunk's rows of z (row-major, whole tiles) into the same landing order -- an LDS-DMA lane
                    // fetches from any address: lane (row j, half h) of piece (t, q) takes columns 32 t + 8 q + 4 h .. + 3 of its row
                    const int64_t ngrp = next_chunk * WB + wave;
                    if (ngrp < ((n_rows + 31) >> 5)) {       // wave-uniform
                        const int64_t nrow = ngrp * 32 + (lane & 31), nr = nrow < n_rows ? nrow : n_rows - 1;
                        const int64_t ngrp_s = __builtin_amdgcn_readfirstlane((int)ngrp);
                        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(reinterpret_cast<const float *>(k.x) + ngrp_s * 32 * dim), 0, 0x7fffffff, 0x00020000);
                        const int voff = ((int)(nr - ngrp_s * 32) * dim + 4 * (lane >> 5)) * 4;
                        char *ldst = reinterpret_cast<char *>(smem + pf_base + __builtin_amdgcn_readfirstlane(wave) * 4096);
#pragma unroll
                        for (int i = 0; i < (TX / 2) * 4; ++i)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void *)(ldst + i * 1024), 16, voff, ((i >> 2) * 32 + (i & 3) * 8) * 4, 0, 0);
                        gg_next = k.row_t[nr];
                        have_pf = true;
                    }
                }
            }
            const int nxt = (s + 1 < n_steps) ? s + 1 : 0, nxt2 = (nxt + 1 < n_steps) ? nxt + 1 : 0;
            st_next = load_step(prog, nxt);
            dma_off = prog.steps[nxt2].blob_off;
            dma_floats = prog.steps[nxt2].blob_floats;

            const wptr w = wptr{reinterpret_cast<const char *>(smem) + wb_off, reinterpret_cast<const char *>(smem) + cb_off};
            [[maybe_unused]] float st_cur_const = st.ldj_const;      // (a spline triple moves on to its next steps inside the iteration)
            if constexpr (MODE == 5 || MODE == 6) {
                // pure split-coupling programs (host: validate_and_convert): two straight-line arms, state in place
                if constexpr (TX >= 2) {
#ifdef SX_F16X3
                    if constexpr (TX == 2 && HT == 2) {        // one source, one transformed tile, hidden 33..64: the k16-step-grain schedule
                        if (st.c0 == 0) coupling_affine_ks<NS, 0, 1, MODE == 5>(xs, w, st, ldj, rg);
                        else coupling_affine_ks<NS, 1, 0, MODE == 5>(xs, w, st, ldj, rg);
                    } else
#endif
                    if (st.c0 == 0) coupling_affine<NS, TX, HT, 0, TX / 2, TX / 2, TX / 2, true, MODE == 5>(xs, w, st, ldj, rg);
                    else coupling_affine<NS, TX, HT, TX / 2, TX / 2, 0, TX / 2, true, MODE == 5>(xs, w, st, ldj, rg);
                }
            } else if constexpr (MODE == 11) {
#ifdef SX_F16X3
                if constexpr (TX == 4 && NS == 1 && HT <= 2) {
                    const float gg = gg11;
                    const bool live = row[0] < n_rows;
                    // one accumulator set: the host keeps a MODE 11 program to one step
                    if (st.c0 == 0) coupling_affine_bwd_acc<HT, 0, 1>(xs, w, gg, live, WA, sel, rg);
                    else coupling_affine_bwd_acc<HT, 1, 0>(xs, w, gg, live, WA, sel, rg);
                }
#endif
            } else if ((MODE == 7 || MODE == 8) && st.kind == SX_STEP_COUPLING_AFFINE) {
                // dense linear layers + pure split couplings (cfg 4): the same two arms instead of the general dispatch
                if constexpr (TX >= 2 && (MODE == 7 || MODE == 8)) {
#ifdef SX_F16X3
                    if constexpr (TX == 4 && HT <= 2) {        // two waves per SIMD: A fragments one tile ahead, vector work between the MFMAs
                        if (st.c0 == 0) coupling_affine_pf<NS, TX, HT, 0, TX / 2, TX / 2, TX / 2, MODE == 7>(xs, w, st, ldj, rg);
                        else coupling_affine_pf<NS, TX, HT, TX / 2, TX / 2, 0, TX / 2, MODE == 7>(xs, w, st, ldj, rg);
                    } else
#endif
                    if (st.c0 == 0) coupling_affine<NS, TX, HT, 0, TX / 2, TX / 2, TX / 2, true, MODE == 7>(xs, w, st, ldj, rg);
                    else coupling_affine<NS, TX, HT, TX / 2, TX / 2, 0, TX / 2, true, MODE == 7>(xs, w, st, ldj, rg);
                }
            } else if constexpr (MODE == 15) {
                // programs of time-conditioned affine couplings (ContinuousAffineCoupling / NeuralFlow)
                if (st.kind == SX_STEP_COUPLING_TIME) {
                    float tv[NS];
#pragma unroll
                    for (int n = 0; n < NS; ++n) tv[n] = ((st.mask >> 8) & 1u) ? k.side[lrow[n]] : k.row_t[lrow[n]];
                    if (st.tt == TX) coupling_time_dispatch<NS, TX, HT, TX>(xs, w, st, ldj, rg, tv);
                    else if constexpr (TX >= 2) {
                        if (st.tt == TX / 2) coupling_time_dispatch<NS, TX, HT, TX / 2>(xs, w, st, ldj, rg, tv);
                        else if constexpr (TX >= 4) { if (st.tt == TX / 4) coupling_time_dispatch<NS, TX, HT, TX / 4>(xs, w, st, ldj, rg, tv); }
                    }
                }
            } else if constexpr (MODE == 21) {
                // MODE 15's programs with time-dependent point-wise flows between the couplings (NeuralFlow over ContinuousAffineCoupling,
                // ContinuousTanh and ContinuousActivation layers): an instance of its own, MODE 15 carries none of this
                if constexpr (TX <= 4) {
                    float tv[NS];
                    if (st.kind == SX_STEP_COUPLING_TIME) {
#pragma unroll
                        for (int n = 0; n < NS; ++n) tv[n] = ((st.mask >> 8) & 1u) ? k.side[lrow[n]] : k.row_t[lrow[n]];
                        if (st.tt == TX) coupling_time_dispatch<NS, TX, HT, TX>(xs, w, st, ldj, rg, tv);
                        else if constexpr (TX >= 2) {
                            if (st.tt == TX / 2) coupling_time_dispatch<NS, TX, HT, TX / 2>(xs, w, st, ldj, rg, tv);
                            else if constexpr (TX >= 4) { if (st.tt == TX / 4) coupling_time_dispatch<NS, TX, HT, TX / 4>(xs, w, st, ldj, rg, tv); }
                        }
                    } else if (st.kind == SX_STEP_POINTWISE_TIME) {
#pragma unroll
                        for (int n = 0; n < NS; ++n) tv[n] = (st.mask & 1u) ? k.side[lrow[n]] : k.row_t[lrow[n]];
                        pointwise_time_step<NS, TX>(xs, w, st, x_tiles, tv);
                    }
                }
            } else if constexpr (MODE == 4 && TX == 8) {
                // training backward of 128-column flows: these three step kinds only (the general switch below would instantiate
                // every coupling variant on eight tiles)
                if constexpr (NS == 1) {
                    float *srow = row[0] < n_rows ? k.side + ((int64_t)st.tt * ((n_rows + 31) >> 5) + (row[0] >> 5)) * (k.side_width * 32) + (row[0] & 31) : nullptr;
                    auto swap_tiles = [&](int a, int b) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) { const float t_ = xs[a].v[0][r]; xs[a].v[0][r] = xs[b].v[0][r]; xs[b].v[0][r] = t_; }
                    };
                    // Both halves of a layer run inside ONE loop iteration (the host plans them back to back and the launcher checks
                    // it): the ring advance of the loop head in the middle of the arm.  As separate iterations, r and dL/d(ls, sh) of
                    // a coupling were loop-carried state (a `keep` array beside xs) that had to survive the dense-layer arm, and the
                    // adjoint half of a dense layer ran on swapped registers: each arm fits the register file on its own, the three
                    // together took 548 B of scratch per lane -- and every scratch reload is a vector-memory operation that waits,
                    // in order, behind all factor stores issued before it (1.5 of the kernel's 3.0 ms).
                    // the state's home at the head of every iteration is the VGPR file: without it the allocator gives the arms
                    // different homes for parts of xs and pays the difference in scratch (116 B; 433 registers and none with it)
#pragma unroll
                    for (int t = 0; t < TX; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(xs[t].v[0][r]));
                    dstep stb;
                    wptr wb_ = w;
                    float *srow_b = nullptr;
                    auto second_half = [&]() {
                        cur ^= 1;
                        ++s;
                        if (stores_young) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
                        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        // (the raw barrier: __syncthreads()'s fence drains the vector-memory counter while the compiler believes an
                        //  LDS-DMA to be in flight -- the one issued at the head of this iteration, waited for just above)
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_s_barrier();
                        stb = st_next;
                        if ((s + 1 < n_steps || has_next_chunk) && dma_floats) stage_blob<WB>(k.blobs + dma_off, (cur ^ 1) * buf_floats, dma_floats);
                        const int nb = (s + 1 < n_steps) ? s + 1 : 0, nb2 = (nb + 1 < n_steps) ? nb + 1 : 0;
                        st_next = load_step(prog, nb);
                        dma_off = prog.steps[nb2].blob_off;
                        dma_floats = prog.steps[nb2].blob_floats;
                        wb_ = make_wptr(cur * buf_floats, lane);
                        srow_b = row[0] < n_rows ? k.side + ((int64_t)stb.tt * ((n_rows + 31) >> 5) + (row[0] >> 5)) * (k.side_width * 32) + (row[0] & 31) : nullptr;
                    };
                    if (st.kind == SX_STEP_COUPLING_AFFINE_BWD_A) {
                        // a coupling whose conditioner sits in the high tiles (c0 = 2) swaps the halves of x and of the adjoint in
                        // registers (64 v_swap) before step A and back after step B
                        const float gg = gg_chunk;
                        const bool high = st.c0 != 0;
                        if (high) { swap_tiles(0, 2); swap_tiles(1, 3); swap_tiles(4, 6); swap_tiles(5, 7); }
                        tile<1> keep[HT + 4];
                        coupling_affine_bwd_a<4, HT, 0, 2, 2, 2>(xs, w, gg, srow, lane, rg, keep);
                        second_half();
                        coupling_affine_bwd_b<4, HT, 0, 2, 2, 2>(xs, wb_, srow_b, lane, rg, keep);
                        if (high) { swap_tiles(0, 2); swap_tiles(1, 3); swap_tiles(4, 6); swap_tiles(5, 7); }
                        head_counted = HT >= 2;
                    } else if (st.kind == SX_STEP_LINEAR_BWD) {
                        linear_bwd_half<4, 0>(xs, w, srow, 32 * st.t0, st.reverse != 0, lane, rg);          // x tiles: v = M u + b
                        second_half();
                        linear_bwd_half<4, 4>(xs, wb_, srow_b, 32 * stb.t0, stb.reverse != 0, lane, rg);    // adjoint tiles: W^T dL/du
                        head_counted = true;
                    }
                }
            } else
            switch (st.kind) {
                case SX_STEP_COUPLING_AFFINE:
                    if constexpr (RQ || MODE == 7 || MODE == 8 || TX == 8) break;   // pure spline programs carry no affine couplings (register budget; mixed: MODE 14); 7 / 8: handled above; 8 tiles: chunk steps only
                    if constexpr (TX >= 2) {
                        if (st.ct == TX / 2 && st.c0 == 0 && st.t0 == TX / 2) {          // cond = low tiles
                            coupling_affine_dispatch<NS, TX, HT, 0, TX / 2, TX / 2, TX / 2>(xs, w, st, ldj, rg);
                            break;
                        }
                        if (st.ct == TX / 2 && st.c0 == TX / 2 && st.t0 == 0) {          // cond = high tiles
                            coupling_affine_dispatch<NS, TX, HT, TX / 2, TX / 2, 0, TX / 2>(xs, w, st, ldj, rg);
                            break;
                        }
                    }
                    coupling_affine_dispatch<NS, TX, HT, 0, TX, 0, TX>(xs, w, st, ldj, rg);       // dense
                    break;
                case SX_STEP_AFFINE_CONST:
                    if constexpr (MODE != 7 && MODE != 8) affine_const<NS, TX>(xs, w, st, x_tiles, ldj);
                    break;
                case SX_STEP_MLP_HIDDEN:
                    if constexpr (MODE == 1) hidden_layer<NS, TX, HT, 0, TX, false>(xs, hid, w, 0, st.act, rg);
                    break;
                case SX_STEP_MLP_INPUT:
                    // a single Linear: the output tiles contract the program's INPUT (tiles <= h_tiles: checked by the launcher)
                    if constexpr (MODE == 1 && TX <= HT) {
#pragma unroll
                        for (int m = 0; m < HT; ++m) {
                            if (m < TX) hid[m] = xs[m];
                            else {
#pragma unroll
                                for (int n = 0; n < NS; ++n)
#pragma unroll
                                    for (int r = 0; r < 16; ++r) hid[m].v[n][r] = 0.f;
                            }
                        }
                    }
                    break;
                case SX_STEP_CPL_HIDDEN:
                    if constexpr (MIX && NS == 1) {
                        // mixed programs: the deep-conditioner steps serve affine couplings (fp32 tiles in hidp) and spline
                        // couplings (B-operand form in rq_bh) alike -- keep both forms
                        if constexpr (TX >= 2) {
                            if (st.ct == TX / 2 && st.c0 == 0) hidden_layer<1, TX, HT, 0, TX / 2, false>(xs, hidp, w, 0, st.act, rg);
                            else if (st.ct == TX / 2) hidden_layer<1, TX, HT, TX / 2, TX / 2, false>(xs, hidp, w, 0, st.act, rg);
                            else hidden_layer<1, TX, HT, 0, TX, false>(xs, hidp, w, 0, st.act, rg);
                        } else {
                            hidden_layer<1, TX, HT, 0, TX, false>(xs, hidp, w, 0, st.act, rg);
                        }
#pragma unroll
                        for (int m = 0; m < HT; ++m) rq_bh[m] = make_btile<1>(hidp[m], rg);
                        break;
                    }
                    if constexpr (RQDEEP && NS == 1) {
                        // spline couplings with deep conditioners: the activations wait for the next layer in split (B
                        // operand) form in rq_bh -- the array the phases use anyway: no extra registers
                        tile<1> hd[HT];
                        if constexpr (TX >= 2) {
                            if (st.ct == TX / 2 && st.c0 == 0) hidden_layer<1, TX, HT, 0, TX / 2, false>(xs, hd, w, 0, st.act, rg);
                            else if (st.ct == TX / 2) hidden_layer<1, TX, HT, TX / 2, TX / 2, false>(xs, hd, w, 0, st.act, rg);
                            else hidden_layer<1, TX, HT, 0, TX, false>(xs, hd, w, 0, st.act, rg);
                        } else {
                            hidden_layer<1, TX, HT, 0, TX, false>(xs, hd, w, 0, st.act, rg);
                        }
#pragma unroll
                        for (int m = 0; m < HT; ++m) rq_bh[m] = make_btile<1>(hd[m], rg);
                    }
                    if constexpr (MODE == 9) {
                        if constexpr (TX >= 2) {
                            if (st.ct == TX / 2 && st.c0 == 0) { hidden_layer<NS, TX, HT, 0, TX / 2, false>(xs, hidp, w, 0, st.act, rg); break; }
                            if (st.ct == TX / 2 && st.c0 == TX / 2) { hidden_layer<NS, TX, HT, TX / 2, TX / 2, false>(xs, hidp, w, 0, st.act, rg); break; }
                        }
                        hidden_layer<NS, TX, HT, 0, TX, false>(xs, hidp, w, 0, st.act, rg);
                    }
                    break;
                case SX_STEP_CPL_HIDDEN2:
                    if constexpr (MIX && NS == 1) {
                        tile<1> nh[HT];
                        hidden_body<1, HT, HT, false>(rq_bh, nh, w, 0, st.act);
#pragma unroll
                        for (int m = 0; m < HT; ++m) { hidp[m] = nh[m]; rq_bh[m] = make_btile<1>(nh[m], rg); }
                        break;
                    }
                    if constexpr (RQDEEP && NS == 1) {
                        tile<1> hd[HT];
                        hidden_body<1, HT, HT, false>(rq_bh, hd, w, 0, st.act);
#pragma unroll
                        for (int m = 0; m < HT; ++m) rq_bh[m] = make_btile<1>(hd[m], rg);
                    }
                    if constexpr (MODE == 9) {
                        tile<NS> nh[HT];
                        hidden_layer<NS, HT, HT, 0, HT, false>(hidp, nh, w, 0, st.act, rg);
#pragma unroll
                        for (int m = 0; m < HT; ++m) hidp[m] = nh[m];
                    }
                    break;
                case SX_STEP_COUPLING_AFFINE_DEEP:
                    if constexpr (MODE == 9 || MIX) {
                        if constexpr (TX >= 2) {
                            if (st.tt == TX / 2 && st.t0 == TX / 2) {
                                if (st.reverse) coupling_affine_deep<NS, TX, HT, TX / 2, TX / 2, true>(xs, hidp, w, st, ldj, rg);
                                else coupling_affine_deep<NS, TX, HT, TX / 2, TX / 2, false>(xs, hidp, w, st, ldj, rg);
                                break;
                            }
                            if (st.tt == TX / 2 && st.t0 == 0) {
                                if (st.reverse) coupling_affine_deep<NS, TX, HT, 0, TX / 2, true>(xs, hidp, w, st, ldj, rg);
                                else coupling_affine_deep<NS, TX, HT, 0, TX / 2, false>(xs, hidp, w, st, ldj, rg);
                                break;
                            }
                        }
                        if (st.reverse) coupling_affine_deep<NS, TX, HT, 0, TX, true>(xs, hidp, w, st, ldj, rg);
                        else coupling_affine_deep<NS, TX, HT, 0, TX, false>(xs, hidp, w, st, ldj, rg);
                    }
                    break;
                case SX_STEP_WIDE_HIDDEN:
                    if constexpr (MODE == 20 && TX == 8 && NS == 1) {
                        if (st.c0 == 0) wide_hidden<TX, HT, 0>(xs, bhp, w, rg);
                        else wide_hidden<TX, HT, TX / 2>(xs, bhp, w, rg);
                    }
                    break;
                case SX_STEP_WIDE_AFFINE_TILE:
                    if constexpr (MODE == 20 && TX == 8 && NS == 1) wide_affine_tile<TX, HT>(xs, bhp, w, st, ldj[0]);
                    break;
                case SX_STEP_COUPLING_AFFINE_HC:
                    if constexpr (MODE == 20 && TX >= 2 && TX <= 4) {
                        if (st.c0 == 0) coupling_affine_chunk_dispatch<NS, TX, HT, 0, TX / 2, TX / 2, TX / 2>(xs, pacc, w, st, ldj, rg);       // cond = low tiles
                        else coupling_affine_chunk_dispatch<NS, TX, HT, TX / 2, TX / 2, 0, TX / 2>(xs, pacc, w, st, ldj, rg);               // cond = high tiles
                    }
                    break;
                case SX_STEP_MLP_HIDDEN2:
                    if constexpr (MODE == 1) {
                        tile<NS> nh[HT];
                        hidden_layer<NS, HT, HT, 0, HT, false>(hid, nh, w, 0, st.act, rg);
#pragma unroll
                        for (int m = 0; m < HT; ++m) hid[m] = nh[m];
                    }
                    break;
                case SX_STEP_MLP_OUT_TILE:
                    if constexpr (MODE == 1) {
                        tile<NS> acc = load_cfrag<NS>(w.cb, HT * 1024);
                        [[maybe_unused]] float mxo = 0.f;
#pragma unroll
                        for (int c = 0; c < HT; ++c) gemm_tile<NS>(w.wb, c * 1024, make_btile_mx<NS>(hid[c], mxo), acc);
#ifdef SX_F16X3
                        rng_note(rg, mxo);      // hidden activations beyond fp16's range (run-time activations are unbounded): rng_note
#endif
                        const bool accumulate = st.reverse != 0;     // a later hidden chunk of a wide conditioner: mlp_out += (see add_mlp)
#ifdef SX_F16X3
                        if (rg.bad && k.redo == nullptr) {   // a row whose operands left the fp16 x 3 range is returned as NaN and flagged
                            if (rng_bad_sample(rg, lane)) {
#pragma unroll
                                for (int n = 0; n < NS; ++n)
#pragma unroll
                                    for (int r = 0; r < 16; ++r) acc.v[n][r] = __builtin_nanf("");
                                if (k.flags != nullptr) __hip_atomic_fetch_or(k.flags, SX_FLAG_F16_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            }
                        }
#endif
                        // (with a redo list the named samples' rows are left to the exact pass -- an ACCUMULATING launch must not add its
                        //  garbage to what the earlier chunks' exact passes left there; a sample is named before the first tile is stored:
                        //  its input in the first hidden step, its activations -- the same for every output tile -- right above)
                        [[maybe_unused]] bool skip_row = false;
#ifdef SX_F16X3
                        skip_row = k.redo != nullptr && rg.bad != 0ull && rng_bad_sample(rg, lane);
#endif
#pragma unroll
                        for (int n = 0; n < NS; ++n) {
                            if (row[n] < n_rows && !skip_row) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const int c = 32 * st.t0 + 8 * q + 4 * h;
                                    float *o = k.mlp_out + row[n] * k.mlp_out_stride + c;
                                    if (c + 3 < k.mlp_out_dim && (k.mlp_out_stride & 3) == 0) {
                                        f32x4 v = f32x4{acc.v[n][4 * q], acc.v[n][4 * q + 1], acc.v[n][4 * q + 2], acc.v[n][4 * q + 3]};
                                        if (accumulate) v += *reinterpret_cast<const f32x4 *>(o);
                                        *reinterpret_cast<f32x4 *>(o) = v;
                                    } else {
#pragma unroll
                                        for (int e = 0; e < 4; ++e)
                                            if (c + e < k.mlp_out_dim) o[e] = accumulate ? o[e] + acc.v[n][4 * q + e] : acc.v[n][4 * q + e];
                                    }
                                }
                            }
                        }
                    }
                    break;
                case SX_STEP_LINEAR_TILE:
                    // one 32-row slab of y = M . x + b (AffineLU affine.py:157,159-163; MatrixExponential
                    // affine.py:243-270 with the triangular solves folded into M on the host, in fp64)
                    // The whole layer is one step (its packed matrix always fits the LDS ring: <= 4 x 4 tiles): the
                    // state's fp16 hi/lo B operands are formed once and hold the complete old state, so every output
                    // slab is written straight over the state tile it replaces -- no second copy of the state.
                    if constexpr (LIN) {
#ifdef SX_F16X3
                        if (x_tiles == TX && TX >= 2) {
                            // full-width layers, K-MAJOR over TX live accumulators: the fp16 split of source tile c + 1 rides between the
                            // MFMAs of k-tile c (see coupling_affine_pf), so only the first tile's split is not covered; the A fragments
                            // of the next gemm tile are requested before the MFMAs of the current one go out (two register sets).
                            // (Known cost: the state has ONE home in the register file across the step loop, so the compiler copies it away
                            //  in front of the layer -- 32 v_mov_b64 -- and accumulates in place.  Handing the accumulators over inside the last
                            //  k-tile's MFMA shadows was tried two ways, a pinned assignment and an explicit v_mov_b64 per pair: the
                            //  allocator renames the first away and coalesces the second into a self-move; the copies stay where they are.)
                            tile<NS> acc[TX];
#pragma unroll
                            for (int m = 0; m < TX; ++m) acc[m] = load_cfrag<NS>(w.cb, TX * TX * 1024 + m * 32);
                            afr cura = afr_load(w.wb, 0);
                            float mx = 0.f;
                            btile<NS> bcur = make_btile_mx<NS>(xs[0], mx);
                            __builtin_amdgcn_sched_barrier(0);
                            u32x4 nhi[NS][2], nlo[NS][2];
                            constexpr int PPM = 8 / TX;            // split pairs of the next source tile per gemm tile (TX = 4: two)
#pragma unroll
                            for (int c = 0; c < TX; ++c) {
#pragma unroll
                                for (int m = 0; m < TX; ++m) {
                                    const int qn = c * TX + m + 1;                                     // next gemm tile in k-major order
                                    const int next_off = qn < TX * TX ? ((qn % TX) * TX + qn / TX) * 1024 : -1;
                                    gemm_tile_pf<NS>(w.wb, cura, next_off, bcur, acc[m], [&](int i) {
                                        if (c + 1 < TX) {
                                            // PPM pairs, each right behind an MFMA: units 0, 8 (PPM = 2) or 0, 3, 8, 11 (PPM = 4)
                                            if (PPM == 2) { if (i == 0 || i == 8) split_pair<NS, true>(xs[c + 1 < TX ? c + 1 : 0], nhi, nlo, PPM * m + (i >> 3), mx); }
                                            else { if (i == 0 || i == 3 || i == 8 || i == 11) split_pair<NS, true>(xs[c + 1 < TX ? c + 1 : 0], nhi, nlo, PPM * m + (i >> 3) * 2 + ((i & 7) != 0), mx); }
                                        }
                                    });
                                }
                                if (c + 1 < TX) bcur = btile_of<NS>(nhi, nlo);
                            }
                            rng_note(rg, mx);      // a sample's state beyond fp16's range: rng_note
#pragma unroll
                            for (int m = 0; m < TX; ++m) xs[m] = acc[m];
                        } else
#endif
                        {
                        btile<NS> bx[TX];
                        [[maybe_unused]] float mx = 0.f;
#pragma unroll
                        for (int c = 0; c < TX; ++c) bx[c] = make_btile_mx<NS>(xs[c], mx);
                        __builtin_amdgcn_sched_barrier(0);
                        rng_note(rg, mx);      // a sample's state beyond fp16's range: rng_note
#pragma unroll
                        for (int m = 0; m < TX; ++m) {
                            if (m < x_tiles) {
                                tile<NS> acc = load_cfrag<NS>(w.cb, x_tiles * TX * 1024 + m * 32);
#pragma unroll
                                for (int c = 0; c < TX; ++c) gemm_tile<NS>(w.wb, (m * TX + c) * 1024, bx[c], acc);
                                xs[m] = acc;
                            }
                        }
                        }
                        // the layer's (parameter-only) log-det rides in the blob behind the bias, so a parameter update
                        // refreshes it with the matrix (affine.py:171, 287-288)
                        ldj_c += smem[cur * buf_floats + x_tiles * TX * 1024 + x_tiles * 32];
                    }
                    break;
                case SX_STEP_COUPLING_AFFINE_BWD:
                    if constexpr (MODE == 4 && NS == 1 && (TX == 2 || TX == 4)) {
                        constexpr int XT = TX / 2;
                        const float gg = k.row_t[lrow[0]];
                        float *srow = row[0] < n_rows ? k.side + ((int64_t)st.tt * ((n_rows + 31) >> 5) + (row[0] >> 5)) * (k.side_width * 32) + (row[0] & 31) : nullptr;
                        if constexpr (XT == 2) {
                            if (st.ct == 1 && st.c0 == 0) coupling_affine_bwd<2, HT, 0, 1, 1, 1>(xs, w, gg, srow, lane, rg);
                            else if (st.ct == 1) coupling_affine_bwd<2, HT, 1, 1, 0, 1>(xs, w, gg, srow, lane, rg);
                            else coupling_affine_bwd<2, HT, 0, 2, 0, 2>(xs, w, gg, srow, lane, rg);
                        } else {
                            coupling_affine_bwd<1, HT, 0, 1, 0, 1>(xs, w, gg, srow, lane, rg);
                        }
                    }
                    break;
                case SX_STEP_POINTWISE:
                    if constexpr (MODE == 0 || MIX) pointwise_step<NS, TX>(xs, w, st, x_tiles, TX, ldj);
                    break;
                case SX_STEP_RQS_HIDDEN:
                    if constexpr ((RQ || MIX) && NS == 1) {
                        tile<1> hd[HT];
                        if ((RQDEEP || MIX) && st.pad == 1) {   // deep conditioner: the last hidden layer, from the previous one's activations
                            hidden_body<1, HT, HT, true>(rq_bh, hd, w, 0, st.act);
                        } else
                        if constexpr (TX >= 2) {
                            if (st.ct == TX / 2 && st.c0 == 0) hidden_layer<1, TX, HT, 0, TX / 2, true>(xs, hd, w, 0, st.act, rg);
                            else if (st.ct == TX / 2) hidden_layer<1, TX, HT, TX / 2, TX / 2, true>(xs, hd, w, 0, st.act, rg);
                            else hidden_layer<1, TX, HT, 0, TX, true>(xs, hd, w, 0, st.act, rg);
                        } else {
                            hidden_layer<1, TX, HT, 0, TX, true>(xs, hd, w, 0, st.act, rg);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) hd[HT - 1].v[0][r] = fast_sig2(hd[HT - 1].v[0][r]);
#pragma unroll
                        for (int m = 0; m < HT; ++m) rq_bh[m] = make_btile<1>(hd[m]);
                        // optional side output for the training backward (sx_rqs_slab_bwd keeps the conditioner's last hidden
                        // activation): tanh h = 1 - 2 r, row-major [n_rows, mlp_out_dim] -- instead of a library GEMM + tanh
                        // (bits 8..15 of the step's mask = the layer's ordinal among the program's spline couplings: a whole-flow program
                        //  leaves one [n_rows, H] block per layer, and -- `side` given -- the state each layer but the first received,
                        //  row-major [n_rows, dim] blocks: what the per-layer training backward needs from ONE forward launch)
                        // (the deep and mixed instances keep the h block they always had -- never requested there, sx_flow_run refuses
                        //  it, but their register allocation is fragile: MODE 16 ran 7 % slower without it)
                        if constexpr (SIDE_OUT || MIX || RQDEEP) {
                        const int slot = SIDE_OUT ? (int)((st.mask >> 8) & 0xffu) : 0;
                        if (SIDE_OUT && k.side != nullptr && slot > 0 && row[0] < n_rows) {
                            float *so = k.side + ((int64_t)(slot - 1) * n_rows + row[0]) * dim;
#pragma unroll
                            for (int t = 0; t < TX; ++t)
                                if (t < x_tiles) {
#pragma unroll
                                    for (int q = 0; q < 4; ++q) {
                                        const int c = 32 * t + 8 * q + 4 * h;
                                        const f32x4 sv = {xs[t].v[0][4 * q], xs[t].v[0][4 * q + 1], xs[t].v[0][4 * q + 2], xs[t].v[0][4 * q + 3]};
                                        if (c + 3 < dim && (dim & 3) == 0) *reinterpret_cast<f32x4 *>(so + c) = sv;
                                        else {
#pragma unroll
                                            for (int e = 0; e < 4; ++e)
                                                if (c + e < dim) so[c + e] = sv[e];
                                        }
                                    }
                                }
                        }
                        if (k.mlp_out != nullptr && row[0] < n_rows) {
#pragma unroll
                            for (int m = 0; m < HT; ++m)
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const int c = 32 * m + 8 * q + 4 * h;
                                    float *o = k.mlp_out + ((int64_t)slot * n_rows + row[0]) * k.mlp_out_stride + c;
                                    const f32x4 tv = {1.f - 2.f * hd[m].v[0][4 * q], 1.f - 2.f * hd[m].v[0][4 * q + 1],
                                                      1.f - 2.f * hd[m].v[0][4 * q + 2], 1.f - 2.f * hd[m].v[0][4 * q + 3]};
                                    if (c + 3 < k.mlp_out_dim && (k.mlp_out_stride & 3) == 0) *reinterpret_cast<f32x4 *>(o) = tv;
                                    else {
#pragma unroll
                                        for (int e = 0; e < 4; ++e)
                                            if (c + e < k.mlp_out_dim) o[e] = tv[e];
                                    }
                                }
                        }
                        }   // SIDE_OUT
                    }
                    break;
                case SX_STEP_RQS_PHASE:
                    if constexpr (MIXC && NS == 1) cubic_phase<TX, HT>(xs, rq_bh, rq_e, w, st, ldj[0], lane);
                    else if constexpr (MODE == 14 && NS == 1) {
                        if (st.act == 1) cubic_phase<TX, HT>(xs, rq_bh, rq_ec, w, st, ldj[0], lane);
                        else rqs_phase<TX, HT>(xs, rq_bh, rq_e, w, st, ldj[0], lane, rq_lean);
                    } else
                    if constexpr (MIXQ && NS == 1) rqs_phase<TX, HT>(xs, rq_bh, rq_e, w, st, ldj[0], lane, rq_lean);     // (the triple form below was tried here: 320 B of scratch instead of 128)
                    else if constexpr (RQ && NS == 1) {
                        // the group's three blocks in this one iteration (the host plans them back to back, the launcher checks it)
                        auto advance = [&](dstep &stn, wptr &wn) {
                            ldj_c += st_cur_const;
                            cur ^= 1;
                            ++s;
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            __builtin_amdgcn_s_barrier();
                            stn = st_next;
                            st_cur_const = stn.ldj_const;
                            int wb2 = cur * buf_floats * 4 + lane * 16, cb2 = cur * buf_floats * 4 + (lane >> 5) * 64;
                            asm volatile("" : "+v"(wb2), "+v"(cb2));
                            if ((s + 1 < n_steps || has_next_chunk) && dma_floats) stage_blob<WB>(k.blobs + dma_off, (cur ^ 1) * buf_floats, dma_floats);
                            const int nb = (s + 1 < n_steps) ? s + 1 : 0, nb2 = (nb + 1 < n_steps) ? nb + 1 : 0;
                            st_next = load_step(prog, nb);
                            dma_off = prog.steps[nb2].blob_off;
                            dma_floats = prog.steps[nb2].blob_floats;
                            wn = wptr{reinterpret_cast<const char *>(smem) + wb2, reinterpret_cast<const char *>(smem) + cb2};
                        };
                        if constexpr (CUB) cubic_triple<TX, HT>(xs, rq_bh, w, st, ldj[0], lane, advance);
                        else rqs_triple<TX, HT>(xs, rq_bh, w, st, ldj[0], lane, advance);
                    }
                    break;
                case SX_STEP_ROW_SCALE_EXP:
                    // x *= exp(+-diag * t_row)  (affine.py:263), t_row optionally log1p|t| (affine.py:239-240)
                    if constexpr (LIN) {
#pragma unroll
                        for (int n = 0; n < NS; ++n) {
                            float tr = k.row_t != nullptr ? k.row_t[lrow[n]] : st.ldj_const;
                            if (st.act) tr = log1pf(fabsf(tr));
                            const float sg = st.reverse ? -tr : tr;
                            float sd = 0.f;
#pragma unroll
                            for (int t = 0; t < TX; ++t) {
                                if (t < x_tiles) {
                                    const f32x16 dg = load_cfrag1(w.cb, t * 32);
#pragma unroll
                                    for (int r = 0; r < 16; ++r) {
                                        xs[t].v[n][r] *= fast_exp(dg[r] * sg);
                                        sd += dg[r];
                                    }
                                }
                            }
                            ldj[n] += st.ldj_scale * sd * tr;
                        }
                    }
                    break;
                default: break;
            }
            if constexpr (MODE == 21) { if (st.kind == SX_STEP_COUPLING_TIME) ldj_c += st_cur_const; }          // (SX_STEP_POINTWISE_TIME keeps its parameter there)
            else
            if (st.kind != SX_STEP_ROW_SCALE_EXP && st.kind != SX_STEP_POINTWISE) ldj_c += st_cur_const;      // (those two keep a parameter there)
            if constexpr (DMA_LATE) {
                // (buffer cur ^ 1 has been free since this step's barrier; the pieces land while the younger half finishes the step)
                if (dma_floats_now && __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) < WB / 2)
                    stage_blob<WB / 2>(k.blobs + dma_off_now, (cur ^ 1) * buf_floats, dma_floats_now);
            }
            if (!resident) cur ^= 1;
        }
        if constexpr (MODE == 11) {
            // E: the next chunk's state (LDS-DMA) and dL/dlog_prob were requested a whole step ago: waiting for them HERE, in
            // front of this chunk's stores, costs nothing; the stores then drain under the next chunk's arithmetic.  (The
            // "+v" operand makes the compiler's own wait for gg_next land here too, not behind the stores.)
            if (have_pf) asm volatile("s_waitcnt vmcnt(0)" : "+v"(gg_next) : : "memory");
        }

        // ---- epilogue: outputs -----------------------------------------------------------------------------
#ifdef SX_F16X3
        if constexpr (MODE != 1) {
            // a sample whose GEMM operands left the fp16 x 3 range (|v| > 65504) comes back as NaN, never as a
            // plausible number, and SX_FLAG_F16_RANGE is raised (the two lane halves hold one sample)
            if (rg.bad && k.redo != nullptr) {
                // the redo list (flow_kargs): the named samples are neither stored nor summed here -- the exact pass does both
                redo_push<NS>(k.redo, rg, lane, (uint32_t)chunk * (uint32_t)(WB * NS) + (uint32_t)(wave * NS));
                if (rng_bad_sample(rg, lane)) {
#pragma unroll
                    for (int n = 0; n < NS; ++n) row[n] = n_rows;
                }
            } else
            if (rg.bad) {
                if (rng_bad_sample(rg, lane)) {
#pragma unroll
                    for (int n = 0; n < NS; ++n) {
                        ldj[n] = __builtin_nanf("");
#pragma unroll
                        for (int t = 0; t < TX; ++t)
#pragma unroll
                            for (int r = 0; r < 16; ++r) xs[t].v[n][r] = __builtin_nanf("");
                    }
                    if (k.flags != nullptr) __hip_atomic_fetch_or(k.flags, SX_FLAG_F16_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        } else {
            // MLP programs store tile by tile inside the steps: with a redo list the exact pass rewrites the named samples' rows
            if (rg.bad && k.redo != nullptr) redo_push<NS>(k.redo, rg, lane, (uint32_t)chunk * (uint32_t)(WB * NS) + (uint32_t)(wave * NS));
        }
#endif
        if constexpr (X_AHEAD) {
            // the next chunk's rows, raw, and the ticket that goes with it: their round trip passes under this chunk's stores, row
            // reduction and sum instead of in front of the next chunk's first barrier, where all waves of the workgroup stood in it
            // together.  They stand BEHIND the range check above: in front of it the compiler parked the state tiles in other
            // registers behind an s_waitcnt vmcnt(0) of its own, i.e. waited for these loads right where they were issued.  (The
            // redo pass takes its rows from its list at the top.)  Bounds: next_chunk < n_chunks, so the chunk has a row; every
            // lane's row is clamped to [0, n_rows) as lrow[] is, and dim == 32 * TX: the pieces are the bytes of that row of x.
            have_xpre = x_flight && bf16 && !redo_pass && next_chunk < n_chunks;
#pragma unroll
            for (int n = 0; n < NS; ++n)
#pragma unroll
                for (int t = 0; t < TX; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q)      // (defined on every path, by no instruction)
                        asm volatile("" : "=v"(xpre[n][t][q].x), "=v"(xpre[n][t][q].y));
            ticket_pre = 0;
            if (have_xpre) {
                uint32_t tid_ = threadIdx.x;
                asm volatile("" : "+v"(tid_));
#pragma unroll
                for (int n = 0; n < NS; ++n) {
                    const int64_t r = next_chunk * ROWS_PER_BLOCK + (tid_ >> 6) * (32 * NS) + n * 32 + (tid_ & 31);
                    x_flight_issue<TX>(xpre[n], reinterpret_cast<const uint16_t *>(k.x) + (r < n_rows ? r : n_rows - 1) * dim, (tid_ >> 5) & 1);
                }
                if (dyn && threadIdx.x == 0) ticket_pre = atomicAdd(k.work, 1u);
            }
        }
        if constexpr (MODE == 11) {
            if (k.frag_out != nullptr && chunk * WB + wave < ((n_rows + 31) >> 5)) {
                f32x4 *fo = reinterpret_cast<f32x4 *>(k.frag_out) + (chunk * WB + wave) * (TX * 4 * 64) + lane;
#pragma unroll
                for (int t = 0; t < TX; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        fo[(t * 4 + q) * 64] = f32x4{xs[t].v[0][4 * q], xs[t].v[0][4 * q + 1], xs[t].v[0][4 * q + 2], xs[t].v[0][4 * q + 3]};
            }
        }
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            if (k.y != nullptr && row[n] < n_rows) {
#pragma unroll
                for (int t = 0; t < TX; ++t) {
                    if (t < x_tiles) {
                        const int ts = (MODE == 4 || MODE == 11) ? t + TX / 2 : t;      // backward: y receives dL/d(input)
                        if (prog.identity_cols) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int c = 32 * t + 8 * q + 4 * h;
                                if (c + 3 < dim) {
                                    const f32x16 &v = xs[ts].v[n];
                                    if (bf16) {
                                        u16x4 u{f32_to_bf16(v[4 * q]), f32_to_bf16(v[4 * q + 1]), f32_to_bf16(v[4 * q + 2]),
                                                f32_to_bf16(v[4 * q + 3])};
                                        *reinterpret_cast<u16x4 *>(reinterpret_cast<uint16_t *>(k.y) + row[n] * dim + c) = u;
                                    } else {
                                        *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(k.y) + row[n] * dim + c) =
                                            f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
                                    }
                                }
                            }
                        } else {
                            int cidx[16];                  // all indices first: one wait instead of one per element
#pragma unroll
                            for (int r = 0; r < 16; ++r) cidx[r] = k.out_col[32 * t + sx_kmap(r, h)];
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                if (cidx[r] >= 0) st_elem(k.y, row[n] * dim + cidx[r], xs[ts].v[n][r], bf16);
                        }
                    }
                }
            }
            if (k.ldj_out != nullptr || k.logp_out != nullptr || k.sum_out != nullptr) {
                float sq = 0.f;
                if (k.logp_out != nullptr) {
#pragma unroll
                    for (int t = 0; t < TX; ++t)
                        if (t < x_tiles) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) sq += xs[t].v[n][r] * xs[t].v[n][r];
                        }
                }
                const float part_lp = ldj[n] - 0.5f * sq;
                const float tot = part_lp + __shfl_xor(part_lp, 32, 64);   // the two lane halves of one sample
                const float ldj_tot = ldj[n] + __shfl_xor(ldj[n], 32, 64) + ldj_c;
                const float lp = tot + ldj_c - (float)dim * SX_HALF_LOG_2PI;
                if (row[n] < n_rows && h == 0) {
                    if (k.ldj_out != nullptr) k.ldj_out[row[n]] = ldj_tot;
                    if (k.logp_out != nullptr) k.logp_out[row[n]] = lp;
                    if constexpr (LDS_SUM) *lds_sum += (double)(k.logp_out != nullptr ? lp : ldj_tot);
                    else block_sum += (double)(k.logp_out != nullptr ? lp : ldj_tot);
                }
            }
        }
        chunk = next_chunk;
    }
    if (dyn && threadIdx.x == 0) {     // the last workgroup out re-arms the counters for the next launch on this stream
        __threadfence();
        if (atomicAdd(k.work + 1, 1u) == gridDim.x - 1) { k.work[0] = 0u; k.work[1] = 0u; }
    }
#ifdef SX_F16X3
    if constexpr (MODE == 11) {
        // one partial per workgroup and layer, in wgrad_reduce_kernel's layout: [64 x 32 HT | 64] then [32 HT x 32 | 32 HT];
        // the waves add their tiles in LDS by turns, then dW2 = (sum dp) 1^T - 2 sum dp r^T is applied and stored
        constexpr int N2 = 32 * HT, E2 = 64 * N2 + 64, E1 = 32 * HT * 32 + 32 * HT;
        const int i = lane & 31, kk = lane >> 5;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                    // nobody reads the weight ring any more
        float *red = smem;
        if (n_steps > 0) {
            const wacc<HT> &A = WA;
            for (int wv = 0; wv < WB; ++wv) {
                if (wave == wv) {
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
#pragma unroll
                        for (int m = 0; m < HT; ++m)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int e = (32 * p + (r & 3) + 8 * (r >> 2) + 4 * kk) * N2 + 32 * m + i;
                                red[e] = (wv == 0 ? 0.f : red[e]) + A.c2[p][m][r];
                            }
                        const float tb = A.b2[p] + __shfl_xor(A.b2[p], 32, 64);
                        if (kk == 0) { const int e = 64 * N2 + 32 * p + i; red[e] = (wv == 0 ? 0.f : red[e]) + tb; }
                    }
#pragma unroll
                    for (int m = 0; m < HT; ++m) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int e = E2 + (32 * m + (r & 3) + 8 * (r >> 2) + 4 * kk) * 32 + i;
                            red[e] = (wv == 0 ? 0.f : red[e]) + A.c1[m][r];
                        }
                        const float tb = A.b1[m] + __shfl_xor(A.b1[m], 32, 64);
                        if (kk == 0) { const int e = E2 + 32 * HT * 32 + 32 * m + i; red[e] = (wv == 0 ? 0.f : red[e]) + tb; }
                    }
                }
                __syncthreads();
            }
            // [gridDim.x][E2] then [gridDim.x][E1] (two inputs of wgrad_reduce_kernel)
            float *dst2 = k.acc_out + (int64_t)blockIdx.x * E2;
            float *dst1 = k.acc_out + (int64_t)gridDim.x * E2 + (int64_t)blockIdx.x * E1;
            for (int e = threadIdx.x; e < E2 + E1; e += 64 * WB) {
                float v = red[e];
                if (e < 64 * N2) v = red[64 * N2 + e / N2] - 2.f * v;          // tanh = 1 - 2 r
                if (e < E2) dst2[e] = v; else dst1[e - E2] = v;
            }
            __syncthreads();
        }
    }
#endif

    if (k.sum_out != nullptr) {
        double *part = reinterpret_cast<double *>(smem);   // no second __shared__ object beside the DMA ring
        if constexpr (LDS_SUM) block_sum = *lds_sum;
        block_sum = wave_sum_f64(block_sum);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (lane == 0) part[wave] = block_sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
#pragma unroll
            for (int i = 0; i < WB; i += 4) tot += (part[i] + part[i + 1]) + (part[i + 2] + part[i + 3]);
            atomicAdd(redo_pass && k.sum_slot != nullptr ? k.sum_slot : k.sum_out, tot);
        }
    }
    // (the redo pass reports AFTER its rows' sum has gone out: whoever reports last sees every total)
    if (redo_pass && threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(k.redo + 1, 1u) == gridDim.x - 1) {
            __threadfence();
            if (k.sum_slot != nullptr) redo_close_sum(k.sum_slot, k.sum_out);
            k.redo[0] = 0u; k.redo[1] = 0u;
        }
    }
}

// (a template so that the `if constexpr` around a MODE's launch is value-dependent: the discarded MODEs are never instantiated)
#ifndef SX_FAMILY
#define SX_FAMILY -1
#endif
template <int TX>
constexpr bool in_family(int f) { return SX_FAMILY < 0 || SX_FAMILY == f; }

template <int TX, int HT>
static int sx_flow_launch_impl(const sx_flow_args &a) {
    constexpr int NS = SX_NS_FOR(TX);
    int dev = 0;
    (void)hipGetDevice(&dev);
    flow_kargs k;
    k.blobs = a.blobs; k.x = a.x; k.latent = a.latent; k.in_col = a.in_col; k.out_col = a.out_col; k.y = a.y;
    k.ldj_out = a.ldj_out; k.logp_out = a.logp_out; k.sum_out = a.sum_out; k.mlp_out = a.mlp_out; k.row_t = a.row_t; k.side = a.side;
    k.mlp_out_stride = a.mlp_out_stride; k.n_rows = a.n_rows; k.mlp_out_dim = a.mlp_out_dim;
    k.buf_floats = a.buf_floats; k.bf16 = a.bf16; k.side_width = a.side_width; k.work = a.work; k.flags = a.flags;
    k.frag_in = a.frag_in; k.frag_out = a.frag_out; k.acc_out = a.acc_out;
    k.redo = a.redo; k.redo_pass = a.redo_pass; k.sum_slot = a.sum_slot;
#define SX_FL(MD)                                                                                              \
    do {                                                                                                       \
        auto kern = flow_fused_kernel<NS, TX, HT, MD>;                                                         \
        /* The attribute is set to what THIS launch needs, and only when that changes (per kernel variant and device): a    \
           blanket 160 KiB cost the spline slab backward a workgroup per CU (1.16 vs 0.92 ms); this kernel measures the   \
           same either way (0.334 ms on cfg 2), the exact value is simply never worse                                   */ \
        static int lds_set[64];                                                                                \
        if (a.lds > 48 * 1024 && lds_set[dev & 63] != a.lds) {                                                 \
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds); \
            if (e != hipSuccess) { sx_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; } \
            lds_set[dev & 63] = a.lds;                                                                         \
        }                                                                                                      \
        hipLaunchKernelGGL(kern, dim3(a.grid), dim3(64 * SX_BLOCK_WAVES(TX, MD)), a.lds, a.stream, a.prog, k);                         \
    } while (0)
#ifdef SX_ONLY_MODE      // resource / ISA studies of one variant (tools/rescheck.sh TX HT -DSX_ONLY_MODE=11): seconds instead of minutes
    if (a.mlp_mode == SX_ONLY_MODE) SX_FL(SX_ONLY_MODE);
    else { sx_set_error("built with SX_ONLY_MODE"); return SX_E_UNSUPPORTED; }
#else
    // SX_FM(MD): the MODE is instantiated in the object of its family only (-DSX_FAMILY: sx_flow_types.h; none: every MODE)
#define SX_FM(MD) do { if constexpr (in_family<TX>(SX_MODE_FAMILY(MD))) SX_FL(MD); else { sx_set_error("sx_flow_run: mode %d is not in this object's family", MD); return SX_E_UNSUPPORTED; } } while (0)
    if constexpr (TX == 8) {            // 4 data + 4 adjoint tiles: the training backward of 128-column flows; 8 data tiles: hidden-chunk programs
        if (a.mlp_mode == 4) { if constexpr (HT <= 2) SX_FM(4); else { sx_set_error("sx_flow_run: backward programs on 4 + 4 tiles are built for hidden <= 64"); return SX_E_UNSUPPORTED; } }
        else if (a.mlp_mode == 20) SX_FM(20);
        else { sx_set_error("sx_flow_run: 8 state tiles are the backward program's or a hidden-chunk program's (mode %d)", a.mlp_mode); return SX_E_UNSUPPORTED; }
    } else
    if (a.mlp_mode == 1) SX_FM(1); else if (a.mlp_mode == 2) SX_FM(2); else if (a.mlp_mode == 3) SX_FM(3);
    else if (a.mlp_mode == 4) SX_FM(4);
    else if (a.mlp_mode == 5) { if constexpr (TX >= 2) SX_FM(5); }
    else if (a.mlp_mode == 6) { if constexpr (TX >= 2) SX_FM(6); }
    else if (a.mlp_mode == 9) SX_FM(9);
    else if (a.mlp_mode == 10) SX_FM(10);
    else if (a.mlp_mode == 12) SX_FM(12);
    else if (a.mlp_mode == 18) SX_FM(18);
    else if (a.mlp_mode == 19) SX_FM(19);
    else if (a.mlp_mode == 13) SX_FM(13);
    else if (a.mlp_mode == 14) SX_FM(14);
    else if (a.mlp_mode == 15) SX_FM(15);
    else if (a.mlp_mode == 16) SX_FM(16);
    else if (a.mlp_mode == 17) SX_FM(17);
    else if (a.mlp_mode == 20) { if constexpr (TX >= 2) SX_FM(20); }
    else if (a.mlp_mode == SX_MODE_TIME_POINTWISE) SX_FM(SX_MODE_TIME_POINTWISE);
    else if (a.mlp_mode == 7) { if constexpr (TX >= 2) SX_FM(7); }
    else if (a.mlp_mode == 8) { if constexpr (TX >= 2) SX_FM(8); }
    else if (a.mlp_mode == 11) {
#ifdef SX_F16X3
        if constexpr (TX == 4 && HT <= 2) SX_FM(11); else
#endif
        { sx_set_error("sx_flow_bwd_run: needs 4 state tiles, hidden <= 64 and the fp16 x 3 arithmetic"); return SX_E_UNSUPPORTED; }
    }
    else SX_FM(0);
#undef SX_FM
#endif
#undef SX_FL
    SX_LAUNCH_CHECK();
    return SX_OK;
}

}  // namespace SX_PREC_NS
