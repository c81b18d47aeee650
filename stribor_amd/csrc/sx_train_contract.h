// The weight-gradient contraction of the one-launch training backward kernels (sx_cnf_train.hip, sx_resnet_bwd.hip,
// sx_equivariant.hip, sx_time_coupling_bwd.hip; included by nothing else).  A wave holds 32 rows on the MFMA column; dW = sum over those rows of X Y^T needs
// the rows on the K index of BOTH operands, so the two tiles turn through two per-wave LDS slots (feature-major, stride 33) and meet
// in v_mfma_f32_32x32x2_f32; a bias gradient is a row sum of the same slot.  A wave owns one partial; tc_reduce_kernel sums the
// partials in slot order, without atomics.  Operands are f32x16, float * and ints: nothing here knows a tile type, an LDS array or
// an argument struct.  Everything has internal linkage.
//
// THE FENCE RULE.  Slot traffic is ordered by wave fences, not barriers.  tc_outer fences on both sides.  tc_rowsum fences BEFORE
// its reads only: a caller that writes the SAME slot next must fence first (tc_add_rowsum does); one that writes the other slot and
// then calls tc_outer (sx_cnf_train.hip) is covered by tc_outer's opening fence.
#pragma once
#include "sx_common.h"

#define SX_TC_SLOT 1056                  /* one transposed tile: 32 features x (32 rows + 1) */
#define SX_TC_PRUNE_ROWS 1               /* tc_reduce_entry::prune */
#define SX_TC_PRUNE_COLS 2
// Loads whose address depends on nothing in the loop around them would all be lifted to its top and kept live: a compiler-only
// memory barrier per output tile keeps each tile's reads beside its MFMAs.
#define SX_NO_HOIST() asm volatile("" ::: "memory")

namespace {

// A loop-invariant address would be computed once, outside the loop, and kept: two registers per word.  One that passes through
// here is rebuilt where it is used.
template <class T>
__device__ __forceinline__ T *tc_here(T *p) {
    asm volatile("" : "+v"(p));
    return p;
}

// a tile into a slot, feature-major: slot[feature * 33 + row]
__device__ __forceinline__ void tc_put(float *slot, const f32x16 &x, int lane) {
    const int h = lane >> 5, n = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) slot[sx_kmap(r, h) * 33 + n] = x[r];
}

// acc[X feature kmap(r, h)][Y feature lane & 31] += sum over the wave's 32 rows of X Y^T, X in slot sa, Y in slot sb
__device__ __forceinline__ void tc_outer(f32x16 &acc, const float *sa, const float *sb, int lane) {
    const int o = (lane & 31) * 33 + (lane >> 5);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[o + 2 * kk], sb[o + 2 * kk], acc, 0, 0, 0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// feature lane & 31 of the tile in `slot` summed over rows 16 h .. 16 h + 15 (the two halves meet in the reduction).  No closing
// fence: see the rule above.
__device__ __forceinline__ float tc_rowsum(const float *slot, int lane) {
    const float *p = slot + (lane & 31) * 33 + 16 * (lane >> 5);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += p[i];
    return s;
}

// In-place accumulation into a wave's partial (dst: the lane's first word, register r at dst[r * 64]): the first group writes,
// later ones add, so nothing needs a zero-fill.  dst += (slot sA)(slot sB)^T ...
__device__ __forceinline__ void tc_add_tile(float *dst, const float *sA, const float *sB, bool first, int lane) {
    dst = tc_here(dst);
    f32x16 acc = {};
    if (!first) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = dst[r * 64];
    }
    tc_outer(acc, sA, sB, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[r * 64] = acc[r];
}

// ... and *dst += the row sum of `slot`.  Its callers loop straight into the next tc_put of the same slot: the closing fence.
__device__ __forceinline__ void tc_add_rowsum(float *dst, const float *slot, bool first, int lane) {
    const float sum = tc_rowsum(slot, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    dst = tc_here(dst);
    *dst = first ? sum : *dst + sum;
}

// float offset of element [X feature fx][Y feature fy] (both < 32) inside an accumulator tile as tc_outer's callers store it
__device__ __forceinline__ int tc_tile_off(int fx, int fy) { return ((fx & 3) + 4 * (fx >> 3)) * 64 + fy + 32 * ((fx >> 2) & 1); }

// A-fragment image of W^T (W row-major [out_dim, >= col0 + in_dim], row stride ld) at dst: MT x KT tiles (MT: W's INPUT tiles, KT:
// its output tiles); tile (m, c), float g*256 + lane*4 + j holds W[32c + kmap(4g + j, lane >> 5)][col0 + 32m + (lane & 31)]
__device__ __forceinline__ void tc_stage_t(float *dst, const float *__restrict__ W, int out_dim, int in_dim, int ld, int col0, int MT, int KT,
                                           int threads) {
    const int n_w = MT * KT * 1024;
    for (int e = threadIdx.x; e < n_w; e += threads) {
        const int tile = e >> 10, rem = e & 1023;
        const int g = rem >> 8, lane = (rem >> 2) & 63, j = rem & 3;
        const int m = tile / KT, c = tile - m * KT;
        const int col = 32 * m + (lane & 31), row = 32 * c + sx_kmap(4 * g + j, lane >> 5);
        dst[e] = (row < out_dim && col < in_dim) ? W[(int64_t)row * ld + col0 + col] : 0.f;
    }
}

// ---- the partial sum: one thread per gradient element, the slots in order ---------------------------------------------------------
// A template over the table's size, N <= 16: a file that includes this header and sums its partials otherwise gets no kernel.
// A kernel that contracted PRUNED operands (sx_time_coupling_bwd.hip) names the rows / columns it kept: element (fx, fy) of the
// gradient then sits at (its rank among the kept rows, its rank among the kept columns) of the partial, and an element of a row or
// column that was not kept is written as zero.
struct tc_reduce_entry {
    float *dst;                          // NULL: not wanted
    int rows, cols, kt, off;             // cols == 0: a vector of `rows` entries (64 floats per tile: the two row halves);
                                         // else a [rows, cols] matrix of kt column tiles per tile row; off: inside a partial
    int ld;                              // dst's row stride (a vector: its element stride); 0: dense
    int prune;                           // SX_TC_PRUNE_ROWS | SX_TC_PRUNE_COLS: keep_r / keep_c below name the kept ones
    uint64_t keep_r, keep_c;             // bit i: row / column i (< 64) was kept
};
template <int N>
struct tc_reduce_args {
    const float *partial;
    tc_reduce_entry e[N];                // in the order of the flat thread index; unused entries: rows == 0
    int n_slots, part_floats;
};

// index i -> its rank among the kept ones, or -1 when it was not kept
__device__ __forceinline__ int tc_rank(bool pruned, uint64_t keep, int i) {
    if (!pruned) return i;
    if (!((keep >> i) & 1)) return -1;
    return __popcll(keep & ((1ull << i) - 1));
}

template <int N>
__global__ void tc_reduce_kernel(const tc_reduce_args<N> a) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < N; ++k) {
        const tc_reduce_entry &t = a.e[k];
        const int n = t.cols ? t.rows * t.cols : t.rows;
        if (i >= n) { i -= n; continue; }
        if (t.dst == nullptr) return;
        int off, fx = i, fy = 0;
        if (t.cols) { fx = i / t.cols; fy = i - fx * t.cols; }
        float *dst = t.dst + (t.ld ? (int64_t)fx * t.ld + fy : (int64_t)i);
        fx = tc_rank(t.prune & SX_TC_PRUNE_ROWS, t.keep_r, fx);
        fy = tc_rank(t.prune & SX_TC_PRUNE_COLS, t.keep_c, fy);
        if (fx < 0 || fy < 0) { *dst = 0.f; return; }
        if (t.cols) off = t.off + ((fx >> 5) * t.kt + (fy >> 5)) * 1024 + tc_tile_off(fx & 31, fy & 31);
        else off = t.off + (fx >> 5) * 64 + (fx & 31);
        double s = 0.0;                 // up to 2048 slots in a row: the sum is carried in fp64 and rounded once
        const float *p = a.partial + off;
        for (int q = 0; q < a.n_slots; ++q, p += a.part_floats) s += t.cols ? (double)p[0] : (double)p[0] + (double)p[32];
        *dst = (float)s;
        return;
    }
}

// `total`: the entries' elements together.  fn: the entry point's name, for the message.
template <int N>
int tc_reduce(const char *fn, const tc_reduce_args<N> &r, int total, void *stream) {
    static_assert(N <= 16, "the table travels as a kernel argument");
    hipLaunchKernelGGL(tc_reduce_kernel<N>, dim3((total + 255) / 256), dim3(256), 0, sx_stream(stream), r);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { sx_set_error("%s: reduce launch failed: %s", fn, hipGetErrorString(err)); return (int)err; }
    return SX_OK;
}

}  // namespace
