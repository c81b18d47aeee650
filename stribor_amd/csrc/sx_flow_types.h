// Types shared by the fused-flow host dispatcher and its per-(tiles, hidden-tiles) kernel objects.
#pragma once
#include "sx_common.h"

// compact device-side copy of sx_step / sx_program (kernarg)
struct dstep {
    uint8_t kind, c0, ct, t0, tt, reverse, act, pad;
    uint32_t blob_off, blob_floats;
    float ldj_scale, ldj_const;
    uint32_t mask;      // RQS phases: live slots of the transformed tile
};
struct dprog {
    int32_t n_steps, dim, latent_dim, x_tiles, identity_cols, pad;
    dstep steps[SX_MAX_STEPS];
};


struct sx_flow_args {
    dprog prog;
    const float *blobs; const void *x; const float *latent; const int32_t *in_col; const int32_t *out_col;
    void *y; float *ldj_out; float *logp_out; double *sum_out; float *mlp_out; int64_t mlp_out_stride;
    int mlp_out_dim; int64_t n_rows; int buf_floats; int bf16; int mlp_mode; int grid; int lds; hipStream_t stream;
    const float *row_t;
    float *side;
    int side_width;
    uint32_t *work;
    uint32_t *flags;
    const float *frag_in;
    float *frag_out;
    float *acc_out;
    uint32_t *redo;         // sx_flow_run2: the redo list (sx_flow_kernel.h, flow_kargs), or NULL
    int redo_pass;          // 1: this launch is the exact pass over the listed groups
    double *sum_slot;       // sx_flow_run3: the redo pass's sum slot (sx_flow_kernel.h, flow_kargs), or NULL
};


// Layers per launch of the training backward with in-kernel weight-gradient contraction (MODE 11): every layer keeps
// 6 accumulator tiles (96 registers) alive over the whole launch.  With 2 the kernel needs 553 registers (984 B of
// scratch per lane on top of the 512-register file); with 1 it fits (457, no scratch).
#define SX_BWD_SLOTS 1

// sample tiles (of 32 rows) per wave (measured on cfg 2, MI355X: 2 sample tiles per wave buy nothing over 1 at 2 workgroups per
// CU -- 1.87e9 rows/s either way -- and cost registers)
#define SX_NS_FOR(TX) 1

// waves per SIMD the kernel is compiled for (= workgroups per CU): the D = 128 state (+ a second copy for the
// dense linear layers) needs the whole 512-register file; D <= 64 coupling flows run 3 per SIMD (168 VGPRs; measured
// +7 % over 2 on cfg 2: the third wave fills issue slots the other two leave at s_waitcnt / barriers)
#define SX_RQS_WAVES 2
// MODE 18 / 19: MODE 3 / 12 with the training forward's side outputs (same occupancy)
#define SX_MODE_BASE(MODE) ((MODE) == 18 ? 3 : ((MODE) == 19 ? 12 : (MODE)))
// waves per SIMD of the 128-column linear / split-coupling kernels (MODE 7 / 8 on four tiles): one workgroup of 4 x this per CU
#define SX_M7_WAVES 2
#define SX_WAVES_FOR(TX, MODE) SX_WAVES_FOR_(TX, SX_MODE_BASE(MODE))
#define SX_WAVES_FOR_(TX, MODE) ((MODE) == 11 || (MODE) == 14 ? 1 : (MODE) == 20 ? ((TX) >= 4 ? 1 : 2) : ((MODE) == 15 || (MODE) == 16 || (MODE) == 17 || (MODE) == 21) ? ((TX) >= 4 ? 1 : 2) : ((MODE) == 10 || (MODE) == 12 || (MODE) == 13) ? ((TX) >= 4 ? 1 : SX_RQS_WAVES) : (MODE) == 9 ? ((TX) >= 4 ? 1 : 2) : (MODE) >= 7 ? ((TX) >= 4 ? SX_M7_WAVES : 2) : (MODE) >= 5 ? ((TX) >= 4 ? 2 : 4) : ((TX) >= 4 ? 1 : ((MODE) == 3 ? SX_RQS_WAVES : ((MODE) == 0 ? 3 : 2))))

// waves per workgroup: the pure split-coupling kernels (MODE 5 / 6) run 8-wave workgroups -- D <= 64 (128 VGPRs): two
// per CU = 4 waves per SIMD sharing two weight rings; D = 128 (216 VGPRs): one per CU = 2 waves per SIMD on one ring
#define SX_BLOCK_WAVES(TX, MODE) ((((MODE) == 7 || (MODE) == 8) && (TX) >= 4) ? 4 * SX_M7_WAVES : ((MODE) == 5 || (MODE) == 6) ? 8 : 4)
// workgroups per CU the kernel is compiled for
#define SX_BLOCKS_FOR(TX, MODE) (SX_WAVES_FOR(TX, MODE) * 4 / SX_BLOCK_WAVES(TX, MODE))

// Kernel-MODE families, one object per (tiles, hidden tiles, arithmetic, family) -- VERDICT r4 #8c: every object used to instantiate
// all twenty MODEs of its pair, so a one-line spline edit rebuilt everything:
//   0  affine / dense / MLP / time-conditioned inference programs (MODE 0, 1, 2, 5 .. 9, 15, 20)
//   1  spline, cubic-spline and mixed programs (MODE 3, 10, 12, 13, 14, 16 .. 19): the only objects that instantiate sx_flow_spline.h
//   2  training backward programs (MODE 4, 11): the only objects that instantiate sx_flow_bwd.h
//   3  time-conditioned programs that hold SX_STEP_POINTWISE_TIME steps (MODE 21 = MODE 15 + that step; up to four tiles): objects of
//      their own, so that MODE 15's code object is what it was
#define SX_MODE_TIME_POINTWISE 21
#define SX_MODE_FAMILY(MODE) ((MODE) == 21 ? 3 : (MODE) == 4 || (MODE) == 11 ? 2 : ((MODE) == 3 || (MODE) == 10 || (MODE) == 12 || (MODE) == 13 || (MODE) == 14 || ((MODE) >= 16 && (MODE) <= 19)) ? 1 : 0)
#define SX_DECL_FLOW_F(T, H, F) int sx_flow_launch_f16x3_t##T##h##H##_f##F(const sx_flow_args &a); int sx_flow_launch_f32x_t##T##h##H##_f##F(const sx_flow_args &a);
#define SX_DECL_FLOW(T, H) SX_DECL_FLOW_F(T, H, 0) SX_DECL_FLOW_F(T, H, 1) SX_DECL_FLOW_F(T, H, 2)
SX_DECL_FLOW(1, 1) SX_DECL_FLOW(1, 2) SX_DECL_FLOW(1, 4)
SX_DECL_FLOW(2, 1) SX_DECL_FLOW(2, 2) SX_DECL_FLOW(2, 4)
SX_DECL_FLOW(4, 1) SX_DECL_FLOW(4, 2) SX_DECL_FLOW(4, 4)
SX_DECL_FLOW(8, 1) SX_DECL_FLOW(8, 2) SX_DECL_FLOW(8, 4)      // 4 data + 4 adjoint tiles: backward programs of 128-column flows (MODE 4); 8 data tiles: MODE 20
SX_DECL_FLOW_F(1, 1, 3) SX_DECL_FLOW_F(1, 2, 3) SX_DECL_FLOW_F(1, 4, 3) SX_DECL_FLOW_F(2, 1, 3) SX_DECL_FLOW_F(2, 2, 3) SX_DECL_FLOW_F(2, 4, 3)
SX_DECL_FLOW_F(4, 1, 3) SX_DECL_FLOW_F(4, 2, 3) SX_DECL_FLOW_F(4, 4, 3)
#undef SX_DECL_FLOW
#undef SX_DECL_FLOW_F
