// Host-side sanitizer driver of sx_cnf_exact_attn.hip's entry points (test infrastructure; built by `make -C stribor_amd/csrc
// asan_exact_attn`, run by tests/test_exact_attn_host.py).  The recipe of tests/asan_base_driver.cpp: the library's HOST code compiled for
// the CPU only (hipcc --offload-host-only) with -fsanitize=address,undefined and driven WITHOUT a GPU -- every call below must come back
// with a status, never crash, never trip a sanitizer report.  Driven: sx_cnf_exact_attn_lds_bytes and sx_cnf_exact_attn_flow with null
// pointers, every field one step out of range, an image_floats that does not match the plan, negative rows (each: 0 bytes / a non-zero
// status and a message in sx_last_error()), and valid arguments with n_rows = 0 (status 0, nothing is launched).
#include "../include/stribor_hip.h"
#include <stdint.h>
#include <stdio.h>

// No device code exists in this build: the registration entry points are taken over here (see tests/asan_driver.cpp).
extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *handle; return &handle; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipRegisterManagedVar(void *, void **, void *, const char *, size_t, unsigned) {}
}

static int g_fail = 0;
static long g_calls = 0;
#define EXPECT_BAD(call)                                                                         \
    do {                                                                                         \
        ++g_calls;                                                                               \
        int rc_ = (call);                                                                        \
        if (rc_ == 0) { fprintf(stderr, "FAIL %s:%d: accepted: %s\n", __FILE__, __LINE__, #call); ++g_fail; } \
        else if (!sx_last_error() || !sx_last_error()[0]) { fprintf(stderr, "FAIL %s:%d: no message: %s\n", __FILE__, __LINE__, #call); ++g_fail; } \
    } while (0)
#define EXPECT_OK(call)                                                                          \
    do {                                                                                         \
        ++g_calls;                                                                               \
        int rc_ = (call);                                                                        \
        if (rc_ != 0) { fprintf(stderr, "FAIL %s:%d: rc %d (%s): %s\n", __FILE__, __LINE__, rc_, sx_last_error(), #call); ++g_fail; } \
    } while (0)
#define EXPECT_EQ(a, b)                                                                          \
    do {                                                                                         \
        ++g_calls;                                                                               \
        if ((a) != (b)) { fprintf(stderr, "FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, (long long)(a), (long long)(b)); ++g_fail; } \
    } while (0)

static const int EXCHANGE = 2 * 128 * 36 + 128;
alignas(16) static float g_image[4], g_x[64], g_y[64], g_ldj[64], g_lat[64 * 64], g_wlat[64 * 64];

// a network inside the coverage: dim 3, [16, 8], d_h 3, sets of 4, 2 heads; image_floats from the library's own plan
static sx_cnf_exact_attn_net valid() {
    sx_cnf_exact_attn_net n = {};
    n.image = g_image;
    n.dim = 3; n.d_h = 3; n.latent_dim = 0; n.n_hidden = 2; n.hidden[0] = 16; n.hidden[1] = 8; n.act = SX_ACT_TANH; n.set_size = 4; n.n_heads = 2;
    n.image_floats = (int32_t)(sx_cnf_exact_attn_lds_bytes(&n) / 4) - EXCHANGE;
    return n;
}

static int flow(const sx_cnf_exact_attn_net *n, int64_t rows = 0, int solver = SX_CNF_RK4, int steps = 4, float step = 0.25f, const float *x = g_x,
                float *y = g_y, float *ldj = g_ldj, const float *lat = nullptr, int want = 1) {
    return sx_cnf_exact_attn_flow(n, x, lat, y, ldj, rows, solver, steps, 0.f, 1.f, step, want, nullptr);
}

int main() {
    // host memory stands in for device memory: no call below reaches a launch
    EXPECT_EQ(sx_cnf_exact_attn_lds_bytes(nullptr), 0);
    EXPECT_BAD(sx_cnf_exact_attn_flow(nullptr, g_x, nullptr, g_y, g_ldj, 0, SX_CNF_RK4, 4, 0.f, 1.f, 0.25f, 1, nullptr));
    sx_cnf_exact_attn_net n = valid();
    // [16, 8], dim 3, d_h 3: q 1056 + 1056, K and V 2 x 2112, proj 1056, dimwise 2240
    EXPECT_EQ(n.image_floats, 2112 + 4224 + 1056 + 2240);
    EXPECT_OK(flow(&n));
    EXPECT_OK(flow(&n, 0, SX_CNF_EULER, 1, 0.f));
    EXPECT_OK(flow(&n, 0, SX_CNF_RK4, 4, 0.25f, g_x, g_y, nullptr, nullptr, 0));

    // ---- the sizes at the mandated shapes and the largest image
    {
        sx_cnf_exact_attn_net m = valid();
        m.dim = 2; m.d_h = 8; m.hidden[0] = 64; m.hidden[1] = 32; m.set_size = 128; m.n_heads = 4;
        EXPECT_EQ(sx_cnf_exact_attn_lds_bytes(&m), (size_t)4 * (22208 + EXCHANGE));
        m.dim = 8; m.hidden[0] = 32; m.hidden[1] = 16;
        EXPECT_EQ(sx_cnf_exact_attn_lds_bytes(&m), (size_t)4 * (12800 + EXCHANGE));
        m.hidden[0] = 64;
        EXPECT_EQ(sx_cnf_exact_attn_lds_bytes(&m), (size_t)4 * (26368 + EXCHANGE));
        m.dim = 4; m.hidden[1] = 32;
        EXPECT_EQ(sx_cnf_exact_attn_lds_bytes(&m), (size_t)4 * (26368 + EXCHANGE));
    }

    // ---- every field one step out of range: no bytes, and the flow call declines with a message
#define OUTSIDE(stmt)                                             \
    do {                                                          \
        sx_cnf_exact_attn_net m = valid();                        \
        stmt;                                                     \
        EXPECT_EQ(sx_cnf_exact_attn_lds_bytes(&m), 0);            \
        EXPECT_BAD(flow(&m));                                     \
        EXPECT_BAD(flow(&m, 4));                                  \
    } while (0)
    OUTSIDE(m.dim = 0);
    OUTSIDE(m.dim = SX_CNF_EXACT_ATTN_MAX_DIM + 1);
    OUTSIDE(m.d_h = 0);
    OUTSIDE(m.d_h = SX_CNF_EXACT_ATTN_MAX_DH + 1);
    OUTSIDE(m.latent_dim = -1);
    OUTSIDE(m.latent_dim = SX_CNF_EXACT_ATTN_MAX_LATENT + 1);
    OUTSIDE(m.n_hidden = 0);
    OUTSIDE(m.n_hidden = 3);
    OUTSIDE(m.n_hidden = -1);
    OUTSIDE(m.hidden[0] = 0);
    OUTSIDE(m.hidden[0] = SX_CNF_EXACT_ATTN_MAX_HIDDEN + 1);
    OUTSIDE(m.hidden[1] = 0);
    OUTSIDE(m.hidden[1] = SX_CNF_EXACT_ATTN_MAX_EMBED + 1);
    OUTSIDE(m.n_hidden = 1; m.hidden[0] = SX_CNF_EXACT_ATTN_MAX_EMBED + 1);
    OUTSIDE(m.act = -1);
    OUTSIDE(m.act = SX_ACT_LEAKYRELU + 1);
    OUTSIDE(m.set_size = 0);
    OUTSIDE(m.set_size = SX_CNF_EXACT_ATTN_MAX_SIZE + 1);
    OUTSIDE(m.n_heads = 0);
    OUTSIDE(m.n_heads = 3);
    OUTSIDE(m.n_heads = 8);
    OUTSIDE(m.hidden[1] = 6; m.n_heads = 4);                      // heads that do not divide the embedding
    OUTSIDE(m.dim = 5; m.hidden[1] = 32);                         // five query tiles (E * dim = 160)
    OUTSIDE(m.dim = 8; m.hidden[1] = 17);                         // E * dim = 136
    OUTSIDE(m.dim = 5; m.hidden[1] = 17);                         // E * dim = 85, but five query tiles of one dimension each

    // ---- the image against the plan, the pointers, the per-call arguments
    { sx_cnf_exact_attn_net m = valid(); m.image_floats += 4; EXPECT_BAD(flow(&m)); EXPECT_BAD(flow(&m, 4)); }
    { sx_cnf_exact_attn_net m = valid(); m.image_floats -= 4; EXPECT_BAD(flow(&m)); }
    { sx_cnf_exact_attn_net m = valid(); m.image_floats = 0; EXPECT_BAD(flow(&m)); }
    { sx_cnf_exact_attn_net m = valid(); m.image_floats = -1; EXPECT_BAD(flow(&m)); }
    { sx_cnf_exact_attn_net m = valid(); m.image = nullptr; EXPECT_BAD(flow(&m)); }
    { sx_cnf_exact_attn_net m = valid(); m.image = g_image + 1; EXPECT_BAD(flow(&m)); }                    // not 16-byte aligned
    { sx_cnf_exact_attn_net m = valid(); m.latent_dim = 3; EXPECT_BAD(flow(&m)); }                         // latent rows and weights missing
    { sx_cnf_exact_attn_net m = valid(); m.latent_dim = 3; m.w_latent = g_wlat; EXPECT_BAD(flow(&m)); }    // latent rows missing
    { sx_cnf_exact_attn_net m = valid(); m.latent_dim = 3; EXPECT_BAD(flow(&m, 0, SX_CNF_RK4, 4, 0.25f, g_x, g_y, g_ldj, g_lat)); }
    { sx_cnf_exact_attn_net m = valid(); m.latent_dim = 3; m.w_latent = g_wlat + 1; EXPECT_BAD(flow(&m, 0, SX_CNF_RK4, 4, 0.25f, g_x, g_y, g_ldj, g_lat)); }
    { sx_cnf_exact_attn_net m = valid(); m.latent_dim = 3; m.w_latent = g_wlat; EXPECT_OK(flow(&m, 0, SX_CNF_RK4, 4, 0.25f, g_x, g_y, g_ldj, g_lat)); }
    EXPECT_BAD(flow(&n, -4));
    EXPECT_BAD(flow(&n, -1));
    EXPECT_BAD(flow(&n, 3));                                      // not a multiple of the set size
    EXPECT_BAD(flow(&n, 0, -1));
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4 + 1));
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4, -1));
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4, 4, 0.f));                  // a grid of several steps without a step size
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4, 4, -0.25f));
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4, 4, 0.25f, nullptr));
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4, 4, 0.25f, g_x, nullptr));
    EXPECT_BAD(flow(&n, 0, SX_CNF_RK4, 4, 0.25f, g_x, g_y, nullptr, nullptr, 1));      // want_ldj without ldj

    printf("asan_exact_attn_driver: %ld calls, %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
