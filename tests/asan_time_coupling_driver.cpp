// Host-side sanitizer driver of the time coupling's backward (test infrastructure; built by `make -C stribor_amd/csrc
// asan_time_coupling`, run by tests/test_time_coupling_train_host.py).  The recipe of tests/asan_driver.cpp: the library's HOST code
// compiled for the CPU only (hipcc --offload-host-only) with -fsanitize=address,undefined and driven WITHOUT a GPU -- every call below
// must come back with a status or a size, never crash, never trip a sanitizer report.  Driven: sx_time_coupling_bwd_lds_bytes and
// sx_time_coupling_bwd_partial_floats over the coverage edges and one step outside each, and every refusal of
// sx_time_coupling_bwd's validator: null and misaligned pointers, bad widths, codes, masks and row counts (each: a non-zero status and a
// message in sx_last_error()), and valid arguments with n_rows = 0 and no parameter gradient (status 0, nothing is launched).
#include "../include/stribor_hip.h"
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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
        if ((long long)(a) != (long long)(b)) { fprintf(stderr, "FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, (long long)(a), (long long)(b)); ++g_fail; } \
    } while (0)
#define EXPECT_TRUE(c)                                                                           \
    do {                                                                                         \
        ++g_calls;                                                                               \
        if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; }     \
    } while (0)

static float g_buf[8192];

// mask: bit c set = column c passes through
static sx_time_coupling_net make_net(int dim, int latent, int hidden, uint64_t mask, int kind, int half, int concat) {
    sx_time_coupling_net net;
    memset(&net, 0, sizeof net);
    net.W1 = g_buf; net.b1 = g_buf + 64; net.W2 = g_buf + 128; net.b2 = g_buf + 192;
    net.time_scale = kind == SX_TIME_IDENTITY ? nullptr : g_buf + 256;
    net.mask[0] = (uint32_t)mask; net.mask[1] = (uint32_t)(mask >> 32);
    net.dim = dim; net.latent_dim = latent; net.hidden = hidden; net.act = SX_ACT_TANH;
    net.time_kind = kind; net.time_half = half; net.concat_time = concat;
    return net;
}

int main() {
    // host memory stands in for device memory: no call below reaches a launch
    float *x = g_buf, *lat = g_buf + 512, *t = g_buf + 1024, *gy = g_buf + 1536, *gl = g_buf + 2048, *gx = g_buf + 2560, *glat = g_buf + 3072,
          *gt = g_buf + 3584, *part = g_buf + 4096;
    float *odd = (float *)((char *)g_buf + 2);
    const uint64_t low32 = 0xffffffffull, odd64 = 0xaaaaaaaaaaaaaaaaull;

    // ---- sx_time_coupling_bwd_lds_bytes: images (forward + transposed), vectors, maps, slots
    sx_time_coupling_net small = make_net(4, 0, 16, 0x3, SX_TIME_TANH, 4, 1);             // 2 inputs, 2 live: KT = HT = LT = 1
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&small), 4 * (2 * 1024 + 4 * 1024 + (32 + 32 + 64 + 32 + 32 + 32 + 64) + 8 * 1056));
    sx_time_coupling_net head = make_net(64, 0, 64, low32, SX_TIME_TANH, 64, 1);          // the README's layer: KT 1, HT 2, LT 1
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&head), 4 * (4 * 1024 + 8 * 1024 + (64 + 64 + 64 + 32 + 32 + 32 + 64) + 8 * 1056));
    sx_time_coupling_net none64 = make_net(64, 0, 64, 0, SX_TIME_IDENTITY, 1, 0);         // the largest plan: KT 1, HT 2, LT 2
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&none64), 4 * (4 * 1024 + 16 * 1024 + (64 + 64 + 128 + 64 + 64 + 32 + 128) + 8 * 1056));
    EXPECT_TRUE((long long)sx_time_coupling_bwd_lds_bytes(&none64) <= SX_CNF_LDS_BYTES);
    sx_time_coupling_net lat33 = make_net(31, 33, 40, odd64 & 0x7fffffffull, SX_TIME_LOG, 1, 1);      // 15 + 33 inputs: KT 2
    EXPECT_TRUE(sx_time_coupling_bwd_lds_bytes(&lat33) != 0);
    sx_time_coupling_net one = make_net(1, 2, 8, 0, SX_TIME_LINEAR, 1, 1);                // dim 1 under mask 'none'
    EXPECT_TRUE(sx_time_coupling_bwd_lds_bytes(&one) != 0);
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(nullptr), 0);
    sx_time_coupling_net bad = make_net(65, 0, 64, low32, SX_TIME_TANH, 65, 1);
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = make_net(32, 33, 64, 0xffff, SX_TIME_TANH, 32, 1);                                // dim + latent_dim = 65
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = make_net(64, 0, 65, low32, SX_TIME_TANH, 64, 1);
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.hidden = 0;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.dim = 0;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.latent_dim = -1;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.act = SX_ACT_SILU;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.act = -1;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.time_kind = SX_TIME_LOG + 1;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.time_kind = -1;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.time_half = 2;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = head; bad.concat_time = 2;
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = make_net(4, 0, 16, 0x13, SX_TIME_TANH, 4, 1);                                     // a mask bit beyond dim
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = make_net(4, 0, 16, 0xf, SX_TIME_TANH, 4, 1);                                      // no live column
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);
    bad = make_net(1, 0, 8, 0x1, SX_TIME_TANH, 1, 1);                                       // dim 1 under a mask that keeps it
    EXPECT_EQ(sx_time_coupling_bwd_lds_bytes(&bad), 0);

    // ---- sx_time_coupling_bwd_partial_floats: 4 waves x min(row blocks, 512) partials
    const long long per_wave = (2 + 4) * 1024 + (2 + 2 + 2 + 2) * 64;                    // head: dW1 2 tiles, dW2 4; db1, dW1's time column, db2, dtime
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&head, 0), 0);
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&head, -3), 0);
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(nullptr, 100), 0);
    bad = head; bad.hidden = 65;
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&bad, 100), 0);
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&head, 1), 4 * per_wave);
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&head, 128), 4 * per_wave);
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&head, 129), 8 * per_wave);
    EXPECT_EQ(sx_time_coupling_bwd_partial_floats(&head, (int64_t)1 << 40), 512 * 4 * per_wave);
    size_t prev = 0;
    for (int64_t n = 0; n < 70000; n += 95) {
        ++g_calls;
        const size_t now = sx_time_coupling_bwd_partial_floats(&head, n);
        if (now < prev) { fprintf(stderr, "FAIL sx_time_coupling_bwd_partial_floats is not monotone at %lld\n", (long long)n); ++g_fail; }
        prev = now;
    }

    // ---- the validator
    sx_time_coupling_grads gr;
    memset(&gr, 0, sizeof gr);
    EXPECT_OK(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 0, 0, 1.f, nullptr));
    EXPECT_OK(sx_time_coupling_bwd(&head, x, nullptr, t, gy, nullptr, gx, nullptr, nullptr, nullptr, &gr, 0, 1, -1.f, nullptr));
    EXPECT_OK(sx_time_coupling_bwd(&lat33, x, lat, t, nullptr, gl, gx, glat, gt, nullptr, &gr, 0, 1, 1.f, nullptr));
    EXPECT_OK(sx_time_coupling_bwd(&none64, x, nullptr, t, gy, gl, nullptr, nullptr, gt, nullptr, nullptr, 0, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(nullptr, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, nullptr, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, nullptr, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, nullptr, nullptr, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));   // no cotangent
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, nullptr, nullptr, nullptr, nullptr, nullptr, 5, 0, 1.f, nullptr));   // nothing to compute
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, nullptr, nullptr, nullptr, part, &gr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&lat33, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));            // the latent is missing
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, glat, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));                // glatent without a latent
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, -5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 2, 1.f, nullptr));             // reverse is 0 or 1
    EXPECT_BAD(sx_time_coupling_bwd(&head, odd, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&lat33, x, odd, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, odd, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, odd, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, odd, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, odd, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&lat33, x, lat, t, gy, gl, gx, odd, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, odd, nullptr, nullptr, 5, 0, 1.f, nullptr));
    EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, gt, odd, nullptr, 5, 0, 1.f, nullptr));
    float **slots[5] = {&gr.dW1, &gr.db1, &gr.dW2, &gr.db2, &gr.dtime};
    for (int k = 0; k < 5; ++k) {
        *slots[k] = part;
        EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, &gr, 5, 0, 1.f, nullptr));             // gradients without the partial buffer
        *slots[k] = odd;
        EXPECT_BAD(sx_time_coupling_bwd(&head, x, nullptr, t, gy, gl, gx, nullptr, gt, part, &gr, 5, 0, 1.f, nullptr));
        *slots[k] = nullptr;
    }
    gr.dtime = part;
    EXPECT_BAD(sx_time_coupling_bwd(&none64, x, nullptr, t, gy, gl, gx, nullptr, gt, part, &gr, 5, 0, 1.f, nullptr));                  // TimeIdentity has no parameter
    gr.dtime = nullptr;
    const float **params[5] = {&bad.W1, &bad.b1, &bad.W2, &bad.b2, &bad.time_scale};
    for (int k = 0; k < 5; ++k) {
        bad = head; *params[k] = nullptr;
        EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
        bad = head; *params[k] = odd;
        EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    }
    bad = make_net(65, 0, 64, low32, SX_TIME_TANH, 65, 1);
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = make_net(32, 33, 64, 0xffff, SX_TIME_TANH, 32, 1);
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, lat, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = head; bad.hidden = 65;
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = head; bad.act = SX_ACT_GELU;
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = head; bad.time_kind = 4;
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = head; bad.time_half = 32;
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = head; bad.concat_time = -1;
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = head; bad.mask[0] = 0xffffffffu; bad.mask[1] = 0xffffffffu;                       // no live column
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));
    bad = small; bad.mask[0] = 0x10;                                                        // a mask bit beyond dim
    EXPECT_BAD(sx_time_coupling_bwd(&bad, x, nullptr, t, gy, gl, gx, nullptr, gt, nullptr, nullptr, 5, 0, 1.f, nullptr));

    printf("asan_time_coupling_driver: %ld calls, %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
