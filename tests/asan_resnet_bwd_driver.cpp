// Host-side sanitizer driver of the ResNet-flow backward (test infrastructure; built by `make -C stribor_amd/csrc asan_resnet_bwd`,
// run by tests/test_iresnet_train_host.py).  The recipe of tests/asan_driver.cpp: the library's HOST code compiled for the CPU only
// (hipcc --offload-host-only) with -fsanitize=address,undefined and driven WITHOUT a GPU -- every call below must come back with a
// status or a size, never crash, never trip a sanitizer report.  Driven: sx_resnet_bwd_lds_bytes and sx_resnet_bwd_partial_floats
// over the coverage and one step outside each of its bounds, and sx_resnet_flow_bwd's validator: null and misaligned pointers, bad
// widths, a negative iteration count, a wrapped network without its sigma row, gradients without the partial buffer (each: a
// non-zero status and a message in sx_last_error()), and valid arguments with n_rows = 0 (status 0, nothing is launched).
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

static float g_buf[8192];

// dim -> widths[0] -> ... -> dim, every layer after the first wrapped
static sx_resnet_net make_net(int dim, int n_hidden, const int *hidden) {
    sx_resnet_net net;
    memset(&net, 0, sizeof net);
    net.n_layers = n_hidden + 1;
    net.dim = dim;
    net.act = SX_ACT_RELU;
    net.final_act = SX_ACT_IDENTITY;
    for (int l = 0; l <= n_hidden && l < SX_RESNET_MAX_LAYERS; ++l) {
        net.layer[l].W = g_buf;
        net.layer[l].b = g_buf + 4096;
        net.layer[l].in_dim = l == 0 ? dim : hidden[l - 1];
        net.layer[l].out_dim = l == n_hidden ? dim : hidden[l];
        net.layer[l].sigma_col = l == 0 ? -1 : l - 1;
    }
    net.n_wrapped = n_hidden;
    return net;
}

int main() {
    // host memory stands in for device memory: no call below reaches a launch
    float *x = g_buf, *gin = g_buf + 1024, *gout = g_buf + 2048, *sig = g_buf + 3072, *part = g_buf + 5120;
    const int h64[3] = {64, 64, 64}, h32[3] = {32, 32, 32}, h65[3] = {65, 64, 64}, h48[1] = {48};

    // ---- the two size functions
    sx_resnet_net n0 = make_net(3, 0, h32), n1 = make_net(33, 1, h48), n2 = make_net(64, 2, h64), n3 = make_net(64, 3, h64);
    sx_resnet_net n3s = make_net(32, 3, h32);
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&n0), 4 * ((1024 + 32) + 1024 + 8 * 1056));
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&n1), 4 * (2 * (2 * 2 * 1024 + 64) + 2 * 4096 + 8 * 1056));
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&n2), 4 * (3 * (4096 + 64) + 3 * 4096 + 8 * 1056));
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&n3), 0);                     // 162 KiB: over the budget
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&n3s), 4 * (4 * (1024 + 32) + 4 * 1024 + 8 * 1056));
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(nullptr), 0);
    sx_resnet_net bad = make_net(65, 1, h48);
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = make_net(64, 1, h65);
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = n2; bad.n_layers = 5;
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = n2; bad.n_layers = 0;
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = n2; bad.act = SX_ACT_GELU + 1;
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = n2; bad.final_act = -1;
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = n2; bad.layer[1].in_dim = 32;
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    bad = n2; bad.layer[2].out_dim = 32;
    EXPECT_EQ(sx_resnet_bwd_lds_bytes(&bad), 0);
    EXPECT_EQ(sx_resnet_bwd_partial_floats(&n2, 0), 0);
    EXPECT_EQ(sx_resnet_bwd_partial_floats(&n2, -5), 0);
    EXPECT_EQ(sx_resnet_bwd_partial_floats(nullptr, 100), 0);
    const long long per_wave = 12 * 1024 + 6 * 64 + 2 * 6 * 1024;   // G_l, db_l, the stash of the layers' inputs and of e_l
    EXPECT_EQ(sx_resnet_bwd_partial_floats(&n2, 1), 4 * per_wave);
    EXPECT_EQ(sx_resnet_bwd_partial_floats(&n2, 128), 4 * per_wave);
    EXPECT_EQ(sx_resnet_bwd_partial_floats(&n2, 129), 8 * per_wave);
    EXPECT_EQ(sx_resnet_bwd_partial_floats(&n2, (int64_t)1 << 40), 512 * 4 * per_wave);
    size_t prev = 0;
    for (int64_t n = 0; n < 70000; n += 97) {
        ++g_calls;
        const size_t now = sx_resnet_bwd_partial_floats(&n2, n);
        if (now < prev) { fprintf(stderr, "FAIL sx_resnet_bwd_partial_floats is not monotone at %lld\n", (long long)n); ++g_fail; }
        prev = now;
    }

    // ---- the validator
    sx_resnet_grads gr;
    memset(&gr, 0, sizeof gr);
    EXPECT_OK(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 0, 100, 1, nullptr));
    EXPECT_OK(sx_resnet_flow_bwd(&n2, x, x, sig, gin, gout, gout, nullptr, &gr, 0, 0, 0, nullptr));
    EXPECT_OK(sx_resnet_flow_bwd(&n0, x, nullptr, nullptr, gin, gout, nullptr, nullptr, nullptr, 0, 1, 0, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(nullptr, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, nullptr, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, nullptr, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, nullptr, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, nullptr, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));      // no sigma row
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, -1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, -4, 1, 1, nullptr));
    float *odd = (float *)((char *)g_buf + 2);
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, odd, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, odd, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, odd, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, odd, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, odd, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, odd, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, nullptr, odd, nullptr, 4, 1, 1, nullptr));
    gr.dW[1] = odd;
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, nullptr, part, &gr, 4, 1, 1, nullptr));
    gr.dW[1] = part;
    EXPECT_BAD(sx_resnet_flow_bwd(&n2, x, nullptr, sig, gin, gout, nullptr, nullptr, &gr, 4, 1, 1, nullptr));     // no partial buffer
    gr.dW[1] = nullptr;
    bad = n2; bad.layer[0].W = nullptr;
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = n2; bad.layer[1].b = odd;
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = make_net(65, 1, h48);
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = make_net(64, 1, h65);
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = n2; bad.layer[2].out_dim = 32;
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = n2; bad.n_layers = 5;
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = n2; bad.act = 99;
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    bad = n2; bad.layer[1].sigma_col = 7;
    EXPECT_BAD(sx_resnet_flow_bwd(&bad, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));
    EXPECT_BAD(sx_resnet_flow_bwd(&n3, x, nullptr, sig, gin, gout, nullptr, nullptr, nullptr, 4, 1, 1, nullptr));         // LDS budget

    printf("asan_resnet_bwd_driver: %ld calls, %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
