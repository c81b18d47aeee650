// Host-side sanitizer driver of the Deep Sets conditioner (test infrastructure; built by `make -C stribor_amd/csrc asan_equivariant`,
// run by tests/test_equivariant_host.py).  The recipe of tests/asan_driver.cpp: the library's HOST code compiled for the CPU only
// (hipcc --offload-host-only) with -fsanitize=address,undefined and driven WITHOUT a GPU -- every call below must come back with a
// status or a size, never crash, never trip a sanitizer report.  Driven: sx_equivariant_lds_bytes and
// sx_equivariant_bwd_partial_floats over the coverage edges and one step outside each, and the validators of sx_equivariant_fwd and
// sx_equivariant_bwd: null and misaligned pointers, bad widths, strides and row counts (each: a non-zero status and a message in
// sx_last_error()), and valid arguments with n_rows = 0 (status 0, nothing is launched).
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

static sx_equivariant_net make_net(int in, int n_hidden, const int *hidden, int out, int N) {
    sx_equivariant_net net;
    memset(&net, 0, sizeof net);
    net.n_layers = n_hidden + 1;
    net.in_dim = in;
    net.act = SX_ACT_TANH;
    net.final_act = SX_ACT_IDENTITY;
    net.set_size = N;
    for (int l = 0; l <= n_hidden && l < 3; ++l) {
        net.A[l] = g_buf; net.a[l] = g_buf + 64; net.B[l] = g_buf + 128; net.b[l] = g_buf + 192;
        net.out_dim[l] = l == n_hidden ? out : hidden[l];
    }
    return net;
}

int main() {
    // host memory stands in for device memory: no call below reaches a launch
    float *x = g_buf, *y = g_buf + 1024, *gy = g_buf + 2048, *dx = g_buf + 3072, *part = g_buf + 4096, *mask = g_buf + 5120;
    float *odd = (float *)((char *)g_buf + 2);
    const int h64[2] = {64, 64}, h32[2] = {32, 32}, h65[2] = {65, 64}, h5[1] = {5}, h33[2] = {33, 32};
    const long long budget = SX_CNF_LDS_BYTES;

    // ---- sx_equivariant_lds_bytes: the forward's coverage
    sx_equivariant_net small = make_net(3, 1, h5, 2, 1), wide = make_net(64, 2, h64, 128, 128), mid = make_net(32, 2, h32, 64, 5);
    // vectors 2 x (32 + 32), scratch 128 x 36, A and B images of two layers
    EXPECT_EQ(sx_equivariant_lds_bytes(&small, 0), 4 * (128 + 128 * 36 + 4 * 1024));
    // the widest shape: every image but the last B fits beside 512 floats of vectors and the 128 x 68 scratch
    EXPECT_EQ(sx_equivariant_lds_bytes(&wide, 0), 4 * (512 + 128 * 68 + 24 * 1024));
    EXPECT_TRUE((long long)sx_equivariant_lds_bytes(&wide, 0) <= budget);
    EXPECT_EQ(sx_equivariant_lds_bytes(nullptr, 0), 0);
    sx_equivariant_net bad = make_net(65, 2, h64, 128, 128);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = make_net(64, 2, h65, 128, 128);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = make_net(64, 2, h64, 129, 128);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = make_net(64, 2, h64, 128, 129);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = wide; bad.set_size = 0;
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = wide; bad.n_layers = 4;
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = wide; bad.n_layers = 1;
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = wide; bad.act = SX_ACT_SILU;
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = wide; bad.final_act = -1;
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);
    bad = wide; bad.out_dim[1] = 0;
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 0), 0);

    // ---- ... and the backward's: in <= 32, out <= 64, and every forward and transposed image resident
    // vectors 2 x (32 + 32 + 64), scratch 128 x 68, slots 8 x 1056, 4 images of 1 + 1 + 2 tiles
    EXPECT_EQ(sx_equivariant_lds_bytes(&mid, 1), 4 * (256 + 128 * 68 + 8 * 1056 + 16 * 1024));
    sx_equivariant_net one64 = make_net(32, 1, h64, 32, 128);
    EXPECT_EQ(sx_equivariant_lds_bytes(&one64, 1), 4 * (192 + 128 * 68 + 8 * 1056 + 16 * 1024));
    EXPECT_EQ(sx_equivariant_lds_bytes(&small, 1), 4 * (128 + 128 * 36 + 8 * 1056 + 8 * 1024));
    EXPECT_EQ(sx_equivariant_lds_bytes(&wide, 1), 0);
    bad = make_net(33, 2, h32, 64, 5);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 1), 0);
    EXPECT_TRUE(sx_equivariant_lds_bytes(&bad, 0) != 0);
    bad = make_net(32, 2, h32, 65, 5);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 1), 0);
    bad = make_net(32, 2, h33, 64, 5);                  // two hidden layers, one of them two tiles wide: the images do not fit
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 1), 0);
    bad = make_net(32, 1, h64, 33, 5);                  // one hidden layer of two tiles with a two-tile output: the same
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 1), 0);
    bad = make_net(32, 1, h65, 32, 5);
    EXPECT_EQ(sx_equivariant_lds_bytes(&bad, 1), 0);

    // ---- sx_equivariant_bwd_partial_floats: 4 waves x min(passes, 512) partials
    const long long per_wave = 2 * (1024 + 1024 + 2048) + 2 * (64 + 64 + 128);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&mid, 0), 0);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&mid, -5), 0);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(nullptr, 100), 0);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&wide, 128), 0);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&mid, 5), 4 * per_wave);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&mid, 125), 4 * per_wave);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&mid, 130), 8 * per_wave);
    EXPECT_EQ(sx_equivariant_bwd_partial_floats(&mid, (int64_t)5 << 40), 512 * 4 * per_wave);
    size_t prev = 0;
    for (int64_t n = 0; n < 70000; n += 95) {
        ++g_calls;
        const size_t now = sx_equivariant_bwd_partial_floats(&mid, n);
        if (now < prev) { fprintf(stderr, "FAIL sx_equivariant_bwd_partial_floats is not monotone at %lld\n", (long long)n); ++g_fail; }
        prev = now;
    }

    // ---- the forward's validator
    EXPECT_OK(sx_equivariant_fwd(&wide, x, 64, nullptr, 0, y, 0, nullptr));
    EXPECT_OK(sx_equivariant_fwd(&mid, x, 40, mask, 3, y, 0, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(nullptr, x, 64, nullptr, 0, y, 128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&wide, nullptr, 64, nullptr, 0, y, 128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 64, nullptr, 0, nullptr, 128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&wide, odd, 64, nullptr, 0, y, 128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 64, odd, 1, y, 128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 64, nullptr, 0, odd, 128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 63, nullptr, 0, y, 128, nullptr));          // the row stride is below in_dim
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 64, mask, 0, y, 128, nullptr));             // a mask without a row stride
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 64, nullptr, 0, y, 127, nullptr));          // not a whole number of sets
    EXPECT_BAD(sx_equivariant_fwd(&wide, x, 64, nullptr, 0, y, -128, nullptr));
    EXPECT_BAD(sx_equivariant_fwd(&mid, x, 32, nullptr, 0, y, 7, nullptr));
    bad = wide; bad.A[1] = nullptr;
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 128, nullptr));
    bad = wide; bad.b[2] = nullptr;
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 128, nullptr));
    bad = wide; bad.B[0] = odd;
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 128, nullptr));
    bad = make_net(65, 2, h64, 128, 128);
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 65, nullptr, 0, y, 128, nullptr));
    bad = make_net(64, 2, h64, 129, 128);
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 128, nullptr));
    bad = wide; bad.set_size = 129;
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 129, nullptr));
    bad = wide; bad.act = 7;
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 128, nullptr));
    bad = wide; bad.n_layers = 4;
    EXPECT_BAD(sx_equivariant_fwd(&bad, x, 64, nullptr, 0, y, 128, nullptr));

    // ---- the backward's validator
    sx_equivariant_grads gr;
    memset(&gr, 0, sizeof gr);
    EXPECT_OK(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, dx, nullptr, nullptr, 0, nullptr));
    EXPECT_OK(sx_equivariant_bwd(&mid, x, 32, mask, 1, gy, dx, nullptr, &gr, 0, nullptr));
    gr.dB[2] = part;
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, dx, nullptr, &gr, 5, nullptr));       // gradients without the partial buffer
    gr.dB[2] = odd;
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, dx, part, &gr, 5, nullptr));
    gr.dB[2] = nullptr;
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, nullptr, part, &gr, 5, nullptr));     // nothing to compute
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, nullptr, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(nullptr, x, 32, nullptr, 0, gy, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, nullptr, 32, nullptr, 0, gy, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, nullptr, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, odd, 32, nullptr, 0, gy, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, odd, 1, gy, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, odd, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, odd, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, dx, odd, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 31, nullptr, 0, gy, dx, nullptr, nullptr, 5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, dx, nullptr, nullptr, 6, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&mid, x, 32, nullptr, 0, gy, dx, nullptr, nullptr, -5, nullptr));
    EXPECT_BAD(sx_equivariant_bwd(&wide, x, 64, nullptr, 0, gy, dx, nullptr, nullptr, 128, nullptr)); // outside the backward's coverage
    bad = make_net(32, 2, h33, 64, 5);
    EXPECT_BAD(sx_equivariant_bwd(&bad, x, 32, nullptr, 0, gy, dx, nullptr, nullptr, 5, nullptr));    // the images are not resident
    bad = mid; bad.a[0] = nullptr;
    EXPECT_BAD(sx_equivariant_bwd(&bad, x, 32, nullptr, 0, gy, dx, nullptr, nullptr, 5, nullptr));

    printf("asan_equivariant_driver: %ld calls, %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
