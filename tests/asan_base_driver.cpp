// Host-side sanitizer driver of the base-density entry points (test infrastructure; built by `make -C stribor_amd/csrc asan_base`, run
// by tests/test_base_host.py).  The recipe of tests/asan_driver.cpp: the library's HOST code compiled for the CPU only
// (hipcc --offload-host-only) with -fsanitize=address,undefined and driven WITHOUT a GPU -- every call below must come back with a
// status, never crash, never trip a sanitizer report.  Driven: sx_base_logprob, sx_normal_bwd_partial_floats, sx_normal_logprob_bwd,
// sx_mvn_lds_bytes, sx_mvn_logprob: null pointers, dim <= 0, negative row counts, bad dtype / kind, dim beyond SX_MVN_MAX_DIM (each: a
// non-zero status and a message in sx_last_error()), and valid arguments with n_rows = 0 (status 0, nothing is launched).
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

int main() {
    // host memory stands in for device memory: no call below reaches a launch
    static float buf[4096];
    float *p = buf, *q = buf + 1024, *o = buf + 2048, *w = buf + 3072;

    // ---- sx_base_logprob
    for (int kind = SX_BASE_NORMAL; kind <= SX_BASE_UNIFORM; ++kind) {
        for (int dtype = SX_F32; dtype <= SX_BF16; ++dtype) {
            EXPECT_OK(sx_base_logprob(p, p, q, 0.f, nullptr, o, 0, 5, dtype, kind, nullptr));
            EXPECT_OK(sx_base_logprob(p, p, q, 0.f, w, o, 0, 128, dtype, kind, nullptr));
        }
        EXPECT_BAD(sx_base_logprob(nullptr, p, q, 0.f, nullptr, o, 4, 5, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, nullptr, q, 0.f, nullptr, o, 4, 5, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, nullptr, 0.f, nullptr, o, 4, 5, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, nullptr, 4, 5, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 4, 0, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 4, -3, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, -1, 5, SX_F32, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 4, 5, 2, kind, nullptr));
        EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 4, 5, -1, kind, nullptr));
    }
    EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 4, 5, SX_F32, 2, nullptr));
    EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 4, 5, SX_F32, -1, nullptr));
    EXPECT_BAD(sx_base_logprob(p, p, q, 0.f, nullptr, o, 0, 5, SX_F32, 7, nullptr));       // (the checks come before the empty return)

    // ---- sx_normal_logprob_bwd and its size function
    EXPECT_EQ(sx_normal_bwd_partial_floats(0, 5), 0);
    EXPECT_EQ(sx_normal_bwd_partial_floats(-4, 5), 0);
    EXPECT_EQ(sx_normal_bwd_partial_floats(4, 0), 0);
    EXPECT_EQ(sx_normal_bwd_partial_floats(1, 3), 2 * 3);
    EXPECT_EQ(sx_normal_bwd_partial_floats(130, 128), 2 * 128 * 33);                       // 4 row lanes: 4 rows per block
    for (long long n = 1; n <= (1ll << 40); n *= 7)
        for (int d : {1, 3, 33, 64, 128, 1000}) {
            ++g_calls;
            const size_t f = sx_normal_bwd_partial_floats(n, d);
            if (f < (size_t)2 * d || f > (size_t)2 * d * 1024) { fprintf(stderr, "FAIL partial floats(%lld, %d) = %zu\n", n, d, f); ++g_fail; }
        }
    EXPECT_OK(sx_normal_logprob_bwd(p, q, p, q, o, nullptr, nullptr, nullptr, 0, 5, nullptr));
    EXPECT_OK(sx_normal_logprob_bwd(p, q, p, q, nullptr, nullptr, nullptr, nullptr, 0, 5, nullptr));
    EXPECT_OK(sx_normal_logprob_bwd(p, q, p, q, nullptr, nullptr, nullptr, nullptr, 9, 5, nullptr));    // nothing wanted: nothing launched
    EXPECT_BAD(sx_normal_logprob_bwd(nullptr, q, p, q, o, nullptr, nullptr, nullptr, 4, 5, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, nullptr, p, q, o, nullptr, nullptr, nullptr, 4, 5, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, nullptr, q, o, nullptr, nullptr, nullptr, 4, 5, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, p, nullptr, o, nullptr, nullptr, nullptr, 4, 5, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, p, q, o, nullptr, nullptr, nullptr, 4, 0, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, p, q, o, nullptr, nullptr, nullptr, 4, -1, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, p, q, o, nullptr, nullptr, nullptr, -4, 5, nullptr));
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, p, q, o, w, nullptr, nullptr, 4, 5, nullptr));               // column sums without the partial buffer
    EXPECT_BAD(sx_normal_logprob_bwd(p, q, p, q, nullptr, nullptr, w, nullptr, 4, 5, nullptr));

    // ---- sx_mvn_logprob and its LDS query
    EXPECT_EQ(sx_mvn_lds_bytes(0), 0);
    EXPECT_EQ(sx_mvn_lds_bytes(-5), 0);
    EXPECT_EQ(sx_mvn_lds_bytes(SX_MVN_MAX_DIM + 1), 0);
    EXPECT_EQ(sx_mvn_lds_bytes(1), (1 * 1024 + 32) * 4);
    EXPECT_EQ(sx_mvn_lds_bytes(32), (1 * 1024 + 32) * 4);
    EXPECT_EQ(sx_mvn_lds_bytes(33), (3 * 1024 + 64) * 4);
    EXPECT_EQ(sx_mvn_lds_bytes(96), (6 * 1024 + 96) * 4);
    EXPECT_EQ(sx_mvn_lds_bytes(128), (10 * 1024 + 128) * 4);
    for (int d = 1; d <= SX_MVN_MAX_DIM; ++d) {
        ++g_calls;
        if (sx_mvn_lds_bytes(d) == 0 || sx_mvn_lds_bytes(d) > 64 * 1024) { fprintf(stderr, "FAIL sx_mvn_lds_bytes(%d)\n", d); ++g_fail; }
    }
    for (int dtype = SX_F32; dtype <= SX_BF16; ++dtype)
        for (int d : {1, 3, 32, 33, 96, 128}) EXPECT_OK(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, 0, d, dtype, nullptr));
    EXPECT_BAD(sx_mvn_logprob(nullptr, p, q, 0.f, nullptr, o, 4, 5, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, nullptr, q, 0.f, nullptr, o, 4, 5, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, nullptr, 0.f, nullptr, o, 4, 5, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, nullptr, 4, 5, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, 4, 0, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, 4, -2, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, -1, 5, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, 4, SX_MVN_MAX_DIM + 1, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, 0, SX_MVN_MAX_DIM + 1, SX_F32, nullptr));
    EXPECT_BAD(sx_mvn_logprob(p, p, q, 0.f, nullptr, o, 4, 5, 2, nullptr));

    printf("asan_base_driver: %ld calls, %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
