// Host-side sanitizer driver of the slab forward tier's wide form (test infrastructure; built by `make -C stribor_amd/csrc
// asan_slab_wide`, run by tests/test_slab_wide_host.py).  The recipe of tests/asan_driver.cpp: the library's HOST code compiled for
// the CPU only (hipcc --offload-host-only) with -fsanitize=address,undefined and driven WITHOUT a GPU -- every call below must come
// back with a status or a size, never crash, never trip a sanitizer report.  Driven: sx_rqs_slab_wide_slots and
// sx_rqs_slab_wide_fwd_scratch_floats over their edges and beyond, every refusal of sx_rqs_slab_wide_fwd's validator (each: a non-zero
// status and a message in sx_last_error()), and valid arguments with n_rows = 0 (status 0, nothing is launched).
#include "../include/stribor_hip.h"
#include <limits.h>
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
        if ((long long)(a) != (long long)(b)) { fprintf(stderr, "FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, (long long)(a), (long long)(b)); ++g_fail; } \
    } while (0)

alignas(16) static float g_buf[256];

int main() {
    // host memory stands in for device memory: no call below reaches a launch
    float *f = g_buf;
    float *odd = (float *)((char *)g_buf + 4);
    const int32_t *idx = (const int32_t *)g_buf;

    // ---- the size queries: n_live * 96 slots, n_live * n_rows floats, 0 outside the widths a slab pass exists for
    EXPECT_EQ(sx_rqs_slab_wide_slots(1), 96);
    EXPECT_EQ(sx_rqs_slab_wide_slots(33), 33 * 96);
    EXPECT_EQ(sx_rqs_slab_wide_slots(1 << 20), 96ll << 20);
    EXPECT_EQ(sx_rqs_slab_wide_slots(0), 0);
    EXPECT_EQ(sx_rqs_slab_wide_slots(-1), 0);
    EXPECT_EQ(sx_rqs_slab_wide_slots((1 << 20) + 1), 0);
    EXPECT_EQ(sx_rqs_slab_wide_slots(INT_MAX), 0);
    EXPECT_EQ(sx_rqs_slab_wide_slots(INT_MIN), 0);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(300, 32), 300 * 32);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(0, 32), 0);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(((int64_t)1 << 36) - 1, 1 << 20), (((int64_t)1 << 36) - 1) << 20);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats((int64_t)1 << 36, 32), 0);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(-1, 32), 0);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(INT64_MAX, INT_MAX), 0);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(300, 0), 0);
    EXPECT_EQ(sx_rqs_slab_wide_fwd_scratch_floats(300, INT_MIN), 0);

    // ---- the validator (argument list: sx_rqs_slab_fwd's without `cubic`)
    EXPECT_BAD(sx_rqs_slab_wide_fwd(nullptr, f, 64, 64, f, f, f, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, f, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, nullptr, 64, 64, f, f, f, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, f, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, nullptr, f, f, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, f, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, nullptr, f, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, f, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, f, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));   // ldj without scratch
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 16, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));   // bins: sx_rqs_slab_fwd's
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 33, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 0, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, INT_MIN, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 320, 257, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr)); // hidden
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 0, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 32, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));   // ld_h < hidden
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 65, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));   // n_live > dim
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 0, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 0, 1, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 0, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));      // dim
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, 3.f, -3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));   // empty domain
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, 3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));    // empty codomain
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, -1, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));  // n_rows < 0
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, (int64_t)1 << 36, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 2, 1.f, 0, 0, nullptr, nullptr, nullptr));   // reverse = 2 is the cubic splines' mode
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, -1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 5, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));   // pass-through columns without their list
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, idx, 33, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));      // more than dim - n_live
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, idx, -1, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, f, 64, 64, odd, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr)); // misaligned pack
    EXPECT_BAD(sx_rqs_slab_wide_fwd(f, odd, 0, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 4, 64, 1, 1.f, 0, 1, nullptr, nullptr, nullptr));  // misaligned fragments
    EXPECT_OK(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, nullptr, nullptr, 32, 32, nullptr, 0, 17, -3.f, 3.f, -3.f, 3.f, 0, 64, 1, 1.f, 0, 0, nullptr, nullptr, nullptr));
    EXPECT_OK(sx_rqs_slab_wide_fwd(f, f, 64, 64, f, f, f, nullptr, 32, 32, idx, 32, 32, -3.f, 3.f, -2.f, 2.f, 0, 64, 0, -1.f, 1, 0, f, nullptr, nullptr));
    EXPECT_OK(sx_rqs_slab_wide_fwd(f, f, 0, 256, f, f, nullptr, idx, 0, 64, nullptr, 0, 24, -3.f, 3.f, -3.f, 3.f, 0, 64, 1, 1.f, 0, 1, nullptr, nullptr, nullptr));

    printf("asan_slab_wide_driver: %ld calls, %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
