// The failed-allocation rule of hip_owning.h's buffers, on a machine (or in an environment) without a
// HIP device: an ensure that fails leaves p == nullptr and n == 0, the first time and after an earlier
// failure, so no later call can take a stale capacity for a buffer.  Host only; with a device visible
// the program refuses to run (exit code 2) rather than allocate.
#include <cstdio>

#include "../../ldso_amd/csrc/hip_owning.h"

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                               \
        }                                                             \
    } while (0)

static int hook_calls = 0;
struct CountingHook {
    static void changed() { hook_calls++; }
};

template <typename Buf>
static void check_ensure_fails(const char *what, size_t first, size_t second) {
    Buf b;
    const int rc1 = b.ensure(first);
    CHECK(rc1 < 0);
    CHECK(b.p == nullptr && b.n == 0);
    CHECK(ldso_ba::last_error()[0] != 0);
    const int rc2 = b.ensure(second);  // smaller than the first: a stale capacity would let it pass
    CHECK(rc2 < 0);
    CHECK(b.p == nullptr && b.n == 0);
    std::printf("%s: rc %d, %d: %s\n", what, rc1, rc2, ldso_ba::last_error());
}

int main() {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) {
        std::printf("a HIP device is visible: not provoking allocation failures on it\n");
        return 2;
    }
    check_ensure_fails<DevBuf<float>>("DevBuf", 1000, 10);
    check_ensure_fails<DevBuf<float, CountingHook>>("DevBuf with a hook", 1000, 10);
    CHECK(hook_calls == 2);  // every attempt to (re)allocate is announced; the destructor of an empty buffer is not
    check_ensure_fails<PinBuf<double>>("PinBuf", 1000, 10);
    check_ensure_fails<PinMappedOf<int>>("PinBuf, mapped", 1000, 10);
    DevBuf<float> d;
    CHECK(d.alloc(0) == 0 && d.p == nullptr && d.n == 0);  // an empty buffer is not an error
    Event ev;
    CHECK(ev.ensure(hipEventDisableTiming) < 0 && ev.e == nullptr);
    // a borrow that cannot create its events refuses, holds neither, and refuses again
    StreamBorrow sb;
    for (int attempt = 0; attempt < 2; attempt++) {
        CHECK(sb.begin(nullptr, nullptr) < 0);
        CHECK(sb.taken.e == nullptr && sb.given.e == nullptr);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
