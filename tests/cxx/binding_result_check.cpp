// Host-only check of who frees a result buffer of the Python binding (gbrl_amd/csrc/binding_result.h; compiled with the address and
// undefined-behaviour sanitizers and run by tests/test_host.py).  The device side goes through a memory policy that counts; the host side is
// new[] / delete[], which the address sanitizer watches: a leak or a second free ends the program with a non-zero status.
#include "binding_result.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

using gbrl_py::ResultBuffer;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("MISMATCH " __VA_ARGS__); std::printf("  (%s)\n", #cond); std::exit(1); } } while (0)

// "device" memory: malloc behind counters, and an allocation that can be told to fail
struct Counting {
    static int allocs, frees, last_device;
    static bool fail_next;
    static void *alloc(int device_id, size_t bytes) {
        last_device = device_id;
        if (fail_next) { fail_next = false; return nullptr; }
        ++allocs;
        return std::malloc(bytes ? bytes : 1);
    }
    static void free(void *p) { ++frees; std::free(p); }
    static void reset() { allocs = frees = 0; last_device = -1; fail_next = false; }
};
int Counting::allocs = 0, Counting::frees = 0, Counting::last_device = -1;
bool Counting::fail_next = false;

template <typename T>
using Buf = ResultBuffer<T, Counting>;

// a call that fails: the buffer is still owned when the exception passes, and is freed exactly once
static void check_failed_call() {
    Counting::reset();
    try {
        Buf<float> dev(true, 3, 16);
        Buf<int32_t> host(false, 3, 16);
        CHECK(dev.get() && dev.on_device() && dev.device_id() == 3 && Counting::last_device == 3, "device buffer on device 3\n");
        CHECK(host.get() && !host.on_device() && host.device_id() == 0, "a host buffer names device 0\n");
        host.get()[15] = 7;
        throw std::runtime_error("the C call failed");
    } catch (const std::runtime_error &) {
    }
    CHECK(Counting::allocs == 1 && Counting::frees == 1, "failed call: %d allocations, %d frees\n", Counting::allocs, Counting::frees);
    {   // an allocation that fails leaves nothing to free
        Counting::fail_next = true;
        Buf<float> none(true, 0, 16);
        CHECK(none.get() == nullptr, "a failed allocation is a null buffer\n");
    }
    CHECK(Counting::allocs == 1 && Counting::frees == 1, "failed allocation: %d allocations, %d frees\n", Counting::allocs, Counting::frees);
    std::printf("failed call: one device and one host buffer freed once, a failed allocation frees nothing\n");
}

// a call that succeeds: take() hands the buffer over exactly once, and the destructor leaves it alone
static void check_handover() {
    Counting::reset();
    float *dp = nullptr;
    int32_t *hp = nullptr;
    {
        Buf<float> dev(true, 1, 8);
        Buf<int32_t> host(false, 0, 8);
        float *before = dev.get();
        dp = dev.take();
        hp = host.take();
        CHECK(dp == before && dev.get() == nullptr && dev.take() == nullptr, "take() empties the buffer: a second take() is null\n");
        CHECK(hp != nullptr && host.get() == nullptr, "host take()\n");
    }
    CHECK(Counting::frees == 0, "a buffer handed over is not freed by its former owner (%d frees)\n", Counting::frees);
    Counting::free(dp);   // the new owner's turn: a double free or a leak here is the sanitizer's to report
    delete[] hp;
    CHECK(Counting::allocs == 1 && Counting::frees == 1, "handover: %d allocations, %d frees\n", Counting::allocs, Counting::frees);
    std::printf("handover: take() hands over once, the destructor frees nothing afterwards\n");
}

// the in-place form: the caller's buffer is never freed, whether the call fails or succeeds
static void check_adopted() {
    Counting::reset();
    float callers[4] = {1.0f, 2.0f, 3.0f, 4.0f};
    for (int on_device = 0; on_device <= 1; ++on_device) {
        try {
            Buf<float> in_place(Buf<float>::Adopt{}, callers, on_device != 0);
            CHECK(in_place.get() == callers && in_place.adopted() && in_place.on_device() == (on_device != 0), "an adopted buffer is the caller's pointer\n");
            if (on_device) throw std::runtime_error("the C call failed");
        } catch (const std::runtime_error &) {
        }
    }
    CHECK(Counting::allocs == 0 && Counting::frees == 0 && callers[3] == 4.0f, "adopted: %d allocations, %d frees\n", Counting::allocs, Counting::frees);
    std::printf("adopted: nothing allocated, nothing freed\n");
}

int main() {
    check_failed_call();
    check_handover();
    check_adopted();
    std::printf("all sections passed\n");
    return 0;
}
