// dev_mem.h — device memory and events owned by the variable that holds them: a DevBuf frees its array when it goes out of scope, when it is
// allocated again and when the struct it is a member of is destroyed.  No list of pointers to free is kept anywhere.
#pragma once
#include "kmdb_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <type_traits>
#include <utility>

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return kmdb_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// A meter of the device bytes the calling thread holds through DevBuf (and build.hip's BBuf) while it is installed: kmdb_build_finish_device
// reports the peak of builder plus handle with it.  Null (the default): nothing is counted.  A buffer made before the meter was installed and
// released under it would count as negative: the hand-off installs it before the handle exists and takes it off before it returns.
struct DevMemMeter {
    long long live = 0, peak = 0;
    void add(size_t b) { live += (long long)b; if (live > peak) peak = live; }
    void sub(size_t b) { live -= (long long)b; }
};
inline thread_local DevMemMeter* dev_mem_meter = nullptr;

// Reads as the T* it replaces: a kernel argument, `q.field = buf`, `buf + n` and `if (!buf)` go through the conversion.  (A function template
// that deduces its argument takes buf.get(): a DevBuf cannot be copied.)
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {       // (declaring the moves deletes the copies)
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~DevBuf() { reset(); }
    // n elements (DevBuf<void>: bytes).  What the buffer held goes FIRST — the pools are tens of GB, old and new do not fit side by side — and
    // a size of 0 still yields an array.  0, or 1 with the error set.
    int alloc(size_t n, const char* what = "DevBuf::alloc") {
        reset();
        const size_t want = std::max<size_t>(n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>), 1);
        const hipError_t e = hipMalloc((void**)&p_, want);
        if (e != hipSuccess) { p_ = nullptr; return kmdb_set_error(std::string(what) + ": hipMalloc of " + std::to_string(want) + " B: " + hipGetErrorString(e)); }
        bytes_ = want;
        if (dev_mem_meter) dev_mem_meter->add(want);
        return 0;
    }
    void reset() {
        if (p_) { (void)hipFree(p_); if (dev_mem_meter) dev_mem_meter->sub(bytes_); }
        p_ = nullptr; bytes_ = 0;
    }
    // the array of a buffer of another element type becomes this one's (what this one held goes first); `o` is left empty
    template <class U> void take(DevBuf<U>& o) { reset(); bytes_ = o.bytes(); p_ = (T*)o.release(); }
    T* release() { bytes_ = 0; return std::exchange(p_, nullptr); }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "a copy of a DevBuf would free its array twice");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value && std::is_nothrow_move_assignable<DevBuf<int>>::value, "a DevBuf moves");

// frees several buffers at once: a growth path gives ALL its old arrays back before it allocates the first new one
template <class... B> inline void dev_reset(B&... b) { (b.reset(), ...); }
// buf.alloc(n) in a function that returns the engine's int status; the error names the buffer and the count, as HIP_TRY names its expression
#define DEV_ALLOC(buf, n) do { if ((buf).alloc((n), #buf ".alloc(" #n ")")) return 1; } while (0)
// untyped scratch (DevBuf<void>) sized in bytes, 16 at the least
#define DEV_ALLOC_BYTES(buf, bytes) DEV_ALLOC(buf, std::max<size_t>((bytes), 16))

class DevEvent {
public:
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); } return *this; }
    ~DevEvent() { reset(); }
    // destroys the event it held first; 0, or 1 with the error set
    int create(unsigned flags = hipEventDefault) {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) { e_ = nullptr; return kmdb_set_error(std::string("hipEventCreate: ") + hipGetErrorString(e)); }
        return 0;
    }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};
static_assert(!std::is_copy_constructible<DevEvent>::value && std::is_nothrow_move_constructible<DevEvent>::value, "a DevEvent moves and is never copied");
