// mx_owned.h -- the one owning buffer type of the host code (index.hip, encoder.hip).
// A member or local that OWNS device or pinned memory is an Owned<T, Policy>: freeing is its destructor's job, a view into
// somebody else's buffer stays a raw pointer.  A buffer is released with its owner's device current (DeviceGuard).
#pragma once
#include <cstddef>
#include <type_traits>

namespace mx {

// Policy: `using error = ...; static constexpr error ok; static error acquire(void **, size_t bytes, unsigned flags);
// static void release(void *)`.  acquire leaves *p alone on failure.
template <class T, class Policy>
class Owned {
    T *p_ = nullptr;
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);

  public:
    using error = typename Policy::error;
    Owned() = default;
    Owned(Owned &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }

    // both release what was held first and leave the buffer null on failure
    error alloc_bytes(size_t bytes, unsigned flags = 0) {
        reset();
        void *p = nullptr;
        const error e = Policy::acquire(&p, bytes, flags);
        if (e == Policy::ok) p_ = static_cast<T *>(p);
        return e;
    }
    error alloc(size_t count, unsigned flags = 0) { return alloc_bytes(count * kElem, flags); }
    void reset() {
        if (p_) Policy::release(const_cast<std::remove_const_t<T> *>(p_));
        p_ = nullptr;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }  // reads (p.x = idx->x, idx->flags + 2, if (idx->dead), buf[i]) stay as they were
};

}  // namespace mx

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <atomic>

namespace mx {
namespace {  // internal linkage: the -DMEMEX_TESTING object and the plain ones share a library, each with its own policies

#ifdef MEMEX_TESTING
// the testing build counts live buffers and can fail the n-th next allocation without calling HIP
// (mx_testing_live_buffers, mx_testing_fail_alloc)
std::atomic<long> g_owned_live{0}, g_owned_allocs{0}, g_owned_fail_at{0};
inline bool owned_fail_now() {
    g_owned_allocs.fetch_add(1);
    return g_owned_fail_at.load() > 0 && g_owned_fail_at.fetch_sub(1) == 1;
}
inline hipError_t owned_count(hipError_t e) {
    if (e == hipSuccess) g_owned_live.fetch_add(1);
    return e;
}
#define MX_OWNED_ACQUIRE(call) (owned_fail_now() ? hipErrorOutOfMemory : owned_count(call))
#define MX_OWNED_RELEASED() g_owned_live.fetch_sub(1)
#else
#define MX_OWNED_ACQUIRE(call) (call)
#define MX_OWNED_RELEASED() (void)0
#endif

struct DevMem {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error acquire(void **p, size_t bytes, unsigned) { return MX_OWNED_ACQUIRE(hipMalloc(p, bytes)); }
    static void release(void *p) {
        (void)hipFree(p);
        MX_OWNED_RELEASED();
    }
};
struct PinMem {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error acquire(void **p, size_t bytes, unsigned flags) { return MX_OWNED_ACQUIRE(hipHostMalloc(p, bytes, flags)); }
    static void release(void *p) {
        (void)hipHostFree(p);
        MX_OWNED_RELEASED();
    }
};

}  // namespace

template <class T>
using Dev = Owned<T, DevMem>;
template <class T>
using Pin = Owned<T, PinMem>;

}  // namespace mx
#endif
