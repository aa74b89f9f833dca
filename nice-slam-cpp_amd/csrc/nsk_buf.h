// nsk_buf.h -- DevBuf<T, A>: the one owner of a device allocation and of the capacity it was made with.
// A is the allocator policy: static int alloc(void**, size_t bytes) (0 = success) and static void free(void*).  nsk.hip instantiates it with
// hipMalloc / hipFree, host/test/buf_test.cpp with a counting fake; nothing here needs HIP.
#pragma once
#include <cstddef>
#include <utility>

template <typename T, typename A>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;            // elements
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }          // kernel-argument structs and launches keep raw pointers
    size_t cap() const { return cap_; }
    void reset() { if (p_) A::free(p_); p_ = nullptr; cap_ = 0; }
    // Frees first, so a failure leaves the buffer empty (null, capacity 0) and never pointing at freed memory; returns the allocator's code.
    int alloc(size_t n)
    {
        reset();
        void* q = nullptr;
        const int e = A::alloc(&q, n * sizeof(T));
        if (e != 0) return e;
        p_ = static_cast<T*>(q); cap_ = n;
        return 0;
    }
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
};

// Buffers that share one capacity fail as a group: after a failure none of them is allocated.
template <typename... B>
inline void reset_all(B&... b) { (b.reset(), ...); }
