// nsk_devarr.h -- nskh::DevArr<T>: the one device array of the host classes.  It owns its memory through DevBuf<T, A> of csrc/nsk_buf.h (the
// owner of every device buffer of the context), and every copy and memset goes through the context's stream, so it is ordered with the
// launches: an upload waits for the kernels that still read the old contents, a download for the kernels that write what it fetches.
#pragma once
#include <algorithm>
#include <type_traits>

#include <hip/hip_runtime_api.h>

#include "nsk_buf.h"
#include "nsk_host.h"

namespace nskh {

struct HipAlloc {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};

inline void hip_ok(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// grow-only; movable, not copyable.  An array asked for zero elements still has a pointer (the entry points reject NULL even beside a zero count).
template <typename T>
class DevArr {
    DevBuf<T, HipAlloc> buf;
    static hipStream_t stream() { return (hipStream_t)nsk_stream(ctx()); }
public:
    DevArr() = default;
    explicit DevArr(size_t n) { ensure(n); }
    T* p() const { return buf.get(); }
    size_t cap() const { return buf.cap(); }
    void ensure(size_t n)
    {
        if (buf.get() && n <= buf.cap()) return;
        nsk_ctx* c = ctx();                              // (the allocation lands on the context's device)
        if (buf.get()) check(nsk_sync(c));               // nobody may still be reading the old buffer
        const size_t m = std::max<size_t>(n, 1);
        const int e = buf.alloc(m);
        if (e != 0) throw std::runtime_error("DevArr: hipMalloc of " + std::to_string(m * sizeof(T)) + " bytes failed: " + hipGetErrorString((hipError_t)e));
    }
    // n elements of h to the elements from `at` on; `at` > 0 needs an array that already holds at + n
    void upload(const T* h, size_t n, size_t at = 0)
    {
        ensure(at + n);
        if (n == 0) return;
        hip_ok(hipMemcpyAsync(buf.get() + at, h, n * sizeof(T), hipMemcpyHostToDevice, stream()), "hipMemcpyAsync H2D");
        check(nsk_sync(ctx()));                          // h may be a temporary
    }
    void zero(size_t n) { ensure(n); hip_ok(hipMemsetAsync(buf.get(), 0, n * sizeof(T), stream()), "hipMemsetAsync"); }
    void download(T* h, size_t n) const
    {
        if (n == 0) return;
        hip_ok(hipMemcpyAsync(h, buf.get(), n * sizeof(T), hipMemcpyDeviceToHost, stream()), "hipMemcpyAsync D2H");
        check(nsk_sync(ctx()));
    }
};
static_assert(!std::is_copy_constructible<DevArr<float>>::value && !std::is_copy_assignable<DevArr<float>>::value, "a copy would free the memory twice");
static_assert(std::is_nothrow_move_constructible<DevArr<float>>::value && std::is_nothrow_move_assignable<DevArr<float>>::value, "DevArr moves");

DevArr<float> to_device(const torch::Tensor& t);                        // any float tensor (CPU or CUDA) -> contiguous fp32 on the device
torch::Tensor to_host(const DevArr<float>& d, at::IntArrayRef shape);   // the first numel(shape) floats -> CPU tensor

}  // namespace nskh
