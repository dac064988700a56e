// Host-side scaffolding of the C ABI's entry points (satba_capi.hip and its *_api.inc files): who owns temporary device memory, the
// context of a stand-alone run, and the argument checks that more than one entry point makes.  Host code only.  satba_capi.hip
// includes it behind HIP_TRY, TRY and fail(), which it uses; a new entry point starts from here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
// Owner of device allocations: what it allocated is freed when it goes, in the order of allocation, whatever path leaves the scope.
// On the stack for the temporaries of a call (on the handle's stream or the default stream), a member of a result handle for its arrays.
struct DevAllocs {
    std::vector<void*> ptrs;
    DevAllocs() = default;
    DevAllocs(const DevAllocs&) = delete;
    DevAllocs& operator=(const DevAllocs&) = delete;
    ~DevAllocs() { release(); }
    void release() {
        for (void* q : ptrs) (void)hipFree(q);
        ptrs.clear();
    }
    // n elements, uninitialised (at least one: a pointer to nothing is still a pointer a kernel may be handed)
    template <class T>
    int alloc(T** out, size_t n) {
        HIP_TRY(hipMalloc((void**)out, (n ? n : 1) * sizeof(T)));
        ptrs.push_back(*out);
        return 0;
    }
};

// The context of a stand-alone entry point (no problem handle): a stream of its own, two events around the timed part, and the
// temporaries of the run.
struct DevRun : DevAllocs {
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DevRun() {
        release();  // the memory first, then what the work on it was queued with
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int begin(int device) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamCreate(&stream));
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        return 0;
    }
    // n elements of host data, queued on the stream
    template <class T>
    int upload(T** d, const T* h, size_t n) {
        TRY(alloc(d, n));
        if (h && n) HIP_TRY(hipMemcpyAsync(*d, h, n * sizeof(T), hipMemcpyHostToDevice, stream));
        return 0;
    }
};

// LDS a workgroup may opt in to (asked, not assumed: the Makefile's ARCH can be overridden); 0 when the device does not answer
int dev_lds_limit(int device) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
    int lim = (int)std::max(prop.sharedMemPerBlockOptin, prop.sharedMemPerBlock);
    if (strstr(prop.gcnArchName, "gfx950")) lim = std::max(lim, 160 * 1024);  // CDNA4: 160 KB per workgroup
    return lim;
}

// an int64 offset array of n + 1 entries, checked (starts at 0, does not decrease, total below 2^31) and narrowed to 32 bits;
// have_obs: the arrays it indexes were passed
int dev_check_offsets(int64_t n, const int64_t* ofs, bool have_obs, std::vector<int>& ofs32) {
    const int64_t K = ofs[n];
    if (ofs[0] != 0 || K < 0 || K >= (int64_t)1 << 31 || n >= (int64_t)1 << 31) return fail(SATBA_E_ARG, "offsets out of range");
    if (K && !have_obs) return fail(SATBA_E_ARG, "null observations");
    ofs32.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) {
        if (i && ofs[i] < ofs[i - 1]) return fail(SATBA_E_ARG, "pt_ofs must not decrease");
        ofs32[(size_t)i] = (int)ofs[i];
    }
    return 0;
}

bool cam_all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
}  // namespace
