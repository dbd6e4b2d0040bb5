// Host-only: what every unit of the library builds on -- the device guard and the step from a HIP error to a status, the
// capture query, the ONE wait for a stamp in mapped host memory, the owners of mapped / pinned host blocks and of device
// arrays, and the step from a runtime value to a template argument.  Nothing here launches a kernel or knows a workspace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <utility>

#include "cavmd.h"

namespace
{
constexpr unsigned kResultHistoryMax = 16384; // deepest result ring: of a workspace ("result_history") and of a batch

// ---- the device of an object, and HIP errors as statuses --------------------------------------------------------------------
struct DeviceGuard
{
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev)
        {
            switched = (hipSetDevice(dev) == hipSuccess);
        }
    }
    ~DeviceGuard()
    {
        if (switched)
            (void)hipSetDevice(prev);
    }
};

inline int hip_status(hipError_t e)
{
    return e == hipSuccess ? CAVMD_OK : (int)e;
}

#define CAVMD_HIP_TRY(expr)              \
    do                                   \
    {                                    \
        hipError_t _e = (expr);          \
        if (_e != hipSuccess)            \
            return (int)_e;              \
    } while (0)

// ---- is `stream` being captured? --------------------------------------------------------------------------------------------
// The null stream cannot be captured and costs no query (HOOMD-blue's and torch's default path).  `unknown` is a query that
// failed: callers that must not enqueue into a capture treat it as one, callers that only skip a wait treat it as none.
enum class Capture
{
    none,
    active,
    unknown
};

Capture capture_state(hipStream_t stream)
{
    if (stream == nullptr)
        return Capture::none;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess)
        return Capture::unknown;
    return cs != hipStreamCaptureStatusNone ? Capture::active : Capture::none;
}

bool stream_capturing(hipStream_t stream)
{
    return capture_state(stream) == Capture::active;
}

// ---- the wait for a stamp ---------------------------------------------------------------------------------------------------
// A publishing kernel stores its block and then a sequence stamp (system-scope release) into mapped coherent host memory.  The
// host spins on that stamp: the values arrive about a PCIe write after the block that computes them has them, instead of a
// stream synchronisation (~15 us).  Never a stream synchronisation here: it would wait behind newer work.  The wait is also
// over once `later()` says so (a LATER evaluation has published: the stream runs them in order) or the stream is idle (a
// failed launch never sets the stamp); the stamp is then looked at once more, since it may have landed in between.
struct StampWait
{
    bool arrived;     // the stamp carries `want`; false with error == hipSuccess: the work is over without its stamp
    hipError_t error; // of the stream query
};

template <class Later>
StampWait wait_for_stamp(const uint64_t* stamp, uint64_t want, hipStream_t stream, Later later)
{
    for (;;)
    {
        if (__atomic_load_n(stamp, __ATOMIC_ACQUIRE) == want)
            return {true, hipSuccess};
        if (!later())
        {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipErrorNotReady)
                continue;
            if (q != hipSuccess)
                return {false, q};
        }
        return {__atomic_load_n(stamp, __ATOMIC_ACQUIRE) == want, hipSuccess};
    }
}

inline StampWait wait_for_stamp(const uint64_t* stamp, uint64_t want, hipStream_t stream)
{
    return wait_for_stamp(stamp, want, stream, [] { return false; });
}
} // namespace

// ---- owners -----------------------------------------------------------------------------------------------------------------
// Move-only; an owner is either empty or holds one live allocation, and a failed alloc leaves it empty.  Freed by free() or
// with the owner; whoever destroys an owner holds the DeviceGuard of its device.  A group of buffers that belongs together
// is allocated into local owners and moved into place once all of them are there: commit whole or not at all.
// In the library's named namespace, not the anonymous one: struct cavmd_workspace, which two units define, has such members.
namespace cavmd
{
// `count` zeroed Ts of pinned host memory; kMapped: mapped into the device's address space and coherent (the polled stamps
// must not depend on HIP_HOST_COHERENT), `dev` being the device-side address of `host`
template <class T, bool kMapped>
struct HostBlock
{
    T* host = nullptr;
    T* dev = nullptr;

    HostBlock() = default;
    HostBlock(HostBlock&& o) noexcept : host(o.host), dev(o.dev) { o.host = o.dev = nullptr; }
    HostBlock& operator=(HostBlock&& o) noexcept
    {
        if (this != &o)
        {
            free();
            host = o.host;
            dev = o.dev;
            o.host = o.dev = nullptr;
        }
        return *this;
    }
    ~HostBlock() { free(); }

    hipError_t alloc(size_t count = 1)
    {
        free();
        T* h = nullptr;
        T* d = nullptr;
        hipError_t e = hipHostMalloc((void**)&h, sizeof(T) * count,
                                     kMapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault);
        if (e == hipSuccess && kMapped)
            e = hipHostGetDevicePointer((void**)&d, h, 0);
        if (e != hipSuccess)
        {
            if (h)
                (void)hipHostFree(h);
            return e;
        }
        memset(h, 0, sizeof(T) * count);
        host = h;
        dev = d;
        return hipSuccess;
    }

    void free()
    {
        if (host)
            (void)hipHostFree(host);
        host = dev = nullptr;
    }
};
template <class T>
using MappedBlock = HostBlock<T, true>;
template <class T>
using PinnedBlock = HostBlock<T, false>;

// `count` Ts of device memory
template <class T>
struct DeviceArray
{
    T* ptr = nullptr;

    DeviceArray() = default;
    DeviceArray(DeviceArray&& o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    DeviceArray& operator=(DeviceArray&& o) noexcept
    {
        if (this != &o)
        {
            free();
            ptr = o.ptr;
            o.ptr = nullptr;
        }
        return *this;
    }
    ~DeviceArray() { free(); }

    hipError_t alloc(size_t count)
    {
        free();
        T* p = nullptr;
        const hipError_t e = hipMalloc((void**)&p, sizeof(T) * count);
        if (e == hipSuccess)
            ptr = p;
        return e;
    }

    hipError_t alloc_zeroed(size_t count)
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess)
            e = hipMemset(ptr, 0, sizeof(T) * count);
        if (e != hipSuccess)
            free();
        return e;
    }

    // a fresh array holding the `count` Ss at `src`, reinterpreted as Ts; at least one T, so that ptr is not NULL afterwards
    template <class S>
    hipError_t upload(const S* src, size_t count)
    {
        const size_t bytes = sizeof(S) * count;
        hipError_t e = alloc(bytes < sizeof(T) ? 1 : bytes / sizeof(T));
        if (e == hipSuccess && bytes)
            e = hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess)
            free();
        return e;
    }

    void free()
    {
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
    }
};
} // namespace cavmd

namespace
{
// ---- from a runtime value to a template argument ----------------------------------------------------------------------------
// A kernel's variants are named by lists of the values a template parameter takes.  with_constant() calls f with the entry
// equal to v as a std::integral_constant (with the LAST entry if none is: every caller's v comes from a checked tunable or
// from arithmetic that stays within its list); with_each_constant() calls f with every entry.  f is a generic lambda that
// reads `decltype(c)::value`, so a kernel's argument list is written once whatever the number of variants.
template <int... Vs>
struct IntList
{
};

template <int V, int... Rest, class F>
auto with_constant(IntList<V, Rest...>, int v, F&& f)
{
    if constexpr (sizeof...(Rest) == 0)
        return f(std::integral_constant<int, V> {});
    else
        return v == V ? f(std::integral_constant<int, V> {}) : with_constant(IntList<Rest...> {}, v, std::forward<F>(f));
}

// (last entry first)
template <int V, int... Rest, class F>
auto with_each_constant(IntList<V, Rest...>, F&& f)
{
    if constexpr (sizeof...(Rest) != 0)
        with_each_constant(IntList<Rest...> {}, f);
    f(std::integral_constant<int, V> {});
}
} // namespace
