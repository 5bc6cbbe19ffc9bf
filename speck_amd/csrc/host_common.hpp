// host_common.hpp -- what the host side of every entry point shares: the error macro, size and grid arithmetic, the
// grow-only device buffer the side operations keep their temporaries in, two questions about an address a caller
// passed (on_16_bytes, is_one_of, spans_overlap), and the two questions an entry point asks of its config ("is there a device at all?"
// when none was given, "which stream?" when one was).  Light on purpose: dcsr.hip and extras.hip include it without the
// launch machinery (launch.hpp, chain.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/speck_c_api.h"
#include "device_common.hpp"
#include "guards.hpp"

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            std::fprintf(stderr, "speck_amd: HIP error %s at %s:%d (%s)\n",                 \
                         hipGetErrorString(_e), __FILE__, __LINE__, #expr);                 \
            return (_e == hipErrorOutOfMemory) ? SPECK_ERR_OOM                              \
                   : (_e == hipErrorNoDevice)  ? SPECK_ERR_NO_DEVICE                        \
                                               : SPECK_ERR_HIP;                             \
        }                                                                                   \
    } while (0)

struct speck_config;

namespace speck {

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// workgroups for `work` of them, `cap` at most, one at least (the kernels stride over what a capped grid leaves)
inline u32 grid_of(u64 work, u32 cap) { return (u32)std::max<u64>(1, std::min<u64>(work, cap)); }

// A device allocation that only grows (guards.hpp: with canary zones when the debug option is on).  What it held is
// lost when it grows.
struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t want)
    {
        if (bytes >= want && p) return SPECK_OK;
        release();
        HIP_TRY(guarded_malloc(&p, want));
        bytes = want;
        return SPECK_OK;
    }
    void release()
    {
        if (p) (void)guarded_free(p);
        p = nullptr, bytes = 0;
    }
};

// whether a 16-byte load may start at p
inline bool on_16_bytes(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// whether v is one of X's three arrays (a vector the caller passes may not be)
inline bool is_one_of(const void* v, const speck_dcsr* X) { return v == X->data || v == X->col_ids || v == X->row_offsets; }

// whether [p, p + plen) and [q, q + qlen) share a byte (a NULL span shares nothing): an array a caller passes against a buffer
inline bool spans_overlap(const void* p, u64 plen, const void* q, u64 qlen)
{
    if (!p || !q) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + std::max<u64>(qlen, 1) && b < a + std::max<u64>(plen, 1);
}

// an entry point called without a config: a config exists only where a device does, so nobody has asked yet
inline bool device_present()
{
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess && n > 0) return true;
    (void)hipGetLastError();
    return false;
}

// the stream a call on this config runs on: the caller's (speck_config_set_stream) or the config's own (pipeline.hip)
hipStream_t call_stream(speck_config* c);

}  // namespace speck
