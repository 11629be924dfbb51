// Host helpers shared by the objects of the C ABI (plan.cpp, type3.cpp, toeplitz.cpp, coilmaps.cpp, wavelet.cpp, llr.cpp and, through
// solver_common.h, the solvers): error reporting, the device guard, device buffers counted into an object's own_bytes, the
// struct_size rule of the parameter and info structs, the checks of the callers' pointer tables, and the pinned mirror of a block of device scalars.  What only the iterative
// solvers need (cg.cpp, fista.cpp, tv.cpp, lps.cpp, dcf.cpp, precond.cpp) is in solver_common.h, which includes this file.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "nufft_internal.h"

namespace nufft {

inline int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

#define NUFFT_HIP(expr)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return nufft::fail(e__ == hipErrorOutOfMemory ? NUFFT_ERR_ALLOC : NUFFT_ERR_HIP,   \
                               std::string(#expr) + ": " + hipGetErrorString(e__));            \
    } while (0)

// (for translation units that include rocfft.h)
#define NUFFT_ROCFFT(expr)                                                                     \
    do {                                                                                       \
        rocfft_status s__ = (expr);                                                            \
        if (s__ != rocfft_status_success)                                                      \
            return nufft::fail(NUFFT_ERR_ROCFFT, std::string(#expr) + ": rocfft status " + std::to_string((int)s__)); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool active = false;
    explicit DeviceGuard(int dev) {
        if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) active = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (active) (void)hipSetDevice(prev);
    }
};

inline bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

inline size_t real_bytes(int dtype) { return dtype == NUFFT_F32 ? 4 : 8; }

// Device buffers are padded to whole 16-byte packs of the streaming kernels and to 256 bytes.
inline size_t padded(size_t bytes) { return (std::max<size_t>(bytes, 16) + 255) / 256 * 256; }

// A padded device buffer counted into the owner's own_bytes; `noun` names the owner in the message ("CG", "Toeplitz", ...).
inline int alloc_buffer(int64_t& own_bytes, const char* noun, void** ptr, size_t bytes) {
    bytes = padded(bytes);
    hipError_t e = hipMalloc(ptr, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *ptr = nullptr;
        return fail(NUFFT_ERR_ALLOC, "hipMalloc(" + std::to_string(bytes) + ") of a " + noun + " buffer: " + hipGetErrorString(e));
    }
    own_bytes += (int64_t)bytes;
    return NUFFT_OK;
}

template <typename P>
void free_buffer(int64_t& own_bytes, P*& ptr, size_t bytes) {
    if (!ptr) return;
    (void)hipFree(ptr);
    own_bytes -= (int64_t)padded(bytes);
    ptr = nullptr;
}

// Whether the na bytes at a and the nb bytes at b (or `bytes` at both) share a byte
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char* x = static_cast<const char*>(a);
    const char* y = static_cast<const char*>(b);
    return x < y + nb && y < x + na;
}
inline bool overlap(const void* a, const void* b, size_t bytes) { return overlap(a, bytes, b, bytes); }

// A table of `count` device pointers, 16-byte aligned
inline int check_table(const void* const* tab, int count) {
    if (!tab) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    for (int k = 0; k < count; ++k) {
        if (!tab[k]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if ((uintptr_t)tab[k] & 15) return fail(NUFFT_ERR_INVALID_ARG, "the arrays must be 16-byte aligned");
    }
    return NUFFT_OK;
}

// C outputs and C inputs of `bytes` bytes each, 16-byte aligned.  No output overlaps another output; none overlaps an input either (the
// caller's `refusal` says why), except that out[c] may be exactly in[c] where `in_place` allows it.
inline int check_tables(int C, size_t bytes, void* const* out, const void* const* in, bool in_place, const char* refusal) {
    if (!out || !in) return fail(NUFFT_ERR_INVALID_ARG, "null table");
    for (int c = 0; c < C; ++c) {
        if (!out[c] || !in[c]) return fail(NUFFT_ERR_INVALID_ARG, "null data vector");
        if (((uintptr_t)out[c] | (uintptr_t)in[c]) & 15) return fail(NUFFT_ERR_INVALID_ARG, "the arrays must be 16-byte aligned");
    }
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < C; ++k) {
            if (!(in_place && k == c && out[c] == in[k]) && overlap(out[c], in[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, refusal);
            if (k != c && overlap(out[c], out[k], bytes)) return fail(NUFFT_ERR_INVALID_ARG, "two components of the output overlap");
        }
    return NUFFT_OK;
}

// The struct_size rule.  A caller states how much of a struct its header knows (0: this library's layout).  Parameters: a struct
// smaller than the published layout is refused, and only what this library knows is read.
template <typename S>
int read_params(S& dst, const S* src, const char* name) {
    std::memset(&dst, 0, sizeof(S));
    const size_t known = src->struct_size > 0 ? (size_t)src->struct_size : sizeof(S);
    if (known < sizeof(S)) return fail(NUFFT_ERR_INVALID_ARG, std::string(name) + ".struct_size is smaller than the published layout");
    std::memcpy(&dst, src, sizeof(S));
    return NUFFT_OK;
}

// Info: the smaller of the caller's struct and this library's is written, and its size stored as struct_size.
template <typename S>
void write_info(S* dst, S& src) {
    const size_t known = dst->struct_size > 0 ? std::min((size_t)dst->struct_size, sizeof(S)) : sizeof(S);
    src.struct_size = (int32_t)known;
    std::memcpy(dst, &src, known);
}

// A block of scalars on the device with a pinned copy on the host: the kernels keep them, the host reads them through fetch().
struct ScalarMirror {
    void* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    // The device block (a buffer of the owner) and the host copy; `host_msg` reports the failure that is not alloc_buffer's.
    int create(int64_t& own_bytes, const char* noun, size_t nbytes, const char* host_msg) {
        bytes = nbytes;
        if (int rc = alloc_buffer(own_bytes, noun, &dev, bytes)) return rc;
        if (hipHostMalloc(&host, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            host = nullptr;
            return fail(NUFFT_ERR_ALLOC, host_msg);
        }
        return NUFFT_OK;
    }
    // The initial zeros of the device block; the owner reports a failure together with those of its other memsets.
    hipError_t zero() { return hipMemset(dev, 0, bytes); }
    // Copies the block to the host and waits for it: not on a capturing stream.
    int fetch(hipStream_t stream) {
        NUFFT_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream));
        NUFFT_HIP(hipStreamSynchronize(stream));
        return NUFFT_OK;
    }
    void release() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
    }
};

}  // namespace nufft
