// svo_host.hpp — what the host files of the C ABI share (svo_capi*.hip, svo_ctx*.hip, svo_group*.hip):
// the thread-local error text, HIP_TRY, owners of HIP resources, so that every early return of
// a creation path frees what was made before it, and the chunked upload of a tile table.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <type_traits>

#include "../../include/svo_hip.h"

// the text svo_last_error() returns: per calling thread
inline thread_local char svo_error_text[512] = "";

// stores the message and returns `code`
inline int svo_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(svo_error_text, sizeof(svo_error_text), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return svo_set_error(SVO_ERR_HIP, "%s failed: %s (%s:%d)", #expr,            \
                                 hipGetErrorString(e_), __FILE__, __LINE__);             \
    } while (0)

namespace svo {

inline hipError_t dev_free(void* p) { return hipFree(p); }

struct DevFree { void operator()(void* p) const { (void)dev_free(p); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

template <typename T> using DevPtr = std::unique_ptr<T, DevFree>;        // device memory
template <typename T> using PinnedPtr = std::unique_ptr<T, PinnedFree>;  // pinned host memory
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;

// `bytes` of device memory, not initialised
template <typename T>
hipError_t dev_malloc(DevPtr<T>& p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    p.reset(static_cast<T*>(q));
    return e;
}

template <typename T>
hipError_t pinned_malloc(PinnedPtr<T>& p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
    p.reset(static_cast<T*>(q));
    return e;
}

inline hipError_t make_stream(Stream& s) {
    hipStream_t h = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    s.reset(h);
    return e;
}

inline hipError_t make_event(Event& ev) {
    hipEvent_t h = nullptr;
    const hipError_t e = hipEventCreate(&h);
    ev.reset(h);
    return e;
}

// a diagnostic *_TABLE_TILES override: a table of at most so many tiles (at least one), so that tests reach the
// chunked launches
inline size_t table_tiles(const char* env, size_t cap) {
    if (const char* e = std::getenv(env)) cap = std::max<size_t>(1, std::min<size_t>(cap, (size_t)std::atoll(e)));
    return cap;
}

// A table of at most `cap` tiles, filled on the host (h) and uploaded to its device mirror (d) for
// run(d, tiles, stream): one launch, unless there are more tiles than the table holds.
template <typename Tile, typename Launch>
struct TileTable {
    Tile* h;
    Tile* d;
    size_t cap;
    hipStream_t stream;
    Launch run;
    size_t m = 0;
    // the tiles so far; `more`: the host table is filled again, so the upload must be over
    int launch(bool more) {
        if (m == 0) return SVO_OK;
        HIP_TRY(hipMemcpyAsync(d, h, sizeof(Tile) * m, hipMemcpyHostToDevice, stream));
        run(d, (int)m, stream);
        HIP_TRY(hipGetLastError());
        if (more) HIP_TRY(hipStreamSynchronize(stream));
        m = 0;
        return SVO_OK;
    }
    int add(const Tile& t) {
        if (m == cap)
            if (const int rc = launch(true)) return rc;
        h[m++] = t;
        return SVO_OK;
    }
};
template <typename Tile, typename Launch>
TileTable(Tile*, Tile*, size_t, hipStream_t, Launch) -> TileTable<Tile, Launch>;

}  // namespace svo
