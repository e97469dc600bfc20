// svo_scene_plan.hpp — the planning of a scene job's cloud points (include/svo_hip.h, "scene clouds"): what a span
// must look like, the pieces a span is cut into for the splat pass, the bytes a slot stages and the chunks of slots a
// job runs in. Plain C++: no HIP, no error text; svo_group_scene.hip and svo_capi_tables.hip format their own
// messages. tests/cpp/scene_plan_check.cpp exercises it on the CPU, plain and under the sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace svo {

constexpr int SCENE_PLAN_PIECE = 1024;                          // records of one workgroup of the splat pass
constexpr size_t SCENE_PLAN_STAGING = (size_t)256 << 20;        // a chunk of slots stages at most so much (one slot always fits)

inline size_t scene_up256(size_t v) { return (v + 255) / 256 * 256; }

// the key plane of a cols x rows image
inline size_t scene_key_bytes(int cols, int rows) { return scene_up256((size_t)8 * (size_t)cols * (size_t)rows); }

// a span the entry points accept: n >= 0, and with n > 0 a 16-byte aligned, non-null address
inline bool scene_span_ok(uintptr_t points, int64_t n) { return n >= 0 && (n == 0 || (points != 0 && (points & 15) == 0)); }

// the pieces of a span of n records (n <= 0: none)
inline int64_t scene_span_pieces(int64_t n) { return n <= 0 ? 0 : (n + SCENE_PLAN_PIECE - 1) / SCENE_PLAN_PIECE; }

// f(first, count) for every piece of a span of n records, in order: count is SCENE_PLAN_PIECE but for the last one,
// the pieces are disjoint and cover exactly [0, n)
template <typename F>
void scene_each_piece(int64_t n, F f) {
    for (int64_t first = 0; first < n; first += SCENE_PLAN_PIECE) f(first, (int)std::min<int64_t>(SCENE_PLAN_PIECE, n - first));
}

// the slots of one chunk of a job with `named` slots that stage per_slot bytes each; `lower` > 0: the diagnostic
// that asks for fewer. At least 1, at most max(named, 1)
inline size_t scene_chunk_slots(size_t per_slot, size_t named, long long lower) {
    size_t chunk = std::max<size_t>(1, SCENE_PLAN_STAGING / std::max<size_t>(per_slot, 1));
    if (lower > 0) chunk = std::min<size_t>(chunk, (size_t)lower);
    return std::min(chunk, std::max<size_t>(named, 1));
}

// f(first, count) for every chunk of n slots in chunks of `chunk` (>= 1), in order
template <typename F>
void scene_each_chunk(int n, size_t chunk, F f) {
    for (int64_t first = 0; first < n; first += (int64_t)chunk) f((int)first, (int)std::min<int64_t>((int64_t)chunk, n - first));
}

}  // namespace svo
