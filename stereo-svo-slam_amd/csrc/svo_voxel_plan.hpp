// svo_voxel_plan.hpp — the host arithmetic of the voxel maps (include/svo_hip.h, "voxel maps"): the bytes of a map,
// the placement hash, the load bound a fuse is admitted by, what a span and a region must look like, the tiles a span
// is cut into and the staging of an extraction. Plain C++: no HIP, no error text; svo_capi_voxel.hip formats its own
// messages. tests/cpp/voxel_plan_check.cpp exercises it on the CPU, plain and under the sanitizers; the prune's, the
// carve's and the entries' parts have a program each beside it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace svo {

constexpr uint32_t VOXEL_MAGIC = 0x31585653u;       // "SVX1"
constexpr size_t VOXEL_HEADER_BYTES = 256;
constexpr size_t VOXEL_ENTRY_BYTES = 40;            // key u64 + eight u32 accumulators
constexpr int VOXEL_TILE = 256;                     // records of a fuse workgroup, entries of an extraction tile
constexpr int VOXEL_LOG2_MIN = 6, VOXEL_LOG2_MIN_CTX = 10, VOXEL_LOG2_MAX = 26;
constexpr uint64_t VOXEL_EMPTY = ~(uint64_t)0;
constexpr uint64_t VOXEL_HASH = 0x9E3779B97F4A7C15ull;

inline bool voxel_log2_ok(int log2_capacity, bool ctx) {
    return log2_capacity >= (ctx ? VOXEL_LOG2_MIN_CTX : VOXEL_LOG2_MIN) && log2_capacity <= VOXEL_LOG2_MAX;
}

// header, key plane, accumulator records (0 for a log2_capacity no entry accepts)
inline size_t voxel_map_bytes(int log2_capacity) {
    if (!voxel_log2_ok(log2_capacity, false)) return 0;
    return VOXEL_HEADER_BYTES + (VOXEL_ENTRY_BYTES << log2_capacity);
}

// where a key's probe chain starts
inline uint64_t voxel_home(uint64_t key, int log2_capacity) { return (key * VOXEL_HASH) >> (64 - log2_capacity); }

// the entries a map may hold at most: capacity - capacity / 4
inline uint64_t voxel_load_limit(int log2_capacity) {
    const uint64_t cap = (uint64_t)1 << log2_capacity;
    return cap - cap / 4;
}

// records += n without wrapping (n >= 0): false when the sum does not fit
inline bool voxel_add_records(uint64_t& records, int64_t n) {
    if (n < 0 || (uint64_t)n > UINT64_MAX - records) return false;
    records += (uint64_t)n;
    return true;
}

// the load bound: n_voxels + records <= capacity - capacity / 4, on the bound (every record may claim an entry)
inline bool voxel_load_ok(uint64_t n_voxels, uint64_t records, int log2_capacity) {
    const uint64_t limit = voxel_load_limit(log2_capacity);
    return n_voxels <= limit && records <= limit - n_voxels;
}

// a span the entries accept: n >= 0, and with n > 0 a 16-byte aligned, non-null address
inline bool voxel_span_ok(uintptr_t points, int64_t n) { return n >= 0 && (n == 0 || (points != 0 && (points & 15) == 0)); }

// the workgroups of a span of n records (n <= 0: none)
inline int64_t voxel_span_tiles(int64_t n) { return n <= 0 ? 0 : n / VOXEL_TILE + (n % VOXEL_TILE != 0); }

// the tiles of an extraction pass over a map
inline int64_t voxel_map_tiles(int log2_capacity) { return (((int64_t)1 << log2_capacity) + VOXEL_TILE - 1) / VOXEL_TILE; }

// a region [first, first + capacity) of an array of `total` records
inline bool voxel_region_ok(int64_t first, int64_t capacity, int64_t total) {
    return first >= 0 && capacity >= 0 && total >= 0 && first <= total && capacity <= total - first;
}

inline size_t voxel_up256(size_t v) { return (v + 255) / 256 * 256; }

// the tile offsets of an extraction: one int per tile and the total
inline size_t voxel_offsets_bytes(int log2_capacity) { return voxel_up256(sizeof(int32_t) * ((size_t)voxel_map_tiles(log2_capacity) + 1)); }

// The staging of an extraction that keeps `kept` entries (known after the count pass): the (key, entry index) pairs
// before and after the sort, and the sort's own temporary storage. Offsets into one block, multiples of 256.
struct VoxelExtractPlan {
    size_t keys_in, keys_out, index_in, index_out, sort_temp, bytes;
};
inline VoxelExtractPlan voxel_extract_plan(uint64_t kept, size_t sort_temp_bytes) {
    VoxelExtractPlan p{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t off = at; at += voxel_up256(bytes); return off; };
    p.keys_in = take(sizeof(uint64_t) * (size_t)kept);
    p.keys_out = take(sizeof(uint64_t) * (size_t)kept);
    p.index_in = take(sizeof(uint32_t) * (size_t)kept);
    p.index_out = take(sizeof(uint32_t) * (size_t)kept);
    p.sort_temp = take(sort_temp_bytes);
    p.bytes = at;
    return p;
}

// does an extraction of `kept` entries fit `capacity` records?
inline bool voxel_extract_fits(int64_t kept, int64_t capacity) { return kept >= 0 && capacity >= 0 && kept <= capacity; }

// ---- voxel prune (include/svo_hip.h, "voxel prune"; tests/cpp/voxel_prune_plan_check.cpp)
constexpr size_t VOXEL_PRUNE_STAGING_MAX = (size_t)1 << 30;

// The index the key rule gives one coordinate of a centre (t = c / voxel; q = floorf(t); i = (int)q + 2^20), in
// float32 as the fuse kernel computes it; false: outside (a NaN and an infinity too), and i is left alone. One division
// and one floor, each rounded once on the host as on the device: there is nothing a compiler could contract.
inline bool voxel_center_index(float c, float voxel, int32_t& i) {
    const float t = c / voxel;
    const float q = __builtin_floorf(t);
    if (!(__builtin_fabsf(q) < 1048576.0f)) return false;
    i = (int32_t)q + 1048576;
    return true;
}

// The staging of a prune of a map whose header counts n_voxels entries (the bound of what is kept; nothing is read
// back before the launches): the accumulator records (32 bytes each, 16-byte aligned) and behind them the keys, in one
// block of up256(40 * n_voxels) bytes. false: the block would exceed VOXEL_PRUNE_STAGING_MAX (or n_voxels a table).
struct VoxelPrunePlan {
    size_t acc, keys, bytes;
};
inline bool voxel_prune_plan(uint64_t n_voxels, VoxelPrunePlan& p) {
    p = VoxelPrunePlan{};
    if (n_voxels > VOXEL_PRUNE_STAGING_MAX / VOXEL_ENTRY_BYTES) return false;
    p.acc = 0;
    p.keys = 32 * (size_t)n_voxels;
    p.bytes = voxel_up256(VOXEL_ENTRY_BYTES * (size_t)n_voxels);
    return p.bytes <= VOXEL_PRUNE_STAGING_MAX;
}

// the workgroups of the reinsert pass over at most n_voxels staged entries
inline int64_t voxel_prune_tiles(uint64_t n_voxels) { return (int64_t)((n_voxels + VOXEL_TILE - 1) / VOXEL_TILE); }

// ---- voxel carve (include/svo_hip.h, "voxel carve"): what a carving rebuild needs behind the prune's block: one
// 64-bit ballot word per wavefront of the count pass (VOXEL_TILE / 64 per tile) and a 256-byte block for the two counters
struct VoxelCarvePlan {
    size_t ballots, counters, bytes;      // offsets from the end of the prune's staging, and the bytes added
};
inline VoxelCarvePlan voxel_carve_plan(int log2_capacity) {
    VoxelCarvePlan p{};
    p.ballots = 0;
    p.counters = voxel_up256(sizeof(uint64_t) * (VOXEL_TILE / 64) * (size_t)voxel_map_tiles(log2_capacity));
    p.bytes = p.counters + 256;
    return p;
}

// the carve's scalar arguments: margin finite and >= 0, near finite and > 0, ring 0 or 1, the image 1 .. 32768 a side
inline bool voxel_carve_scalars_ok(float margin, float near, int ring, int width, int height) {
    const float big = 3.40282347e+38f;
    return margin >= 0.f && margin <= big && near > 0.f && near <= big && (ring == 0 || ring == 1) && width >= 1 && width <= 32768 &&
           height >= 1 && height <= 32768;
}

// ---- voxel entries (include/svo_hip.h, "voxel entries"; tests/cpp/voxel_entries_plan_check.cpp)

// a span of entry records the merge accepts: n >= 0, and with n > 0 a non-null, 8-byte aligned address
inline bool voxel_entry_span_ok(uintptr_t entries, int64_t n) { return n >= 0 && (n == 0 || (entries != 0 && (entries & 7) == 0)); }

// the workgroups of a span of n entry records: the fuse's tiles
inline int64_t voxel_entry_span_tiles(int64_t n) { return voxel_span_tiles(n); }

// two voxel edges are the same edge: bit for bit (0.0 and -0.0 differ, a NaN equals itself; the params check admits neither)
inline bool voxel_edge_same(float a, float b) {
    uint32_t ua, ub;
    __builtin_memcpy(&ua, &a, 4);
    __builtin_memcpy(&ub, &b, 4);
    return ua == ub;
}

// The merge's load bound for one map: n_voxels + (the records of the n_spans spans into it) <= capacity - capacity / 4,
// on the bound. false too when a count is negative or the sum does not fit 64 bits.
inline bool voxel_merge_load_ok(uint64_t n_voxels, const int64_t* span_n, int n_spans, int log2_capacity) {
    uint64_t records = 0;
    for (int i = 0; i < n_spans; i++)
        if (!voxel_add_records(records, span_n[i])) return false;
    return voxel_load_ok(n_voxels, records, log2_capacity);
}

// does a pack of `kept` entries fit `capacity` records? (the extraction's rule)
inline bool voxel_pack_fits(int64_t kept, int64_t capacity) { return voxel_extract_fits(kept, capacity); }

// a rehash into a table of 1 << dst_log2_capacity entries is admitted: the log2 is one the stage entries accept and
// the entries fit under the load limit, on the limit
inline bool voxel_rehash_ok(uint64_t n_voxels, int dst_log2_capacity) {
    return voxel_log2_ok(dst_log2_capacity, false) && n_voxels <= voxel_load_limit(dst_log2_capacity);
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte? (no wrap: the sums are formed as differences)
inline bool voxel_ranges_overlap(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) {
    if (a_bytes == 0 || b_bytes == 0) return false;
    return a <= b ? b - a < a_bytes : a - b < b_bytes;
}

}  // namespace svo
