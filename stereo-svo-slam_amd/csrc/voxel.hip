// voxel.hip — svo_map_point records fused into sparse voxel grids: hash tables in device memory, many spans into many
// maps in one launch, and the maps read back as svo_map_point records in key order. The rule is stated to the bit in
// include/svo_hip.h ("voxel maps"); the host arithmetic (bytes, load bound, staging) is svo_voxel_plan.hpp's.
//
// A map: [header, 256 B][keys: uint64[capacity]][acc: 8 x uint32 per entry: count, sx, sy, sz, sr, sg, sb, last].
// The keys are a plane of their own because the probe reads nothing else; the eight accumulators of an entry are one
// 32-byte record because a fuse touches all eight of an entry together (one sector) and the gather pass reads them
// as two 16-byte loads.
//
// Everything that changes an entry is an integer atomic that commutes: the claim of a key is a 64-bit compare-and-swap
// ~0 -> key (a key never changes again), the sums are adds modulo 2^32, `last` is a max. So a map's content does not
// depend on the order in which wavefronts arrive; only WHERE an entry lies in a probe chain does, and the extraction
// sorts by key. No lane waits for a value another lane or wavefront has yet to write: a probe advances only past
// entries that hold another key for good, and ends after `capacity` steps whatever it sees (the overflow counter;
// the load bound the host checks before the launch keeps a quarter of the table empty, so it stays 0).
//
// voxel_fuse_kernel: a workgroup takes VOXEL_TILE = 256 consecutive records of one span (found by a binary search of
// the spans' tile0 with its blockIdx.x), a lane one record: one 16-byte load, three float divisions. The lanes of a
// wavefront that hold the same key elect the lowest of them as leader (readlane of the first remaining lane's key,
// __ballot of equality; at most 64 rounds, one per distinct key). In the default form the group's seven sums are
// formed inside the wavefront (the count is the ballot's popcount; the six byte-sized values travel as three packed
// words, 64 * 255 < 2^16, through a butterfly of __shfl_xor) and the leader issues one set of eight atomics; with
// lane_atomics every lane adds its own record to the entry its leader found. Leaders probe after the election, all
// at once, so a wavefront pays the probe latency once and not once per distinct key. n_voxels, n_fused, n_outside
// and overflow get at most one atomic add each per wavefront.
//
// Extraction: voxel_count_kernel (ballot + popcount per tile of 256 entries), voxel_scan_kernel (one workgroup: the
// exclusive scan of the tile counts in place, the total behind them), voxel_pairs_kernel ((key, entry) of every kept
// entry at offset + rank), rocprim::radix_sort_pairs over the 63 key bits, voxel_gather_kernel (one lane per record:
// the means in double and 64-bit integers, one 16-byte store). Keys are unique, so the sorted order and every byte
// are the same in every run.
//
// Prune ("voxel prune"): blanking the keys of the entries that leave would cut the probe chains behind them, so the
// map is rebuilt in place, in six launches that the stream orders (no workgroup waits for another): voxel_prune_count_kernel
// and voxel_scan_kernel as above with the keep rule (count, stamp, the box over the key's three 21-bit parts),
// voxel_prune_stage_kernel (every kept entry to the staging block at tile offset + rank: two 16-byte loads and stores
// and the key), voxel_prune_clear_kernel (keys and accumulators; the header stays), voxel_prune_reinsert_kernel (one
// lane per staged entry: the fuse's probe and claim, then plain stores) and voxel_prune_finish_kernel (n_voxels = the
// total). Nothing is read back between them: every kernel after the scan compares the scan's total with the header's
// n_voxels and returns when they are equal, so a prune that removes nothing writes no byte of the map; n_voxels
// changes only in the last launch, so all of them see the same answer.
//
// Carve ("voxel carve"): the prune's rebuild with a second predicate. The count and stage kernels are templates on the
// rule: VoxelKeepDev is the plain prune, unchanged; VoxelCarveRule adds, per non-empty entry, the entry's point (the
// gather's three double divisions), the projection and up to nine gathers of 16-byte occluder records. It is evaluated
// once, in the count pass, which leaves one 64-bit ballot word per wavefront; the stage pass reads the words. The two
// counts are summed inside the workgroup and leave as one 64-bit atomic add each.
//
// Entries ("voxel entries"): voxel_pack_kernel is a second gather behind the extraction's count, scan, pairs and sort
// (launch_voxel_sorted_pairs, shared): one lane per kept entry, two 16-byte loads, one 40-byte record out.
// voxel_merge_kernel is the fuse's launch shape (tiles of 256 records, the binary search of tile0) with one lane per
// 40-byte record: the probe, the claim, eight integer atomics per lane, always atomics, and no election (a pack's keys
// are unique; repeated keys meet at the entry). The header's n_voxels, n_fused (a 64-bit sum of counts) and overflow
// and the call's four counts per map get at most one add each per wavefront. voxel_rehash_kernel is one lane per
// entry of the source table into a cleared table of another size by the reinsert's probe, claim and plain stores
// (voxel_place_unique: the keys of a table are unique and the destination is private), between voxel_clear_kernel on
// the destination and a one-lane launch that copies the four counters; no staging block, nothing read back.
//
// Bounds: of a span, records [0, n) are read. Of a map, keys and acc entries [0, capacity) (slot = (slot + 1) &
// (capacity - 1)) and the header. tile_offsets [0, tiles]; pairs and records [0, n) with n the scan's total. Of a
// prune's staging block, records and keys [0, min(total, n_bound)) with n_bound the n_voxels the block was sized by;
// the clear writes the 16-byte units [0, (40 << log2_capacity) / 16) behind the header. Of a carve: occluder records
// [0, cols * rows) (every cell index is checked against cols and rows), ballot words [0, VOXEL_WAVES * tiles), two counters.
// Of a pack: pairs [0, n) and entry records [0, n) with n the scan's total, which the host compared with the capacity;
// the entry index of a pair is masked by capacity - 1. Of a merge: entry records [0, n) of a span are read, counts[map]
// with map < n_maps (checked on the host), map entries as for a fuse. Of a rehash: source entries [0, capacity), the
// destination's 16-byte units [0, (256 + (40 << log2_capacity')) / 16) by the clear and entries [0, capacity') by the probe.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "svo_host.hpp"
#include "svo_tracker.hpp"
#include "svo_voxel_plan.hpp"

namespace svo {

constexpr int VOXEL_THREADS = 256;
constexpr int VOXEL_WAVES = VOXEL_THREADS / 64;
static_assert(VOXEL_TILE == VOXEL_THREADS, "one lane per record or entry of a tile");
static_assert(sizeof(svo_map_point) == 16 && sizeof(VoxelSpanDev) == 32 && sizeof(VoxelMapDev) == 24, "record sizes");
static_assert(sizeof(svo_voxel_entry) == 40 && alignof(svo_voxel_entry) == 8 && sizeof(VoxelEntrySpanDev) == 32 && sizeof(VoxelMergeCounts) == 32 &&
                  sizeof(svo_voxel_merge_result) == 32,
              "entry record sizes");

#define VOXEL_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ SVO_GP(unsigned long long) voxel_keys(const VoxelMapDev& m) {
    return (SVO_GP(unsigned long long))(m.base + VOXEL_HEADER_BYTES);
}
__device__ __forceinline__ SVO_GP(uint32_t) voxel_acc(const VoxelMapDev& m) {
    return (SVO_GP(uint32_t))(m.base + VOXEL_HEADER_BYTES + ((size_t)8 << m.log2_capacity));
}

// one coordinate: the voxel index + 2^20 and the sub-voxel offset; false: outside (a NaN and an infinity too)
__device__ __forceinline__ bool voxel_coord(float c, float voxel, uint32_t& i, uint32_t& o) {
    const float t = c / voxel;
    const float q = floorf(t);
    if (!(fabsf(q) < 1048576.0f)) return false;
    i = (uint32_t)((int)q + 1048576);
    o = min(255u, (uint32_t)((t - q) * 256.0f));
    return true;
}

__device__ __forceinline__ unsigned long long wave_key(unsigned long long key, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), lane);
    return (unsigned long long)hi << 32 | lo;
}

template <bool LANE_ATOMICS>
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_fuse_kernel(const VoxelSpanDev* __restrict__ spans, const int n_spans,
                                                                   const VoxelMapDev* __restrict__ maps) {
    const int64_t tile = blockIdx.x;
    int lo = 0, hi = n_spans - 1;                          // the last span that starts at or before this tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (G(spans)[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const VoxelSpanDev sp = G(spans)[lo];
    const VoxelMapDev mp = G(maps)[sp.map];
    const int lane = threadIdx.x & 63;
    const int64_t k = (tile - sp.tile0) * VOXEL_TILE + (int64_t)threadIdx.x;

    bool active = false, outside = false;
    unsigned long long key = VOXEL_EMPTY;
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};                    // ox, oy, oz, r, g, b
    if (k < sp.n) {
        const uint4 r = ((SVO_GP(const uint4))sp.points)[k];
        const uint32_t flags = r.w >> 24;
        if (!(flags & ((uint32_t)SVO_CLOUD_DROPPED | mp.drop_flags))) {
            uint32_t ix = 0, iy = 0, iz = 0;
            const bool in = voxel_coord(__uint_as_float(r.x), mp.voxel, ix, v[0]) && voxel_coord(__uint_as_float(r.y), mp.voxel, iy, v[1]) &&
                            voxel_coord(__uint_as_float(r.z), mp.voxel, iz, v[2]);
            active = in;
            outside = !in;
            if (in) {
                key = (unsigned long long)ix << 42 | (unsigned long long)iy << 21 | iz;
                v[3] = r.w & 255u; v[4] = (r.w >> 8) & 255u; v[5] = (r.w >> 16) & 255u;
            }
        }
    }
    const unsigned long long all_active = __ballot(active);
    const unsigned long long all_outside = __ballot(outside);
    if ((all_active | all_outside) == 0) return;           // (wave-uniform)

    // election: one round per distinct key of the wavefront, the lowest lane of a key leads
    uint32_t p[3] = {v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16};
    bool leader = false;
    uint32_t cnt = 0;
    int my_leader = lane;
    unsigned long long remaining = all_active;
    for (int round = 0; round < 64 && remaining != 0; round++) {
        const int first = __ffsll(remaining) - 1;
        const unsigned long long k0 = wave_key(key, first);
        const bool mine = active && key == k0;
        const unsigned long long same = __ballot(mine);
        if (LANE_ATOMICS) {
            if (mine) my_leader = first;
        } else if (same & (same - 1)) {                    // (wave-uniform) more than one lane: sum the group
            uint32_t s[3];
            for (int j = 0; j < 3; j++) {
                s[j] = mine ? p[j] : 0u;
                for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o);
            }
            if (lane == first) { p[0] = s[0]; p[1] = s[1]; p[2] = s[2]; }
        }
        if (lane == first) { leader = true; cnt = (uint32_t)__popcll(same); }
        remaining &= ~same;
    }

    // leaders find or claim their key's entry: bounded by the capacity, never waiting
    const uint32_t cap = 1u << mp.log2_capacity, mask = cap - 1;
    int slot = -1;
    bool claimed = false;
    if (leader) {
        SVO_GP(unsigned long long) keys = voxel_keys(mp);
        uint32_t s = (uint32_t)((key * VOXEL_HASH) >> (64 - mp.log2_capacity));
        for (uint32_t it = 0; it < cap; it++) {
            unsigned long long cur = __hip_atomic_load(keys + s, VOXEL_RELAXED);
            if (cur == VOXEL_EMPTY) {
                unsigned long long expected = VOXEL_EMPTY;
                if (__hip_atomic_compare_exchange_strong(keys + s, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    claimed = true;
                    cur = key;
                } else {
                    cur = expected;
                }
            }
            if (cur == key) { slot = (int)s; break; }
            s = (s + 1) & mask;
        }
    }
    SVO_GP(uint32_t) acc = voxel_acc(mp);
    if (LANE_ATOMICS) {
        const int at = __shfl(slot, my_leader);
        if (active && at >= 0) {
            SVO_GP(uint32_t) a = acc + (size_t)at * 8;
            __hip_atomic_fetch_add(a + 0, 1u, VOXEL_RELAXED);
            for (int j = 0; j < 6; j++) __hip_atomic_fetch_add(a + 1 + j, v[j], VOXEL_RELAXED);
            __hip_atomic_fetch_max(a + 7, sp.stamp, VOXEL_RELAXED);
        }
    } else if (leader && slot >= 0) {
        SVO_GP(uint32_t) a = acc + (size_t)slot * 8;
        __hip_atomic_fetch_add(a + 0, cnt, VOXEL_RELAXED);
        for (int j = 0; j < 3; j++) {
            __hip_atomic_fetch_add(a + 1 + 2 * j, p[j] & 0xffffu, VOXEL_RELAXED);
            __hip_atomic_fetch_add(a + 2 + 2 * j, p[j] >> 16, VOXEL_RELAXED);
        }
        __hip_atomic_fetch_max(a + 7, sp.stamp, VOXEL_RELAXED);
    }

    // the header's counters: at most one add each per wavefront
    const unsigned long long n_claimed = __popcll(__ballot(claimed));
    unsigned long long lost = __ballot(leader && slot < 0), n_lost = 0;
    while (lost != 0) {                                    // (wave-uniform; the load bound keeps it empty)
        const int l = __ffsll(lost) - 1;
        n_lost += (uint32_t)__builtin_amdgcn_readlane((int)cnt, l);
        lost &= lost - 1;
    }
    if (lane == 0) {
        SVO_GP(VoxelHeader) hd = (SVO_GP(VoxelHeader))mp.base;
        const unsigned long long n_fused = (unsigned long long)__popcll(all_active) - n_lost, n_outside = __popcll(all_outside);
        if (n_claimed) __hip_atomic_fetch_add(&hd->n_voxels, n_claimed, VOXEL_RELAXED);
        if (n_fused) __hip_atomic_fetch_add(&hd->n_fused, n_fused, VOXEL_RELAXED);
        if (n_outside) __hip_atomic_fetch_add(&hd->n_outside, n_outside, VOXEL_RELAXED);
        if (n_lost) __hip_atomic_fetch_add(&hd->overflow, n_lost, VOXEL_RELAXED);
    }
}

// 16-byte unit u of the map: the header block, zeros, all ones over the keys, zeros over the accumulators
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_clear_kernel(const VoxelMapDev mp, const size_t units) {
    const size_t u = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (u >= units) return;
    const size_t key_units = ((size_t)8 << mp.log2_capacity) / 16;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (u == 0) w = make_uint4(VOXEL_MAGIC, (uint32_t)mp.log2_capacity, __float_as_uint(mp.voxel), mp.drop_flags);
    else if (u >= VOXEL_HEADER_BYTES / 16 && u < VOXEL_HEADER_BYTES / 16 + key_units) w = make_uint4(~0u, ~0u, ~0u, ~0u);
    ((SVO_GP(uint4))mp.base)[u] = w;
}

__global__ __launch_bounds__(64) void voxel_headers_kernel(const VoxelMapDev* __restrict__ maps, VoxelHeader* __restrict__ out) {
    static_assert(sizeof(VoxelHeader) == 4 * 16, "four lanes copy a header");
    if (threadIdx.x < 4) ((SVO_GP(uint4))(out + blockIdx.x))[threadIdx.x] = ((SVO_GP(const uint4))G(maps)[blockIdx.x].base)[threadIdx.x];
}

__device__ __forceinline__ bool voxel_keep(const VoxelMapDev& mp, const VoxelFilterDev& f, uint32_t e, unsigned long long& key) {
    key = VOXEL_EMPTY;
    if (e >= (1u << mp.log2_capacity)) return false;
    key = voxel_keys(mp)[e];
    if (key == VOXEL_EMPTY) return false;
    const SVO_GP(uint32_t) a = voxel_acc(mp) + (size_t)e * 8;
    return a[0] >= f.min_count && a[7] >= f.min_stamp;
}

__global__ __launch_bounds__(VOXEL_THREADS) void voxel_count_kernel(const VoxelMapDev mp, const VoxelFilterDev f, int32_t* __restrict__ tile_counts) {
    __shared__ int wave_n[VOXEL_WAVES];
    unsigned long long key;
    const bool keep = voxel_keep(mp, f, blockIdx.x * VOXEL_TILE + threadIdx.x, key);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < VOXEL_WAVES; w++) n += wave_n[w];
        G(tile_counts)[blockIdx.x] = n;
    }
}

// one workgroup: counts[0, tiles) become their exclusive prefix sums in place, counts[tiles] the total
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_scan_kernel(int32_t* __restrict__ counts, const int tiles) {
    __shared__ int part[VOXEL_THREADS];
    const int i = threadIdx.x, per = (tiles + VOXEL_THREADS - 1) / VOXEL_THREADS;
    const int a = min(tiles, i * per), b = min(tiles, a + per);
    int sum = 0;
    for (int j = a; j < b; j++) sum += G(counts)[j];
    part[i] = sum;
    __syncthreads();
    int before = 0, total = 0;
    for (int j = 0; j < VOXEL_THREADS; j++) {
        if (j < i) before += part[j];
        total += part[j];
    }
    for (int j = a; j < b; j++) {
        const int c = G(counts)[j];
        G(counts)[j] = before;
        before += c;
    }
    if (i == 0) G(counts)[tiles] = total;
}

__global__ __launch_bounds__(VOXEL_THREADS) void voxel_pairs_kernel(const VoxelMapDev mp, const VoxelFilterDev f,
                                                                    const int32_t* __restrict__ tile_offsets, const size_t n,
                                                                    unsigned long long* __restrict__ keys_out, uint32_t* __restrict__ index_out) {
    __shared__ int wave_n[VOXEL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t e = blockIdx.x * VOXEL_TILE + threadIdx.x;
    unsigned long long key;
    const bool keep = voxel_keep(mp, f, e, key);
    const unsigned long long m = __ballot(keep);
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    size_t at = (size_t)G(tile_offsets)[blockIdx.x] + rank;
    for (int w = 0; w < wave; w++) at += wave_n[w];
    if (keep && at < n) {                                  // (at < n always: the scan counted the same predicate)
        G(keys_out)[at] = key;
        G(index_out)[at] = e;
    }
}

__global__ __launch_bounds__(VOXEL_THREADS) void voxel_gather_kernel(const VoxelMapDev mp, const size_t n, const unsigned long long* __restrict__ keys,
                                                                     const uint32_t* __restrict__ index, svo_map_point* __restrict__ points) {
    const size_t i = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = G(keys)[i];
    const uint32_t e = G(index)[i] & ((1u << mp.log2_capacity) - 1);
    const SVO_GP(uint4) a = (SVO_GP(uint4))(voxel_acc(mp) + (size_t)e * 8);
    const uint4 lo = a[0], hi = a[1];                      // count sx sy sz | sr sg sb last
    const uint32_t count = max(lo.x, 1u);
    const int cell[3] = {(int)(uint32_t)(key >> 42) - 1048576, (int)(uint32_t)((key >> 21) & 0x1fffffu) - 1048576,
                         (int)(uint32_t)(key & 0x1fffffu) - 1048576};
    const uint32_t off[3] = {lo.y, lo.z, lo.w}, col[3] = {hi.x, hi.y, hi.z};
    uint4 r;
    uint32_t xyz[3], rgb[3];
    for (int j = 0; j < 3; j++) {
        const double mean = (double)off[j] / (double)count;
        const double at = ((double)cell[j] + (mean + 0.5) / 256.0) * (double)mp.voxel;
        xyz[j] = __float_as_uint((float)at);
        rgb[j] = (uint32_t)min((unsigned long long)255, ((unsigned long long)col[j] + count / 2) / count);
    }
    r.x = xyz[0]; r.y = xyz[1]; r.z = xyz[2];
    r.w = rgb[0] | rgb[1] << 8 | rgb[2] << 16;
    ((SVO_GP(uint4))points)[i] = r;
}

// ---- prune: the map rebuilt in place from its kept entries (include/svo_hip.h, "voxel prune")

// the keep rule of a prune on entry e: count, stamp, and the Chebyshev box over the key's three 21-bit parts
__device__ __forceinline__ bool voxel_prune_keep(const VoxelMapDev& mp, const VoxelKeepDev& f, uint32_t e, unsigned long long& key) {
    key = VOXEL_EMPTY;
    if (e >= (1u << mp.log2_capacity)) return false;
    key = voxel_keys(mp)[e];
    if (key == VOXEL_EMPTY) return false;
    const SVO_GP(uint32_t) a = voxel_acc(mp) + (size_t)e * 8;
    if (!(a[0] >= f.min_count && a[7] >= f.min_stamp)) return false;
    if (f.radius < 0) return true;
    const int d[3] = {(int)(uint32_t)(key >> 42) - f.c[0], (int)(uint32_t)((key >> 21) & 0x1fffffu) - f.c[1], (int)(uint32_t)(key & 0x1fffffu) - f.c[2]};
    return abs(d[0]) <= f.radius && abs(d[1]) <= f.radius && abs(d[2]) <= f.radius;
}

// nothing leaves the map: the scan's total is the header's n_voxels (both final before any rebuild kernel starts; the
// header's count is written again only by voxel_prune_finish_kernel, the last launch)
__device__ __forceinline__ bool voxel_prune_nothing_leaves(const VoxelMapDev& mp, const int32_t* __restrict__ tile_offsets, int tiles) {
    return (unsigned long long)G(tile_offsets)[tiles] == ((SVO_GP(const VoxelHeader))mp.base)->n_voxels;
}

// ---- carve (include/svo_hip.h, "voxel carve"): is the non-empty entry e contradicted by the occluder? tested: it reached step 5
__device__ __forceinline__ bool voxel_carved(const VoxelMapDev& mp, const VoxelCarveDev& c, uint32_t e, unsigned long long key, bool& tested) {
    tested = false;
    if (c.records == nullptr) return false;                // (uniform) no evidence anywhere
    const SVO_GP(uint4) a = (SVO_GP(uint4))(voxel_acc(mp) + (size_t)e * 8);
    const uint4 lo = a[0];                                 // count sx sy sz
    const uint32_t last = voxel_acc(mp)[(size_t)e * 8 + 7];
    if (last > c.max_last) return false;
    const uint32_t count = max(lo.x, 1u);
    const int cell[3] = {(int)(uint32_t)(key >> 42) - 1048576, (int)(uint32_t)((key >> 21) & 0x1fffffu) - 1048576,
                         (int)(uint32_t)(key & 0x1fffffu) - 1048576};
    const uint32_t off[3] = {lo.y, lo.z, lo.w};
    float w[3], cam[3];
    for (int j = 0; j < 3; j++) {                          // the gather's point
        const double mean = (double)off[j] / (double)count;
        w[j] = (float)(((double)cell[j] + (mean + 0.5) / 256.0) * (double)mp.voxel);
    }
    for (int k = 0; k < 3; k++) cam[k] = ((c.view[4 * k] * w[0] + c.view[4 * k + 1] * w[1]) + c.view[4 * k + 2] * w[2]) + c.view[4 * k + 3];
    if (!(fabsf(cam[0]) <= FLT_MAX && fabsf(cam[1]) <= FLT_MAX && fabsf(cam[2]) <= FLT_MAX) || cam[2] < c.near) return false;
    const float u = (c.fx * cam[0]) / cam[2] + c.cx, v = (c.fy * cam[1]) / cam[2] + c.cy;
    if (!(u >= 0.0f && u < c.w && v >= 0.0f && v < c.h)) return false;
    const int ix = (int)u / c.step, iy = (int)v / c.step;
    if (ix >= c.cols || iy >= c.rows) return false;
    float zmin = 0.f;
    bool first = true;
    for (int dy = -c.ring; dy <= c.ring; dy++) {           // (ring is 0 or 1: at most nine cells)
        for (int dx = -c.ring; dx <= c.ring; dx++) {
            const int x = ix + dx, y = iy + dy;
            if (x < 0 || y < 0 || x >= c.cols || y >= c.rows) continue;
            const uint4 r = ((SVO_GP(const uint4))c.records)[(size_t)y * c.cols + x];
            const float zo = __uint_as_float(r.z);
            if (((r.w >> 24) & c.drop_flags) || !(zo > 0.f && zo <= FLT_MAX)) return false;   // incomplete evidence
            zmin = first ? zo : fminf(zmin, zo);
            first = false;
        }
    }
    tested = true;
    return cam[2] + c.margin < zmin;
}

// does entry e stay, by the rule of the launch? key: the entry's, VOXEL_EMPTY past the table. The plain prune:
__device__ __forceinline__ bool voxel_rule_stays(const VoxelMapDev& mp, const VoxelKeepDev& f, uint32_t e, unsigned long long& key, bool&, bool&) {
    return voxel_prune_keep(mp, f, e, key);
}
// the carve: kept by the keep rule and not carved; the carve is evaluated on every non-empty entry
__device__ __forceinline__ bool voxel_rule_stays(const VoxelMapDev& mp, const VoxelCarveRule& f, uint32_t e, unsigned long long& key, bool& tested,
                                                 bool& carved) {
    const bool keep = voxel_prune_keep(mp, f.keep, e, key);
    if (key == VOXEL_EMPTY) return false;
    carved = voxel_carved(mp, f.carve, e, key, tested);
    return keep && !carved;
}

template <class Rule>
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_prune_count_kernel(const VoxelMapDev mp, const Rule f, int32_t* __restrict__ tile_counts) {
    __shared__ int wave_n[VOXEL_WAVES];
    unsigned long long key;
    bool tested = false, carved = false;
    const bool keep = voxel_rule_stays(mp, f, blockIdx.x * VOXEL_TILE + threadIdx.x, key, tested, carved);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
    if constexpr (Rule::carves) {                          // the wavefront's verdicts for the stage pass, and the two counts
        __shared__ int wave_t[VOXEL_WAVES], wave_c[VOXEL_WAVES];
        const unsigned long long mt = __ballot(tested), mc = __ballot(carved);
        if ((threadIdx.x & 63) == 0) {
            if (f.ballots) G(f.ballots)[(size_t)blockIdx.x * VOXEL_WAVES + (threadIdx.x >> 6)] = m;
            wave_t[threadIdx.x >> 6] = __popcll(mt);
            wave_c[threadIdx.x >> 6] = __popcll(mc);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0, c = 0;
            for (int w = 0; w < VOXEL_WAVES; w++) { t += wave_t[w]; c += wave_c[w]; }
            if (t) __hip_atomic_fetch_add(f.counters + 0, t, VOXEL_RELAXED);
            if (c) __hip_atomic_fetch_add(f.counters + 1, c, VOXEL_RELAXED);
        }
    } else {
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < VOXEL_WAVES; w++) n += wave_n[w];
        G(tile_counts)[blockIdx.x] = n;
    }
}

// the kept entry of rank r leaves as acc_out[2 r], acc_out[2 r + 1] (two 16-byte stores) and keys_out[r]
template <class Rule>
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_prune_stage_kernel(const VoxelMapDev mp, const Rule f,
                                                                          const int32_t* __restrict__ tile_offsets, const int tiles, const size_t n_bound,
                                                                          uint4* __restrict__ acc_out, unsigned long long* __restrict__ keys_out) {
    __shared__ int wave_n[VOXEL_WAVES];
    if (voxel_prune_nothing_leaves(mp, tile_offsets, tiles)) return;   // (uniform over the grid)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t e = blockIdx.x * VOXEL_TILE + threadIdx.x;
    unsigned long long key, m;
    bool keep;
    if constexpr (Rule::carves) {                          // the count pass's verdicts; a set bit names a non-empty entry of the table
        if (f.ballots) {                                   // (uniform)
            m = G(f.ballots)[(size_t)blockIdx.x * VOXEL_WAVES + wave];
            keep = (m >> lane) & 1;
            key = keep ? voxel_keys(mp)[e] : VOXEL_EMPTY;
        } else {                                           // (the diagnostic form: no words, the rule evaluated again)
            bool tested = false, carved = false;
            keep = voxel_rule_stays(mp, f, e, key, tested, carved);
            m = __ballot(keep);
        }
    } else {
        keep = voxel_prune_keep(mp, f, e, key);
        m = __ballot(keep);
    }
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    size_t at = (size_t)G(tile_offsets)[blockIdx.x] + rank;
    for (int w = 0; w < wave; w++) at += wave_n[w];
    if (keep && at < n_bound) {                            // (at < n_bound always: the kept are among the header's n_voxels)
        const SVO_GP(uint4) a = (SVO_GP(uint4))(voxel_acc(mp) + (size_t)e * 8);
        const uint4 lo = a[0], hi = a[1];
        ((SVO_GP(uint4))acc_out)[2 * at] = lo;
        ((SVO_GP(uint4))acc_out)[2 * at + 1] = hi;
        G(keys_out)[at] = key;
    }
}

// 16-byte unit u behind the header block: all ones over the keys, zeros over the accumulators; the header stays
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_prune_clear_kernel(const VoxelMapDev mp, const size_t units,
                                                                          const int32_t* __restrict__ tile_offsets, const int tiles) {
    if (voxel_prune_nothing_leaves(mp, tile_offsets, tiles)) return;
    const size_t u = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (u >= units) return;
    const size_t key_units = ((size_t)8 << mp.log2_capacity) / 16;
    const uint32_t w = u < key_units ? ~0u : 0u;
    ((SVO_GP(uint4))(mp.base + VOXEL_HEADER_BYTES))[u] = make_uint4(w, w, w, w);
}

// An entry whose key no other lane of the launch holds, into a table that held none of the launch's keys before it: the
// probe of the fuse from the key's home, the claim ~0 -> key (keys are unique: a lane never meets its own key, and an
// entry another lane claimed holds another key for good), then the eight accumulators as two plain 16-byte stores:
// nobody else writes the entry this lane claimed.
__device__ __forceinline__ void voxel_place_unique(const VoxelMapDev& mp, unsigned long long key, uint4 lo, uint4 hi) {
    const uint32_t cap = 1u << mp.log2_capacity, mask = cap - 1;
    SVO_GP(unsigned long long) keys = voxel_keys(mp);
    uint32_t s = (uint32_t)((key * VOXEL_HASH) >> (64 - mp.log2_capacity));
    for (uint32_t it = 0; it < cap; it++) {
        if (__hip_atomic_load(keys + s, VOXEL_RELAXED) == VOXEL_EMPTY) {
            unsigned long long expected = VOXEL_EMPTY;
            if (__hip_atomic_compare_exchange_strong(keys + s, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                SVO_GP(uint4) a = (SVO_GP(uint4))(voxel_acc(mp) + (size_t)s * 8);
                a[0] = lo;
                a[1] = hi;
                return;
            }
        }
        s = (s + 1) & mask;
    }
    // (not reached: the cleared table has `capacity` empty entries for at most n_voxels <= capacity keys)
}

// One lane per staged entry, placed by voxel_place_unique.
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_prune_reinsert_kernel(const VoxelMapDev mp, const int32_t* __restrict__ tile_offsets, const int tiles,
                                                                             const size_t n_bound, const uint4* __restrict__ acc_in,
                                                                             const unsigned long long* __restrict__ keys_in) {
    if (voxel_prune_nothing_leaves(mp, tile_offsets, tiles)) return;
    const size_t i = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    const size_t n = min((size_t)max(G(tile_offsets)[tiles], 0), n_bound);
    if (i >= n) return;
    const unsigned long long key = G(keys_in)[i];
    const uint4 lo = ((SVO_GP(const uint4))acc_in)[2 * i], hi = ((SVO_GP(const uint4))acc_in)[2 * i + 1];
    voxel_place_unique(mp, key, lo, hi);
}

// the last launch of a prune: the header's n_voxels becomes the kept count
__global__ __launch_bounds__(64) void voxel_prune_finish_kernel(const VoxelMapDev mp, const int32_t* __restrict__ tile_offsets, const int tiles) {
    if (threadIdx.x != 0 || voxel_prune_nothing_leaves(mp, tile_offsets, tiles)) return;
    ((SVO_GP(VoxelHeader))mp.base)->n_voxels = (unsigned long long)max(G(tile_offsets)[tiles], 0);
}

// ---- entries (include/svo_hip.h, "voxel entries"): the raw entries packed out in key order, merged in, rehashed

// the pack's gather: the kept entry of rank i in key order leaves as entries[i], five 8-byte stores (a record is
// 8-byte aligned, no more)
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_pack_kernel(const VoxelMapDev mp, const size_t n, const unsigned long long* __restrict__ keys,
                                                                   const uint32_t* __restrict__ index, svo_voxel_entry* __restrict__ entries) {
    const size_t i = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = G(keys)[i];
    const uint32_t e = G(index)[i] & ((1u << mp.log2_capacity) - 1);
    const SVO_GP(uint4) a = (SVO_GP(uint4))(voxel_acc(mp) + (size_t)e * 8);
    const uint4 lo = a[0], hi = a[1];                      // count sx sy sz | sr sg sb last
    SVO_GP(uint2) out = (SVO_GP(uint2))(entries + i);
    out[0] = make_uint2((uint32_t)key, (uint32_t)(key >> 32));
    out[1] = make_uint2(lo.x, lo.y);
    out[2] = make_uint2(lo.z, lo.w);
    out[3] = make_uint2(hi.x, hi.y);
    out[4] = make_uint2(hi.z, hi.w);
}

// A workgroup takes VOXEL_TILE consecutive records of one span (the fuse's search of tile0), a lane one record. No
// leader is elected among equal keys: the records of a pack have unique keys, and where keys do repeat (across spans,
// or in a span a caller made) every update below is an atomic, so the lanes simply meet at the entry. A lane that
// claimed an entry adds like every other: a second lane with the same key can find the claimed key and add before
// the claimer's first add lands, and plain stores would lose that.
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_merge_kernel(const VoxelEntrySpanDev* __restrict__ spans, const int n_spans,
                                                                    const VoxelMapDev* __restrict__ maps, VoxelMergeCounts* __restrict__ counts) {
    const int64_t tile = blockIdx.x;
    int lo = 0, hi = n_spans - 1;                          // the last span that starts at or before this tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (G(spans)[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const VoxelEntrySpanDev sp = G(spans)[lo];
    const VoxelMapDev mp = G(maps)[sp.map];
    const int lane = threadIdx.x & 63;
    const int64_t k = (tile - sp.tile0) * VOXEL_TILE + (int64_t)threadIdx.x;

    const bool offered = k < sp.n;
    unsigned long long key = VOXEL_EMPTY;
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (offered) {
        SVO_GP(const uint2) r =(SVO_GP(const uint2))(sp.entries + k);
        const uint2 w0 = r[0], w1 = r[1], w2 = r[2], w3 = r[3], w4 = r[4];
        key = (unsigned long long)w0.y << 32 | w0.x;
        v[0] = w1.x; v[1] = w1.y; v[2] = w2.x; v[3] = w2.y; v[4] = w3.x; v[5] = w3.y; v[6] = w4.x; v[7] = w4.y;
    }
    const bool active = offered && !(key >> 63) && v[0] != 0;
    const unsigned long long all_offered = __ballot(offered);
    if (all_offered == 0) return;                          // (wave-uniform)

    // find or claim the key's entry: bounded by the capacity, never waiting
    const uint32_t cap = 1u << mp.log2_capacity, mask = cap - 1;
    int slot = -1;
    bool claimed = false;
    if (active) {
        SVO_GP(unsigned long long) keys = voxel_keys(mp);
        uint32_t s = (uint32_t)((key * VOXEL_HASH) >> (64 - mp.log2_capacity));
        for (uint32_t it = 0; it < cap; it++) {
            unsigned long long cur = __hip_atomic_load(keys + s, VOXEL_RELAXED);
            if (cur == VOXEL_EMPTY) {
                unsigned long long expected = VOXEL_EMPTY;
                if (__hip_atomic_compare_exchange_strong(keys + s, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    claimed = true;
                    cur = key;
                } else {
                    cur = expected;
                }
            }
            if (cur == key) { slot = (int)s; break; }
            s = (s + 1) & mask;
        }
    }
    const bool merged = active && slot >= 0;
    if (merged) {
        SVO_GP(uint32_t) a = voxel_acc(mp) + (size_t)slot * 8;
        for (int j = 0; j < 7; j++) __hip_atomic_fetch_add(a + j, v[j], VOXEL_RELAXED);
        __hip_atomic_fetch_max(a + 7, v[7], VOXEL_RELAXED);
    }

    // the header's counters and the call's: at most one add each per wavefront
    unsigned long long fused = merged ? v[0] : 0u;         // the 64-bit sum of the merged counts
    for (int o = 32; o > 0; o >>= 1) fused += __shfl_xor(fused, o);
    const unsigned long long n_offered = __popcll(all_offered), n_merged = __popcll(__ballot(merged)), n_skipped = __popcll(__ballot(offered && !active)),
                             n_claimed = __popcll(__ballot(claimed)), n_lost = __popcll(__ballot(active && slot < 0));
    if (lane == 0) {
        SVO_GP(VoxelHeader) hd = (SVO_GP(VoxelHeader))mp.base;
        if (n_claimed) __hip_atomic_fetch_add(&hd->n_voxels, n_claimed, VOXEL_RELAXED);
        if (fused) __hip_atomic_fetch_add(&hd->n_fused, fused, VOXEL_RELAXED);
        if (n_lost) __hip_atomic_fetch_add(&hd->overflow, n_lost, VOXEL_RELAXED);   // (the load bound keeps it 0)
        SVO_GP(VoxelMergeCounts) c = G(counts) + sp.map;
        __hip_atomic_fetch_add(&c->n_offered, n_offered, VOXEL_RELAXED);
        if (n_merged) __hip_atomic_fetch_add(&c->n_merged, n_merged, VOXEL_RELAXED);
        if (n_skipped) __hip_atomic_fetch_add(&c->n_skipped, n_skipped, VOXEL_RELAXED);
        if (n_claimed) __hip_atomic_fetch_add(&c->n_claimed, n_claimed, VOXEL_RELAXED);
    }
}

// One lane per entry of the source table: a non-empty entry goes into dst by voxel_place_unique. That is right here:
// the keys of one table are unique, and dst was cleared by the launch before this one and belongs to this call alone.
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_rehash_kernel(const VoxelMapDev src, const VoxelMapDev dst) {
    const uint32_t e = blockIdx.x * VOXEL_TILE + threadIdx.x;
    if (e >= (1u << src.log2_capacity)) return;
    const unsigned long long key = voxel_keys(src)[e];
    if (key == VOXEL_EMPTY) return;
    const SVO_GP(uint4) a = (SVO_GP(uint4))(voxel_acc(src) + (size_t)e * 8);
    const uint4 lo = a[0], hi = a[1];
    voxel_place_unique(dst, key, lo, hi);
}

// the last launch of a rehash: the four counters of the source header, as they are, into the cleared header of dst
__global__ __launch_bounds__(64) void voxel_rehash_finish_kernel(const VoxelMapDev src, const VoxelMapDev dst) {
    if (threadIdx.x != 0) return;
    SVO_GP(const VoxelHeader) from =(SVO_GP(const VoxelHeader))src.base;
    SVO_GP(VoxelHeader) to = (SVO_GP(VoxelHeader))dst.base;
    to->n_voxels = from->n_voxels;
    to->n_fused = from->n_fused;
    to->n_outside = from->n_outside;
    to->overflow = from->overflow;
}

template <class Rule>
static void launch_voxel_rebuild(const VoxelMapDev& map, const Rule& rule, int32_t* tile_offsets, uint8_t* staging, uint64_t n_bound, hipStream_t stream) {
    const int tiles = (int)voxel_map_tiles(map.log2_capacity);
    hipLaunchKernelGGL(voxel_prune_count_kernel<Rule>, dim3(tiles), dim3(VOXEL_THREADS), 0, stream, map, rule, tile_offsets);
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(VOXEL_THREADS), 0, stream, tile_offsets, tiles);
    VoxelPrunePlan plan;
    if (n_bound == 0 || !voxel_prune_plan(n_bound, plan)) return;   // (an empty map keeps nothing; the callers check the plan first)
    uint4* acc = reinterpret_cast<uint4*>(staging + plan.acc);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(staging + plan.keys);
    const size_t units = (voxel_map_bytes(map.log2_capacity) - VOXEL_HEADER_BYTES) / 16;
    hipLaunchKernelGGL(voxel_prune_stage_kernel<Rule>, dim3(tiles), dim3(VOXEL_THREADS), 0, stream, map, rule, tile_offsets, tiles, (size_t)n_bound, acc, keys);
    hipLaunchKernelGGL(voxel_prune_clear_kernel, dim3((unsigned)((units + VOXEL_THREADS - 1) / VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, stream, map,
                       units, tile_offsets, tiles);
    hipLaunchKernelGGL(voxel_prune_reinsert_kernel, dim3((unsigned)voxel_prune_tiles(n_bound)), dim3(VOXEL_THREADS), 0, stream, map, tile_offsets,
                       tiles, (size_t)n_bound, acc, keys);
    hipLaunchKernelGGL(voxel_prune_finish_kernel, dim3(1), dim3(64), 0, stream, map, tile_offsets, tiles);
}

void launch_voxel_prune(const VoxelMapDev& map, VoxelKeepDev keep, int32_t* tile_offsets, uint8_t* staging, uint64_t n_bound,
                        hipStream_t stream) {
    launch_voxel_rebuild(map, keep, tile_offsets, staging, n_bound, stream);
}

void launch_voxel_carve(const VoxelMapDev& map, const VoxelCarveRule& rule, int32_t* tile_offsets, uint8_t* staging, uint64_t n_bound,
                        hipStream_t stream) {
    (void)hipMemsetAsync(rule.counters, 0, 2 * sizeof(unsigned long long), stream);   // (a failure is sticky: the caller's hipGetLastError sees it)
    launch_voxel_rebuild(map, rule, tile_offsets, staging, n_bound, stream);
}

void launch_voxel_clear(const VoxelMapDev& map, hipStream_t stream) {
    const size_t units = voxel_map_bytes(map.log2_capacity) / 16;
    hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)((units + VOXEL_THREADS - 1) / VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, stream, map, units);
}

void launch_voxel_headers(const VoxelMapDev* d_maps, int n, VoxelHeader* d_headers, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(voxel_headers_kernel, dim3(n), dim3(64), 0, stream, d_maps, d_headers);
}

void launch_voxel_fuse(const VoxelSpanDev* d_spans, int n_spans, int64_t tiles, const VoxelMapDev* d_maps, bool lane_atomics,
                       hipStream_t stream) {
    if (n_spans <= 0 || tiles <= 0) return;
    if (lane_atomics) hipLaunchKernelGGL(voxel_fuse_kernel<true>, dim3((unsigned)tiles), dim3(VOXEL_THREADS), 0, stream, d_spans, n_spans, d_maps);
    else hipLaunchKernelGGL(voxel_fuse_kernel<false>, dim3((unsigned)tiles), dim3(VOXEL_THREADS), 0, stream, d_spans, n_spans, d_maps);
}

void launch_voxel_count(const VoxelMapDev& map, VoxelFilterDev f, int32_t* tile_offsets, hipStream_t stream) {
    const int tiles = (int)voxel_map_tiles(map.log2_capacity);
    hipLaunchKernelGGL(voxel_count_kernel, dim3(tiles), dim3(VOXEL_THREADS), 0, stream, map, f, tile_offsets);
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(VOXEL_THREADS), 0, stream, tile_offsets, tiles);
}

int voxel_sort_temp_bytes(size_t n, size_t* bytes) {
    *bytes = 0;
    if (n == 0) return SVO_OK;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, *bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr,
                                      (uint32_t*)nullptr, n, 0, 63, (hipStream_t) nullptr));
    return SVO_OK;
}

// the (key, entry) pairs of the n > 0 kept entries, sorted by key: what the extraction and the pack gather from
static int launch_voxel_sorted_pairs(const VoxelMapDev& map, VoxelFilterDev f, const int32_t* tile_offsets, size_t n, uint64_t* keys_in,
                                     uint64_t* keys_out, uint32_t* index_in, uint32_t* index_out, void* sort_temp, size_t sort_temp_bytes,
                                     hipStream_t stream) {
    const int tiles = (int)voxel_map_tiles(map.log2_capacity);
    hipLaunchKernelGGL(voxel_pairs_kernel, dim3(tiles), dim3(VOXEL_THREADS), 0, stream, map, f, tile_offsets, n,
                       (unsigned long long*)keys_in, index_in);
    HIP_TRY(rocprim::radix_sort_pairs(sort_temp, sort_temp_bytes, (unsigned long long*)keys_in, (unsigned long long*)keys_out, index_in,
                                      index_out, n, 0, 63, stream));
    return SVO_OK;
}

int launch_voxel_extract(const VoxelMapDev& map, VoxelFilterDev f, const int32_t* tile_offsets, size_t n, uint64_t* keys_in,
                         uint64_t* keys_out, uint32_t* index_in, uint32_t* index_out, void* sort_temp, size_t sort_temp_bytes,
                         svo_map_point* points, hipStream_t stream) {
    if (n == 0) return SVO_OK;
    if (const int rc = launch_voxel_sorted_pairs(map, f, tile_offsets, n, keys_in, keys_out, index_in, index_out, sort_temp, sort_temp_bytes, stream))
        return rc;
    hipLaunchKernelGGL(voxel_gather_kernel, dim3((unsigned)((n + VOXEL_THREADS - 1) / VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, stream, map, n,
                       (const unsigned long long*)keys_out, index_out, points);
    return SVO_OK;
}

int launch_voxel_pack(const VoxelMapDev& map, VoxelFilterDev f, const int32_t* tile_offsets, size_t n, uint64_t* keys_in,
                      uint64_t* keys_out, uint32_t* index_in, uint32_t* index_out, void* sort_temp, size_t sort_temp_bytes,
                      svo_voxel_entry* entries, hipStream_t stream) {
    if (n == 0) return SVO_OK;
    if (const int rc = launch_voxel_sorted_pairs(map, f, tile_offsets, n, keys_in, keys_out, index_in, index_out, sort_temp, sort_temp_bytes, stream))
        return rc;
    hipLaunchKernelGGL(voxel_pack_kernel, dim3((unsigned)((n + VOXEL_THREADS - 1) / VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, stream, map, n,
                       (const unsigned long long*)keys_out, index_out, entries);
    return SVO_OK;
}

void launch_voxel_merge(const VoxelEntrySpanDev* d_spans, int n_spans, int64_t tiles, const VoxelMapDev* d_maps, VoxelMergeCounts* d_counts,
                        hipStream_t stream) {
    if (n_spans <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(voxel_merge_kernel, dim3((unsigned)tiles), dim3(VOXEL_THREADS), 0, stream, d_spans, n_spans, d_maps, d_counts);
}

void launch_voxel_rehash(const VoxelMapDev& src, const VoxelMapDev& dst, hipStream_t stream) {
    launch_voxel_clear(dst, stream);
    hipLaunchKernelGGL(voxel_rehash_kernel, dim3((unsigned)voxel_map_tiles(src.log2_capacity)), dim3(VOXEL_THREADS), 0, stream, src, dst);
    hipLaunchKernelGGL(voxel_rehash_finish_kernel, dim3(1), dim3(64), 0, stream, src, dst);
}

}  // namespace svo
