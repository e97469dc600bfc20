// snapshot.hip — many 2-D byte segments copied device to device in one launch: the data path of saving and
// loading a slot's sequence state (svo_submit_save / svo_submit_load, svo_group_snapshot.hip) and of svo_copy_segments.
// The reference has no checkpoint or resume; a snapshot's data part is the image pyramids of the live
// keyframes, the keypoint arrays of the frame and of every keyframe and two words, scattered over image sets,
// keyframe slabs and per-sequence arrays on one side and packed behind offsets on the other. One kernel does both
// directions: the host, which knows every size, writes the segments (svo_copy_segment: src, dst, row_bytes, rows
// and the two pitches) and cuts them into tiles of at most COPY_TILE_BYTES, so the grid is flat and a 361 KB
// image plane and a 33-entry array cost their share.
//
// A tile is itself a small 2-D segment (rows x row_bytes <= COPY_TILE_BYTES unless it is a single row piece). A
// segment whose rows follow each other without a gap on both sides is one long row; a row longer than a tile is
// cut into pieces at multiples of COPY_TILE_BYTES from its start. A workgroup of 256 lanes takes one tile and
// picks the widest unit that source, destination and both pitches allow for every row of the tile alike:
//
//  * 16 bytes per lane when source and destination agree modulo 16 and (more than one row) both pitches are
//    multiples of 16: every row then has the same head (the bytes up to the destination's next 16-byte boundary),
//    body (whole uint4) and tail;
//  * dwords under the same rule modulo 4;
//  * bytes otherwise.
//
// The bodies of all rows are one flat index space (unit k of row r: lanes never idle on short rows), and so are
// the heads and tails, which go byte by byte. The kernel only moves bytes (no LDS, no reduction); its roof is HBM.
//
// Bounds: of a tile exactly [src + r * src_pitch, + row_bytes) is read for r in [0, rows) and the matching
// destination bytes are written, nothing else; rows or row_bytes of 0 make no tile at all.
#include <algorithm>

#include "svo_tracker.hpp"

namespace svo {

constexpr int COPY_THREADS = 256;

void cut_copy_tiles(const void* src, void* dst, int64_t row_bytes, int64_t rows, int64_t src_pitch, int64_t dst_pitch,
                    std::vector<CopyTile>& out) {
    if (row_bytes <= 0 || rows <= 0) return;
    if (rows > 1 && src_pitch == row_bytes && dst_pitch == row_bytes) {      // dense on both sides: one long row
        row_bytes *= rows;
        rows = 1;
    }
    const uint8_t* s = static_cast<const uint8_t*>(src);
    uint8_t* d = static_cast<uint8_t*>(dst);
    if (row_bytes >= COPY_TILE_BYTES) {
        for (int64_t r = 0; r < rows; r++)
            for (int64_t x = 0; x < row_bytes; x += COPY_TILE_BYTES)
                out.push_back(CopyTile{s + r * src_pitch + x, d + r * dst_pitch + x, src_pitch, dst_pitch,
                                       (int)std::min<int64_t>(COPY_TILE_BYTES, row_bytes - x), 1});
        return;
    }
    const int64_t per_tile = COPY_TILE_BYTES / row_bytes;
    for (int64_t r = 0; r < rows; r += per_tile)
        out.push_back(CopyTile{s + r * src_pitch, d + r * dst_pitch, src_pitch, dst_pitch, (int)row_bytes,
                               (int)std::min<int64_t>(per_tile, rows - r)});
}

// the rows of a tile in units of sizeof(V) bytes after a head of `head` bytes each; returns the bytes of a row
// that went as units
template <typename V>
__device__ __forceinline__ int copy_body(SVO_GP(const uint8_t) src, SVO_GP(uint8_t) dst, int64_t sp, int64_t dp,
                                         int rows, int head, int units) {
    const unsigned total = (unsigned)rows * (unsigned)units;
    for (unsigned k = threadIdx.x; k < total; k += COPY_THREADS) {
        const unsigned r = k / (unsigned)units, u = k - r * (unsigned)units;
        *(SVO_GP(V))(dst + r * dp + head + (int64_t)u * sizeof(V)) =
            *(SVO_GP(const V))(src + r * sp + head + (int64_t)u * sizeof(V));
    }
    return units * (int)sizeof(V);
}

__global__ __launch_bounds__(COPY_THREADS) void copy_segments_kernel(const CopyTile* __restrict__ tiles) {
    const CopyTile t = G(tiles)[blockIdx.x];
    SVO_GP(const uint8_t) src = (SVO_GP(const uint8_t))t.src;
    SVO_GP(uint8_t) dst = (SVO_GP(uint8_t))t.dst;
    const int w = t.row_bytes, rows = t.rows;
    const uintptr_t diff = (uintptr_t)t.src ^ (uintptr_t)t.dst;
    const uintptr_t pitches = rows > 1 ? (uintptr_t)t.src_pitch | (uintptr_t)t.dst_pitch : 0;
    const int unit = ((diff | pitches) & 15) == 0 ? 16 : ((diff | pitches) & 3) == 0 ? 4 : 1;
    // every row: head | body of whole units | tail. (-dst) mod unit is the same for every row: the pitches are
    // multiples of the unit
    const int head = unit == 1 ? 0 : min(w, (int)((unit - ((uintptr_t)t.dst & (unit - 1))) & (unit - 1)));
    int body = 0;
    if (unit == 16) body = copy_body<uint4>(src, dst, t.src_pitch, t.dst_pitch, rows, head, (w - head) >> 4);
    else if (unit == 4) body = copy_body<uint32_t>(src, dst, t.src_pitch, t.dst_pitch, rows, head, (w - head) >> 2);
    const int rest = w - body;                   // head + tail bytes of a row (unit 1: the whole row)
    const unsigned total = (unsigned)rows * (unsigned)rest;
    for (unsigned k = threadIdx.x; k < total; k += COPY_THREADS) {
        const unsigned r = k / (unsigned)rest, b = k - r * (unsigned)rest;
        const int x = (int)b < head ? (int)b : (int)b + body;
        dst[r * t.dst_pitch + x] = src[r * t.src_pitch + x];
    }
}

void launch_copy_tiles(const CopyTile* d_tiles, int n_tiles, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(copy_segments_kernel, dim3(n_tiles), dim3(COPY_THREADS), 0, stream, d_tiles);
}

}  // namespace svo
