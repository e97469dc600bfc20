// ssd_common.hpp — what ssd_disparity_kernel (depth.hip) shares with the kernel it replaced, which svo_capi_check.hip
// keeps as the reference of svo_ssd_disparity_check: the pixel-chunk loads and the tile layout.
#pragma once
#include "svo_kernels.hpp"

namespace svo {

// 4 consecutive pixels of row y starting at column x as one (possibly unaligned)
// dword load, cut to `valid` bytes; byte loads only where the dword would run
// past the end of the image row
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
__device__ inline uint32_t load_u8x4(const ImgView& im, int y, int x, int valid) {
    const uint8_t* src = im.g() + (size_t)y * im.stride + x;
    uint32_t v;
    if (x + 4 <= im.w) {
        v = *reinterpret_cast<const u32_unaligned*>(src);
    } else {
        v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (x + b < im.w) v |= (uint32_t)src[b] << (8 * b);
    }
    if (valid < 4) v &= (1u << (8 * valid)) - 1u;
    return v;
}

// the two halves of load_u8x16. The loads: one 16-byte load when the row has them (x + 16 <= im.w), dwords otherwise
__device__ inline uint4 load_u8x16_whole(const ImgView& im, int y, int x) {
    uint32_t w[4];
    const uint8_t* src = im.g() + (size_t)y * im.stride + x;
    __builtin_memcpy(w, src, 16);                         // (one global_load_dwordx4: any byte alignment)
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ inline uint4 load_u8x16_edge(const ImgView& im, int y, int x) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = load_u8x4(im, y, x + 4 * k, 4);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// and what is made of them: every valid byte ^ (flip & 0xff), bytes from `valid` on = (pad & 0xff)
__device__ inline uint4 finish_u8x16(uint4 raw, int valid, uint32_t flip, uint32_t pad) {
    uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int nv = valid - 4 * k;                     // valid bytes of this dword
        const uint32_t vm = nv >= 4 ? 0xFFFFFFFFu : (nv <= 0 ? 0u : ((1u << (8 * nv)) - 1u));
        w[k] = ((w[k] ^ flip) & vm) | (pad & ~vm);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// 16 consecutive pixels of row y starting at column x (any alignment), every valid byte ^ (flip & 0xff),
// bytes from `valid` on = (pad & 0xff)
__device__ inline uint4 load_u8x16(const ImgView& im, int y, int x, int valid, uint32_t flip, uint32_t pad) {
    return finish_u8x16(x + 16 <= im.w ? load_u8x16_whole(im, y, x) : load_u8x16_edge(im, y, x), valid, flip, pad);
}

constexpr int SSD_WIN_ALL = 35, SSD_MH_ALL = 17; // template edge and match-map rows (2*search_y+1) the entry points accept
constexpr int SSD_MAX_MW = 65;                  // match-map columns (search_x+1)
constexpr int SSD_T_STRIDE = 96;                // bytes per padded template row: 16 zeros | row | zeros
constexpr int SSD_R_STRIDE = 144;               // bytes per search-region row (36 dwords: conflict-free b128 rows)

typedef int ssd_v4i __attribute__((ext_vector_type(4)));

// the four-wave kernel that ssd_disparity_kernel replaced (svo_capi_check.hip), launched like it: grid (max_n, batch)
void launch_ssd_ref(const SsdArgs* d_args, int batch, int max_n, int win, int search_y, hipStream_t stream);

}  // namespace svo
