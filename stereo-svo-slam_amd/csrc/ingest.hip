// ingest.hip — the per-pixel step the reference's ImageInput classes do before StereoSlam::new_image sees
// two 8-bit gray images (VideoInput, src/app/video_input.cpp:29-36; EconInput, src/app/econ_input.cpp:102-103).
// The arithmetic (the whole contract):
//
//  * gray from colour: Y = (3735 B + 19235 G + 9798 R + 2^14) >> 15 — OpenCV 4.x RGB2Gray<uchar>, 15-bit
//    coefficients with CV_DESCALE. The weights sum to 2^15, so R = G = B = v gives v, and the sum never exceeds
//    255 * 2^15 + 2^14 = 8372224 < 2^24: 24-bit multiply-adds are exact. (The older 14-bit table 1868 / 9617 /
//    4899 is not implemented.)
//  * channel extract: a byte copy of channel k of an interleaved 3-channel pixel.
//  * side by side: for an output width W, `right` = columns 0 .. W-1 and `left` = columns W .. 2W-1 of the
//    frame (image_width = frame_width / 2, video_input.cpp:33-36). Converting the frame and then splitting it
//    gives the same values as converting each half.
//
// One streaming kernel over a table of output images (IngestImg): a source view, the byte step per source pixel
// (1 or 3), the start column, and the operation (copy channel k, or gray with three weights). The input formats
// of the C ABI are rows of the host table below. A lane makes 16 consecutive pixels of an output row:
//
//  * aligned path (source rows dword aligned from the start column on, output rows 16-byte aligned, the 16
//    pixels inside the row): three 16-byte loads (colour) or one (gray), one 16-byte store; the channels of four
//    pixels are picked out of three dwords with v_perm_b32, the weighted sum is three v_mad_u32_u24. No LDS, no
//    barrier;
//  * byte path (everything else: unaligned bases, odd strides, row tails): pixel by pixel.
//
// Every address either path forms lies inside the `w` pixels of the row it was given: source bytes
// (col0 + x) * step .. + step - 1 for 0 <= x < w, output bytes 0 .. w - 1.
#include "svo_kernels.hpp"

#include <algorithm>

namespace svo {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_ROWS = 16;            // output rows of one workgroup row block (blockIdx.y)
constexpr int INGEST_PX = 16;              // output pixels of a lane

// cvtColor's 15-bit table, by channel of a B, G, R pixel
constexpr int GRAY_B = 3735, GRAY_G = 19235, GRAY_R = 9798;
static_assert(GRAY_B + GRAY_G + GRAY_R == 1 << 15, "the weights sum to 2^15");
static_assert(255 * (GRAY_B + GRAY_G + GRAY_R) + (1 << 14) < 1 << 24, "24-bit multiply-adds are exact");

namespace {

constexpr IngestSide copy_of(int buffer, int start, int channel) { return IngestSide{buffer, start, INGEST_COPY, channel, {0, 0, 0}}; }
constexpr IngestSide gray_of(int buffer, int start, bool rgb) {
    return IngestSide{buffer, start, INGEST_GRAY, 0, {rgb ? GRAY_R : GRAY_B, GRAY_G, rgb ? GRAY_B : GRAY_R}};
}

// the input formats (SVO_INPUT_*): buffers per sequence, channels, the left image, the right image
constexpr IngestFormat FORMATS[] = {
    {2, 1, copy_of(0, 0, 0), copy_of(1, 0, 0)},            // GRAY_PAIR
    {2, 3, gray_of(0, 0, false), gray_of(1, 0, false)},    // BGR_PAIR
    {2, 3, gray_of(0, 0, true), gray_of(1, 0, true)},      // RGB_PAIR
    {1, 1, copy_of(0, 1, 0), copy_of(0, 0, 0)},            // SBS_GRAY: right = left half, left = right half
    {1, 3, gray_of(0, 1, false), gray_of(0, 0, false)},    // SBS_BGR
    {1, 3, gray_of(0, 1, true), gray_of(0, 0, true)},      // SBS_RGB
    {1, 3, copy_of(0, 0, 2), copy_of(0, 0, 1)},            // CH3_ECON: right = channel 1, left = channel 2
};

}  // namespace

const IngestFormat* ingest_format(int format) {
    return format >= 0 && format < (int)(sizeof(FORMATS) / sizeof(FORMATS[0])) ? &FORMATS[format] : nullptr;
}

int ingest_row_pixels(const IngestFormat& f, int w) { return w * (1 + std::max(f.left.start, f.right.start)); }

IngestImg ingest_image(const IngestFormat& f, int side, const uint8_t* buffer, int stride, const ImgView& dst) {
    const IngestSide& s = side ? f.right : f.left;
    IngestImg im;
    im.src = ImgView{buffer, dst.w, dst.h, stride};
    im.dst = dst;
    im.step = f.channels;
    im.col0 = s.start * dst.w;
    im.op = s.op;
    im.channel = s.channel;
    for (int i = 0; i < 3; i++) im.weight[i] = s.weight[i];
    return im;
}

// a 16-byte load from a dword-aligned address
typedef uint32_t dword4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// channel C of the four 3-byte pixels in the dwords a, b, c (bytes C, 3 + C, 6 + C, 9 + C of the twelve), as
// the four bytes of one dword: two v_perm_b32 (selector 0-3: a byte of the second operand, 4-7: of the first)
template <int C>
__device__ __forceinline__ uint32_t pick_channel(uint32_t a, uint32_t b, uint32_t c) {
    constexpr uint32_t sel_ab = (uint32_t)C | (uint32_t)(3 + C) << 8 | (uint32_t)(C < 2 ? 6 + C : 0) << 16;
    constexpr uint32_t sel_c = 0u | 1u << 8 | (uint32_t)(C < 2 ? 2 : 4) << 16 | (uint32_t)(5 + C) << 24;
    return __builtin_amdgcn_perm(c, __builtin_amdgcn_perm(b, a, sel_ab), sel_c);
}

__device__ __forceinline__ uint32_t gray_of_pixel(uint32_t c0, uint32_t c1, uint32_t c2, const IngestImg& im) {
    return (__umul24(c0, (uint32_t)im.weight[0]) + __umul24(c1, (uint32_t)im.weight[1]) +
            __umul24(c2, (uint32_t)im.weight[2]) + (1u << 14)) >> 15;
}

// four output pixels from the three dwords of their source pixels
__device__ __forceinline__ uint32_t ingest_four(uint32_t a, uint32_t b, uint32_t c, const IngestImg& im) {
    const uint32_t p0 = pick_channel<0>(a, b, c), p1 = pick_channel<1>(a, b, c), p2 = pick_channel<2>(a, b, c);
    if (im.op == INGEST_COPY) return im.channel == 0 ? p0 : im.channel == 1 ? p1 : p2;
    uint32_t out = 0;
    for (int i = 0; i < 4; i++)
        out |= gray_of_pixel((p0 >> (8 * i)) & 0xffu, (p1 >> (8 * i)) & 0xffu, (p2 >> (8 * i)) & 0xffu, im) << (8 * i);
    return out;
}

__global__ __launch_bounds__(INGEST_THREADS) void ingest_kernel(const IngestImg* __restrict__ imgs, int chunks) {
    const IngestImg im = G(imgs)[blockIdx.z];
    const int t = blockIdx.x * INGEST_THREADS + threadIdx.x;
    const int r = t / chunks;
    const int y = blockIdx.y * INGEST_ROWS + r;
    const int x0 = (t - r * chunks) * INGEST_PX;
    const int w = im.dst.w;
    if (r >= INGEST_ROWS || y >= im.dst.h || x0 >= w) return;
    // the row from its start column on, and this lane's pixels in it
    SVO_GP(const uint8_t) srow = im.src.g() + (size_t)y * im.src.stride + (size_t)im.col0 * im.step;
    SVO_GP(uint8_t) drow = im.dst.gw() + (size_t)y * im.dst.stride;
    const bool aligned = (((uintptr_t)(im.src.data + (size_t)im.col0 * im.step) | (uintptr_t)im.src.stride) & 3) == 0 &&
                         (((uintptr_t)im.dst.data | (uintptr_t)im.dst.stride) & 15) == 0;
    if (aligned && x0 + INGEST_PX <= w) {
        uint4 out;
        if (im.step == 1) {
            const dword4_a4 v = *(SVO_GP(const dword4_a4))(srow + x0);
            out = make_uint4(v.x, v.y, v.z, v.w);
        } else {
            SVO_GP(const dword4_a4) p = (SVO_GP(const dword4_a4))(srow + (size_t)x0 * 3);
            const dword4_a4 u = p[0], v = p[1], s = p[2];
            out = make_uint4(ingest_four(u.x, u.y, u.z, im), ingest_four(u.w, v.x, v.y, im),
                             ingest_four(v.z, v.w, s.x, im), ingest_four(s.y, s.z, s.w, im));
        }
        *(SVO_GP(uint4))(drow + x0) = out;
        return;
    }
    const int x1 = min(x0 + INGEST_PX, w);
    for (int x = x0; x < x1; x++) {
        SVO_GP(const uint8_t) p = srow + (size_t)x * im.step;
        drow[x] = im.op == INGEST_COPY ? p[im.channel] : (uint8_t)gray_of_pixel(p[0], p[1], p[2], im);
    }
}

void launch_ingest(const IngestImg* d_imgs, int n, int w, int h, hipStream_t stream) {
    const int chunks = (w + INGEST_PX - 1) / INGEST_PX;
    const int rows = std::min(h, INGEST_ROWS);
    dim3 grid((chunks * rows + INGEST_THREADS - 1) / INGEST_THREADS, (h + INGEST_ROWS - 1) / INGEST_ROWS, n);
    hipLaunchKernelGGL(ingest_kernel, grid, dim3(INGEST_THREADS), 0, stream, d_imgs, chunks);
}

}  // namespace svo
