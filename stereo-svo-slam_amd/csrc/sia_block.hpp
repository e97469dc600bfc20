// sia_block.hpp — the pixel block of sia_prep_kernel (sia.hip), host- and device-callable so that a host
// build can check it at the image borders and at the corners of float (tests/cpp/sia_block_check.cpp).
//
// A lane of sia_prep_kernel owns one patch row pr (four patch pixels) of one keypoint. Everything its
// pixels read of the previous level image lies, unless a float increment of the reference's walk rounds
// across an integer, in SIA_BLK_ROWS rows of SIA_BLK_W bytes: with (bx, by) = floor(keypoint - 2.5) the
// columns bx - 1 .. bx + 6 (the patch sums shifted by -1 and +1 of the four pixels, three taps wide) and
// the rows by - 1 + pr .. by + 3 + pr (the patch sums shifted by -1 and +1, three taps high). The lane
// loads each row with one 8-byte load. A block that crosses a border is moved back inside (columns) or
// repeats the border row (rows): every address it forms is a pixel of the image, and the has-tests
// below say whether the taps of a patch sum or of the cost window are bytes the block really holds —
// otherwise the kernel reads them from the image as the reference does.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SVO_SIA_HD __host__ __device__
#else
#define SVO_SIA_HD
#endif

namespace svo {

constexpr int SIA_BLK_W = 8;        // bytes of a block row
constexpr int SIA_BLK_ROWS = 5;     // rows a lane loads

struct SiaBlock {
    int ox, oy;      // column and row of the image the block is meant to start at (patch row 0)
    int cx0;         // column its rows really start at: ox moved into 0 .. w - SIA_BLK_W
    bool ok;         // the image is wide enough for a block row
};

// floor(v) as an int that later sums cannot overflow; NaN goes to the lower end
SVO_SIA_HD inline int sia_block_floor(float v) { return (int)fminf(fmaxf(floorf(v), -8.f), 65536.f); }

// the block of the keypoint at (x, y) of a level image of w x h (any floats: NaN, infinities, far outside)
SVO_SIA_HD inline SiaBlock sia_block(float x, float y, int w, int h) {
    (void)h;
    SiaBlock b;
    b.ox = sia_block_floor((x - 2.f) - 0.5f) - 1;
    b.oy = sia_block_floor((y - 2.f) - 0.5f) - 1;
    b.ok = w >= SIA_BLK_W;
    const int hi = w - SIA_BLK_W;
    b.cx0 = b.ox < 0 ? 0 : (b.ox > hi ? (hi > 0 ? hi : 0) : b.ox);
    return b;
}

// image row that block row j (0 .. SIA_BLK_ROWS - 1) of patch row pr is loaded from
SVO_SIA_HD inline int sia_block_row(const SiaBlock& b, int pr, int j, int h) {
    const int r = b.oy + pr + j;
    return r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
}

// A patch pixel at column kx shifts its block rows right by this many bytes; byte D of a shifted row is
// then column e - 1 + D, e = sia_block_floor(kx - 0.5). Five bytes are used (D + 0..2, D = 0, 1, 2 for the
// patch sums at kx - 1, kx, kx + 1). Negative: the pixel's columns are not all in the block.
SVO_SIA_HD inline int sia_block_shift(const SiaBlock& b, int e) {
    const int c0 = e - 1 - b.cx0;
    return b.ok && c0 >= 0 && c0 + 4 < SIA_BLK_W ? c0 : -1;
}

// the three tap rows ipy .. ipy + 2 of a patch sum are block rows J .. J + 2 of patch row pr, none of them
// a repeated border row
SVO_SIA_HD inline bool sia_block_has_rows3(const SiaBlock& b, int pr, int J, int ipy, int h) {
    return ipy == b.oy + pr + J && ipy >= 0 && ipy <= h - 3;
}

// Take a patch sum from the block? Its tap origin is (ipx, ipy); sh = sia_block_shift of its pixel, e that pixel's
// column (sia_block_floor(kx - 0.5)); the kernel expects the taps at bytes D .. D + 2 (D = 0, 1, 2 for the sums at
// kx - 1, kx, kx + 1) of the block rows J .. J + 2 (J = 0, 1, 2 for the sums at ky - 1, ky, ky + 1) of patch row pr,
// each shifted right by sh bytes. False: read the image at (ipx, ipy).
SVO_SIA_HD inline bool sia_block_has_sum(const SiaBlock& b, int pr, int sh, int e, int D, int J, int ipx, int ipy, int h) {
    return sh >= 0 && ipx == e - 1 + D && sia_block_has_rows3(b, pr, J, ipy, h);
}

// The cost window with origin (ip1x, ip1y) — rows ip1y + pr and ip1y + pr + 1, columns ip1x .. ip1x + 4 —
// is block rows 2 and 3 of every patch row pr = 0..3, shifted right by the returned number of bytes.
// Negative: it is not all in the block.
SVO_SIA_HD inline int sia_block_window_shift(const SiaBlock& b, int ip1x, int ip1y, int h) {
    const int c1 = ip1x - b.cx0;
    return b.ok && ip1y == b.oy + 2 && ip1y >= 0 && ip1y <= h - 5 && c1 >= 0 && c1 + 4 < SIA_BLK_W ? c1 : -1;
}

}  // namespace svo
