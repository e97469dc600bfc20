// klt_bounds.hpp — the range tests of the KLT kernel (klt.hip), host- and device-callable so that a
// host build can check them at the corners of float and int (tests/cpp/klt_bounds_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define SVO_KLT_HD __host__ __device__
#else
#define SVO_KLT_HD
#endif

namespace svo {

// calcOpticalFlowPyrLK's test of a window's top-left corner (x, y) in an image of w x h, with the
// window of win pixels allowed to hang out by up to win - 1 pixels: floor(x) in [-win, w) and
// floor(y) in [-win, h). Decided in float before any conversion to int: for every finite x of int
// range it is the same test (-win and w are integers), and NaN, +-inf and values beyond int fail it
// (the reference's (int)floorf on x86 turns all of them into INT_MIN; on AMDGPU the conversion
// saturates and takes NaN to 0, which would pass).
SVO_KLT_HD inline bool klt_corner_in_range(float x, float y, int win, int w, int h) {
    return x >= (float)-win && x < (float)w && y >= (float)-win && y < (float)h;
}

// the rectangle of `cols` x `rows` pixels at (x0, y0) lies inside an image of w x h: in int without
// overflow for any x0, y0 (cols, rows, w, h >= 0)
SVO_KLT_HD inline bool klt_rect_in_image(int x0, int y0, int cols, int rows, int w, int h) {
    return x0 >= 0 && y0 >= 0 && x0 <= w - cols && y0 <= h - rows;
}

}  // namespace svo
