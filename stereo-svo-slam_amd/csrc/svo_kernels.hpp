// svo_kernels.hpp — argument blocks and launchers of the gfx950 kernels.
//
// Every kernel takes a device array of per-sequence argument blocks and uses
// blockIdx.{z|y} as the sequence index, so B independent sequences (one
// StereoSlam instance each) share every launch. A single sequence is B = 1.
#pragma once

#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

#include "../../include/svo_hip.h"
#include "svo_device.hpp"

namespace svo {

// A kernel's dynamic-LDS limit belongs to the device that is current when it is raised: once per
// device and kernel (a second sequence group's thread must not launch before the first has raised it).
// Returns the HIP error of the attribute call, so a failure surfaces at the launch that needs it.
constexpr int SVO_MAX_DEVICES = 64;
struct LdsLimit {
    std::once_flag once[SVO_MAX_DEVICES];
    hipError_t err[SVO_MAX_DEVICES];
};
inline hipError_t raise_lds_limit(LdsLimit& st, const void* kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= SVO_MAX_DEVICES) return hipErrorInvalidDevice;
    std::call_once(st.once[dev], [&st, dev, kernel, bytes] {
        st.err[dev] = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    });
    return st.err[dev];
}

// ---------------------------------------------------------------- pyramids
struct PyrArgs {
    ImgView level[SVO_MAX_PYRAMID_LEVELS];  // halfSample pyramid: [0] = input (or its resident copy), [1..] = outputs
    int n_levels;
    ImgView lk[SVO_LK_LEVELS];              // Gaussian (LK) pyramid: [0] = level[0], [1..] = outputs
    int n_lk;                               // LK levels to build (<= 1: none)
    // optional ingest of device-resident caller images (svo_new_images, SVO_MEM_DEVICE):
    // level[0] is then WRITTEN from src_left while the pyramid is built, and the
    // right image is copied by the blocks with blockIdx.z >= batch.
    ImgView src_left, src_right, dst_right;
};
// both pyramids of `batch` left images of w x h in one launch; right_blocks: extra workgroups copy
// src_right -> dst_right (ingest of device-resident frames)
// stream_rows: 0 if pyr_stream_rows() is 0 for any argument block of the launch (then the tile kernel), else the
// largest of them (the row-streaming kernel with that row block)
void launch_pyr_fused(const PyrArgs* d_args, int batch, int w, int h, bool right_blocks, int stream_rows, hipStream_t stream);
int pyr_stream_rows(const PyrArgs& host_args);

// ------------------------------------------------------------ rectification (rectify.hip)
// cv::remap(src, dst, map_x, map_y, INTER_LINEAR), BORDER_CONSTANT 0, 8-bit (src/app/euroc_input.cpp:69-70)
// in OpenCV's fixed point. A map in the kernels' form: per output pixel, in 64x64 tiles (tile-major, a
// tile's 4096 entries row by row), the integer source position (sx, sy) as two int16 in one dword and
// the 5-bit fractions fx | fy << 5; (sx, sy) are clamped to [-2, REMAP_MAX_SRC] (no tap of a clamped
// entry can fall inside an image of at most REMAP_MAX_SRC pixels a side) and entries without a source
// (non-finite, |m*32| >= 2^31, tile padding) are (-2, -2). box[t] = x0, x1, y0, y1: the bounding box of
// every tap of tile t that can fall inside an image (x0, y0 >= 0; x1 < x0: none).
constexpr int REMAP_TILE = 64;
constexpr int REMAP_MAX_SRC = 16383;
struct RemapMap {
    const uint32_t* xy;
    const uint16_t* frac;
    const int4* box;
    int w, h, tiles_x, tiles_y;
};
struct RemapImg {
    ImgView src, dst;             // dst: w x h of the map
};
// `n` images per side; side s of image i: img[s * n + i] through map[s]
struct RemapLaunch {
    RemapMap map[2];
    const RemapImg* img;
    int n;
};
// device bytes of a w x h map in the kernels' form, and its views on `base` (256-byte aligned)
size_t remap_map_bytes(int w, int h);
RemapMap remap_map_view(void* base, int w, int h);
// float maps (device, dense rows of w floats) -> the kernels' form in `m` (its storage, written)
void launch_remap_prep(const float* map_x, const float* map_y, const RemapMap& m, hipStream_t stream);
// n_sides = 1: map[0] and img[0..n); 2: both sides in one launch
void launch_remap(const RemapLaunch& a, int n_sides, hipStream_t stream);
// A map per image (camera rigs). The images of a launch are ordered by map; a chunk is at most 16 images
// img[s * n + first .. first + count) of one run of equal maps, through the maps whose storage (the `base` of
// remap_map_view) is map[s]. Every map of a launch has the same size.
struct RemapChunk {
    const uint8_t* map[2];
    int first, count;
};
struct RemapMultiLaunch {
    const RemapChunk* chunks;     // device, one per blockIdx.y
    const RemapImg* img;
    int n;                        // images per side
    RemapMap shape;               // (filled by launch_remap_multi: sizes of a w x h map ...
    size_t frac_offset, box_offset;   // ... and where its parts lie in its storage)
};
// images 0..n) sorted by map_of_image (stable) into `order`, and the chunks of that order as (map, first position in
// `order`, count); returns the longest run
struct RemapChunkSpan { int map, first, count; };
int remap_chunks(const int* map_of_image, int n, std::vector<int>& order, std::vector<RemapChunkSpan>& chunks);
// n_chunks <= 65535 chunks of maps of w x h; single_images: every chunk is one image (the kernel form without an
// image loop); n_sides as launch_remap
void launch_remap_multi(RemapMultiLaunch a, int w, int h, int n_chunks, bool single_images, int n_sides, hipStream_t stream);

// Maps from calibrations: cv::initUndistortRectifyMap (src/app/euroc_input.cpp:48-49) in the f64 statement of
// include/svo_hip.h. One camera of a launch: what the kernel reads (uniform per workgroup, only read) and where
// its output goes: two dense float planes (stage form), or the storage of a map in the kernels' form (fused form).
struct RigCam {
    double ir[9];                 // inverse of P R
    double fx, fy, u0, v0;        // of K
    double k1, k2, p1, p2, k3, k4, k5, k6;
    float* map_x;                 // stage form
    float* map_y;
    uint8_t* fixed;               // fused form: the `base` of remap_map_view
};
// ir of the statement (host); false: an input is not finite, or det is 0 or not finite (ir untouched)
bool rectify_inverse(const svo_camera_calibration& cal, double ir[9]);
// the kernel's block of a validated calibration (outputs null); false as rectify_inverse
bool rig_camera(const svo_camera_calibration& cal, RigCam& out);
// n cameras (device table) of w x h in one launch: one workgroup per (64 x 64 tile, camera); tiles * n < RIG_MAX_WORKGROUPS.
// fused = false: the float planes; true: fix5, the packed entries and the tile boxes remap_prep_kernel writes from them
constexpr long long RIG_MAX_WORKGROUPS = 1ll << 23;   // (2^31 lanes in a launch)
void launch_rig_maps(const RigCam* d_cams, int n, int w, int h, bool fused, hipStream_t stream);

// ------------------------------------------------------------ input formats (ingest.hip)
// The per-pixel step of the reference's ImageInput classes: gray from colour (cvtColor's 15-bit fixed point),
// channel extract, and the halves of a side-by-side frame. One output image of the launch:
enum { INGEST_COPY = 0, INGEST_GRAY = 1 };
struct IngestImg {
    ImgView src;                  // the caller's buffer: data, pitch; w x h = the OUTPUT size
    ImgView dst;                  // w x h
    int step;                     // bytes per source pixel: 1 or 3
    int col0;                     // source column of output column 0
    int op;                       // INGEST_COPY: byte `channel` of the pixel; INGEST_GRAY: (sum weight[i] * byte i + 2^14) >> 15
    int channel;
    int weight[3];
};
// one side of an input format: which of the sequence's buffers (0 = left[s], 1 = right[s]), the start column in
// units of the output width, the operation
struct IngestSide {
    int buffer, start, op, channel;
    int weight[3];
};
struct IngestFormat {
    int buffers, channels;        // buffers per sequence (1 or 2), bytes per pixel (1 or 3)
    IngestSide left, right;
};
const IngestFormat* ingest_format(int format);             // SVO_INPUT_*; null: no such format
int ingest_row_pixels(const IngestFormat& f, int w);       // pixels a buffer row holds at least, for outputs of width w
// the table entry of one side (0 left, 1 right) read from `buffer` (pitch `stride`) into dst
IngestImg ingest_image(const IngestFormat& f, int side, const uint8_t* buffer, int stride, const ImgView& dst);
// n output images of w x h (every dst of the table), n <= 65535
void launch_ingest(const IngestImg* d_imgs, int n, int w, int h, hipStream_t stream);

// ------------------------------------------------- sparse image alignment
struct SiaArgs {
    ImgView prev[SVO_MAX_PYRAMID_LEVELS];
    ImgView cur[SVO_MAX_PYRAMID_LEVELS];
    svo_camera_settings cam;
    const int* n_ptr;             // number of keypoints (device)
    const svo_kp2d* kps2d;        // previous frame, full resolution
    const svo_kp3d* kps3d;
    const uint32_t* flags;        // SVO_IGNORE_TEMPORARY => not used
    const float* pose_guess;      // [6]
    float* pose_out;              // [6]
    float* cost_out;              // [1]
    svo_gn_trace* trace;          // [SVO_MAX_PYRAMID_LEVELS] or null
    float* rec_ws;                // workspace [levels used][68][rec_cap]: per-level records of sia_prep_kernel
    int rec_cap;                  // keypoint capacity (row length) of rec_ws, multiple of 4
    float* kp_ws;                 // workspace [9][rec_cap] floats: per-keypoint values of sets that do not fit LDS
    float* dbg_H;                 // optional [36+6+6]: H, b, step of the first get_gradient of `dbg_level`
    int dbg_level;
    int cap;                      // entries of kps2d / flags that may be read (>= *n_ptr): sia_prep_kernel asks for a slot
                                  // before it knows the count and never for one at or past cap
    int exact_pinv;               // 1: reference-order normal equations + the reference's SVD pseudo-inverse (parity mode)
    PoseMats* mats_out;           // optional: rotation matrices of pose_out, for the kernels that project with it
};
// The workgroup shape of an alignment or reprojection-GN launch, a pure host decision (sia_pick_shape,
// reproj_pick_shape): sia_gn_kernel<waves, mode> / reproj_gn_kernel<waves> (mode 0) with `cap` keypoint
// slots per sequence and `lds` bytes of dynamic LDS. fits == false: the keypoints exceed the kernel's
// workspaces, nothing is launched.
struct LaunchShape {
    bool fits;
    int waves, mode, cap;
    size_t lds;
};
// What launch_sia / launch_reproj report: the shape they chose (shape.fits == false: nothing was launched),
// and the error of raising the kernel's LDS limit (the launch itself: hipGetLastError())
struct LaunchStatus {
    LaunchShape shape;
    hipError_t err;
};
// n_bound: upper bound of the keypoint counts of the launch's sequences (chooses the workgroup
// shape); rec_cap: SiaArgs::rec_cap of every block; exact: the value of SiaArgs::exact_pinv in every block (sizes the LDS staging).
LaunchShape sia_pick_shape(int batch, const svo_camera_settings& cam, int width, int height, int n_bound, int rec_cap,
                           int exact);
LaunchStatus launch_sia(const SiaArgs* d_args, int batch, const svo_camera_settings& cam, int width,
                        int height, int n_bound, int rec_cap, int exact, hipStream_t stream);
size_t sia_rec_ws_floats(const svo_camera_settings& cam, int rec_cap);   // size of SiaArgs::rec_ws
// SiaArgs::rec_ws: [levels used][SIA_REC_ROWS][rec_cap] floats, row = field * 16 + patch pixel (fields REC_*), rows
// 64..66 = sum over the patch of gx gx, gx gy, gy gy; sia_prep_kernel alone (launch_sia runs it first)
constexpr int SIA_REC_ROWS = 68;
enum { REC_I1 = 0, REC_PS = 1, REC_G0 = 2, REC_G1 = 3 };
void launch_sia_prep(const SiaArgs* d_args, int batch, const svo_camera_settings& cam, int n_bound, hipStream_t stream);

// --------------------------------------------------------------------- KLT
struct KfDev {                    // one keyframe as the device sees it
    ImgView lk[SVO_LK_LEVELS];    // Gaussian pyramid (unpadded)
    int n_lk;
    float pose[6];
    svo_kp2d* kps2d;              // keyframe->kps.kps2d
    svo_kp3d* kps3d;              // keyframe->kps.kps3d (updated by the depth filter)
    uint32_t* flags;              // ignore_temporary / ignore_completely mirror
    int* outlier_count;
    int* inlier_count;
    // the rest of frame.kps.info as copied at creation (keyframe_manager.cpp:27): read by the getters only
    int* kf_id; int* kp_index; float* score; int* level_type; uint32_t* color; float* kfx; float* kfP;
    int n;
    // KLT template cache (klt.hip): [tmpl_cap][SVO_LK_LEVELS] records of klt_template_bytes(tmpl_win) and their
    // "stored" flags; null when the keyframe has none (stage API, or evicted from the sequence's ring)
    void* tmpl;
    uint8_t* tmpl_valid;
    int tmpl_cap, tmpl_win;
};

struct KltArgs {
    const KfDev* kfs;             // keyframe table: keyframe id in record id & kf_mask
    const int* kf_id;             // [n] origin keyframe of each point (null: all 0)
    ImgView cur[SVO_LK_LEVELS];
    int n_cur;
    const int* n_ptr;
    const svo_kp2d* prev_pts;     // [n] reference positions
    svo_kp2d* cur_pts;            // [n] in: initial flow, out: tracked
    uint8_t* status;              // [n]
    float* err;                   // [n]
    int win;
    int kf_mask;                  // table records - 1 of a ring (the tracker's); -1: the table is indexed by id as it is
    // optional fused projection (tracker path): cur_pts = project(pose, kps3d) first
    const float* proj_pose;       // [6] or null
    const PoseMats* proj_mats;    // optional: pose_mats(proj_pose) computed once per sequence (sia_gn_kernel)
    const svo_kp3d* kps3d;
    svo_kp2d* proj_out;           // [n] projected positions (frame.kps.kps2d before the merge)
    const int* kp_index;          // [n] with proj_pose: prev_pts is gathered from kfs[kf_id].kps2d[kp_index]
    svo_kp2d* ref_out;            // [n] gathered reference points (or null)
    svo_camera_settings cam;
};
void launch_klt(const KltArgs* d_args, int batch, int max_n, int win, hipStream_t stream);
size_t klt_template_bytes(int win);
size_t klt_template_header_offset(int win);      // of the header (state, A11, A12, A22, cI1, cI2) within a record
size_t klt_template_header_bytes();

// ------------------------------------------- merge + reprojection GN (B1,B3)
struct ReprojArgs {
    svo_camera_settings cam;
    const int* n_ptr;
    svo_kp2d* kps2d;              // in: projected, out: merged
    const svo_kp3d* kps3d;
    uint32_t* flags;
    const svo_kp2d* tracked;      // null: skip the merge
    const float* err;
    const float* pose_in;
    float* pose_out;
    float* cost_out;
    svo_gn_trace* trace;          // [1] or null
    int exact_pinv;
    int* zero_out;                // or null: set to 0 (the inside counter filter_update_kernel adds to)
};
LaunchShape reproj_pick_shape(int batch, int n_bound);
LaunchStatus launch_reproj(const ReprojArgs* d_args, int batch, int n_bound, hipStream_t stream);

// project_keypoints (src/lib/transform_keypoints.cpp:11-48) as a stage of its own (the tracker
// fuses it into klt_track_kernel / filter_update_kernel)
void launch_project(const float* pose, const svo_kp3d* kps3d, int n, const svo_camera_settings& cam,
                    svo_kp2d* out, hipStream_t stream);

// ------------------------------------------------------------ depth filter
struct SsdArgs {
    ImgView left, right;
    const int* n_ptr;
    const svo_kp2d* kps2d;
    float* disparity;
    int win, search_x, search_y, clamp_half;
    int first;                    // process kps [first, n)
    const int* first_ptr;         // optional device value added to `first`
    const int* enable;            // optional device predicate
};
// win / search_y: the largest SsdArgs::win / search_y of the launch (choose the LDS size of the kernel)
void launch_ssd(const SsdArgs* d_args, int batch, int max_n, int win, int search_y, hipStream_t stream);
int ssd_pick_max_win(int win, int search_y);       // the largest window of the kernel shape of that launch (31 or 35)

struct FilterArgs {
    svo_camera_settings cam;
    const int* n_ptr;
    const float* frame_pose;      // [6] refined pose
    svo_kp2d* kps2d;              // in: merged positions; out (if reproject): project(pose, kps3d)
    svo_kp3d* kps3d;
    uint32_t* flags;
    int* outlier_count;
    int* inlier_count;
    float* kf_inv_depth;
    float* kf_variance;
    const float* disparity;
    // explicit per-point references (stage API) ...
    const svo_kp3d* ref3d;
    const svo_kp2d* ref2d;
    const float* kf_pose;         // [n*6]
    // ... or the keyframe table (tracker): gathers refs and writes results back
    KfDev* kfs;                   // (keyframe id in record id & kf_mask, as KltArgs)
    const int* kf_id;
    const int* kp_index;
    int kf_mask;
    int do_outlier_check, do_update, do_flags, do_reproject;
    int width, height;
    int* inside_count;            // keyframe_needed numerator (or null)
};
void launch_filter(const FilterArgs* d_args, int batch, int max_n, hipStream_t stream);   // inside_count must be zero

}  // namespace svo
